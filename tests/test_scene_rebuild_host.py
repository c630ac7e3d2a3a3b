"""phip_scene_rebuild on the CPU: the ABI, and the device pipeline's __host__ __device__ bodies (rebuild_hd.h) run in the kernels' order by
phip_debug_host_rebuild_trace_wide -- Morton keys, a stable sort, the binary radix tree with its bottom-up boxes, the collapse to the 8-wide layout level by level --
followed by the refit of refit_hd.h on the new topology and the CPU twin of the wide traversal.  The arbiter of the hits is the oracle's sweep over all triangles: the
closest hit does not depend on the structure, so (t, u, v, prim) are the same bits whatever tree the rebuild makes.  No GPU needed."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi, scene as S
from test_scene_update_host import FP, U32P, check_boxes, oracle_bruteforce, rays_through, refit_trace, soup

HERE = os.path.dirname(os.path.abspath(__file__))
STACK_LEVELS = 52            # WIDE_STACK_LDS + SPILL_DEPTH / 2 - 2 = 6 + 48 - 2: the deepest wide tree the traversal stacks hold


def rebuild_trace(phip, Pa, Pb, T, rays, camera=None):
    """(hits, info, nodes[n, 20] u32, records[m, 12] f32, rec_prim[m] u32, triangles without a record, rc): the tree is rebuilt on Pb (on Pa when Pb is None)"""
    Pa = np.ascontiguousarray(Pa, np.float32).reshape(-1, 3); T = np.ascontiguousarray(T, np.uint32).reshape(-1, 3)
    keep = [np.ascontiguousarray(a, np.float32) if a is not None else None for a in (Pb, camera)]
    ptr = lambda a: None if a is None else a.ctypes.data_as(FP)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    hits = np.zeros((len(r), 4), np.float32)
    info = A.phip_accel_info(); ndeg = C.c_uint32(0)
    call = lambda n_rays, nodes, recs, prims: phip.phip_debug_host_rebuild_trace_wide(
        Pa.ctypes.data_as(FP), ptr(keep[0]), None, len(Pa), T.ctypes.data_as(U32P), len(T), ptr(keep[1]),
        r.ctypes.data_as(C.POINTER(A.phip_ray)), n_rays, hits.ctypes.data_as(C.POINTER(A.phip_hit)), C.byref(info), nodes, recs, prims, C.byref(ndeg))
    rc = call(0, None, None, None)                    # sizes
    if rc != 0:
        return None, info, None, None, None, 0, rc
    nodes = np.zeros((info.n_nodes, 20), np.uint32); recs = np.zeros((max(info.n_triangle_refs, 1), 12), np.float32); prims = np.zeros(max(info.n_triangle_refs, 1), np.uint32)
    rc = call(len(r), nodes.ctypes.data_as(U32P), recs.ctypes.data_as(FP), prims.ctypes.data_as(U32P))
    return hits, info, nodes, recs[:info.n_triangle_refs], prims[:info.n_triangle_refs], ndeg.value, rc


def non_degenerate(P, T):
    """waldLoad's criterion, restated: the record's denominator b_u c_v - b_v c_u in float32, for the dominant axis k of the float32 normal"""
    P = np.asarray(P, np.float32); tri = P[np.asarray(T, np.int64)]
    A_, B_, C_ = tri[:, 0], tri[:, 1], tri[:, 2]
    b, c = C_ - A_, B_ - A_
    N = np.stack([c[:, 1] * b[:, 2] - c[:, 2] * b[:, 1], c[:, 2] * b[:, 0] - c[:, 0] * b[:, 2], c[:, 0] * b[:, 1] - c[:, 1] * b[:, 0]], axis=1).astype(np.float32)
    k = np.zeros(len(T), np.int64)
    for j in range(3):
        k = np.where(np.abs(N[np.arange(len(T)), j]) > np.abs(N[np.arange(len(T)), k]), j, k)
    u, v = (k + 1) % 3, (k + 2) % 3
    i = np.arange(len(T))
    denom = (b[i, u] * c[i, v]).astype(np.float32) - (b[i, v] * c[i, u]).astype(np.float32)
    return denom.astype(np.float32) != 0


def check_structure(P, T, info, nodes, prims, ndeg):
    """the invariants k_rays_w's node cache and the refit's level ranges rely on; returns the level ranges"""
    valid = non_degenerate(P, T)
    assert ndeg == int((~valid).sum())
    assert sorted(int(p) for p in prims) == [int(i) for i in np.flatnonzero(valid)]          # every non-degenerate triangle in exactly one record, degenerate ones in none
    n, m = len(nodes), len(prims)
    assert n == info.n_nodes >= 1 and m == info.n_triangle_refs
    levels = [0, 1]                              # level l = nodes levels[l] .. levels[l + 1]
    seen_recs = np.zeros(m, np.int64); leaf_slots = 0
    lo = 0
    while lo < levels[-1]:
        hi = levels[-1]
        expect_child = hi                        # the children of a level follow it, in the order of their parents and ranks: breadth first
        for idx in range(lo, hi):
            nd = nodes[idx]
            imask = int(nd[3] >> 24); child_base, tri_base = int(nd[4]), int(nd[5])
            meta = [(int(nd[6 + s // 4]) >> (8 * (s % 4))) & 0xff for s in range(8)]
            off_expect = 0
            for s in range(8):
                if imask & (1 << s):
                    assert meta[s] == (0x20 | (24 + s))
                    child = child_base + bin(imask & ((1 << s) - 1)).count("1")
                    assert child == expect_child, (idx, s)                                   # childBase + rank, inside the next level
                    expect_child += 1
                elif meta[s]:
                    cnt, off = bin(meta[s] >> 5).count("1"), meta[s] & 31
                    assert meta[s] >> 5 in (1, 3, 7) and 1 <= cnt <= 3 and off == off_expect and off + cnt <= 24
                    assert tri_base + off + cnt <= m
                    seen_recs[tri_base + off:tri_base + off + cnt] += 1
                    off_expect += cnt; leaf_slots += 1
            if imask == 0 and not any(meta):
                assert m == 0 and n == 1          # an empty node: only the root of a scene without a valid triangle
        lo = hi
        if expect_child > hi:
            levels.append(expect_child)
    assert levels[-1] == n and all(a < b for a, b in zip(levels, levels[1:]))               # wLevels: increasing, ends at n_nodes
    assert (seen_recs == 1).all()
    assert info.max_depth == len(levels) - 1 <= STACK_LEVELS
    assert info.n_leaves == leaf_slots
    return levels


def check_rebuild(phip, oracle, gauss, P, T, rays, Pa=None, camera=None):
    hits, info, nodes, recs, prims, ndeg, rc = rebuild_trace(phip, P if Pa is None else Pa, None if Pa is None else P, T, rays, camera=camera)
    assert rc == 0, _ffi.debug_lib().phip_last_error()
    want = oracle_bruteforce(oracle, gauss, P, T, rays)
    assert (hits.view(np.uint32) == want.view(np.uint32)).all()
    check_structure(P, T, info, nodes, prims, ndeg)
    if len(prims):
        assert check_boxes(np.asarray(P, np.float32).reshape(-1, 3), np.asarray(T, np.uint32).reshape(-1, 3), nodes, prims, camera=camera) >= info.n_nodes
    # determinism: a second run gives the same node and record arrays
    again = rebuild_trace(phip, P if Pa is None else Pa, None if Pa is None else P, T, rays[:1], camera=camera)
    assert (again[2] == nodes).all() and (again[3].view(np.uint32) == recs.view(np.uint32)).all() and (again[4] == prims).all()
    return hits, want, info, nodes, recs, prims


def mutated_soup():
    """the 6000-triangle soup of test_gpu_scene_update.py (past SPATIAL_MIN_TRIS: the builder splits references) and its `mutate`"""
    Pa, T = soup(np.random.default_rng(17), 6000, 0.3, 8.0)
    Pb = (Pa + 1.6 * np.sin(Pa[:, [1, 2, 0]] * (np.pi / 8.0) + np.array([0.3, 1.1, 2.0]))).astype(np.float32)
    return Pa, Pb, T


def test_abi_of_phip_scene_rebuild(phip, have_gpu):
    assert hasattr(phip, "phip_scene_rebuild")
    header = open(os.path.join(HERE, "..", "include", "phip.h")).read()
    assert "int  phip_scene_rebuild(phip_scene *scene, const phip_update_desc *update /* may be NULL */, phip_update_info *out_info /* may be NULL */);" in header
    assert A.PHIP_ABI_VERSION == 7 and "#define PHIP_ABI_VERSION 7" in header                # an entry point only: no struct of the ABI changed
    assert phip.phip_abi_sizeof(11) == C.sizeof(A.phip_update_desc) and phip.phip_abi_sizeof(12) == C.sizeof(A.phip_update_info)
    assert phip.phip_scene_rebuild.argtypes == phip.phip_scene_update.argtypes == [C.c_void_p, C.POINTER(A.phip_update_desc), C.POINTER(A.phip_update_info)]
    assert phip.phip_scene_rebuild(None, None, None) == A.PHIP_ERR_INVALID
    if not have_gpu:
        never_read = C.create_string_buffer(64)
        info = A.phip_update_info()
        assert phip.phip_scene_rebuild(C.cast(never_read, C.c_void_p), None, C.byref(info)) == A.PHIP_ERR_DEVICE       # no CPU fallback: fails before it looks at the scene
        assert phip.phip_last_error()
    from mitsuba_amd.integrator import Scene
    assert callable(Scene.rebuild) and Scene.rebuild.__code__.co_varnames[:5] == Scene.update.__code__.co_varnames[:5] == ("self", "positions", "normals", "camera", "stream")
    assert ("phip_rebuild.hip", [], "phip_rebuild.o") == _ffi.UNITS[-1] and _ffi.UNITS[-2][2] == "phip_update.o"


def test_rebuild_twin_on_the_mutated_split_soup_and_its_cost_against_the_refit(phip, oracle, gauss):
    Pa, Pb, T = mutated_soup()
    rays = rays_through(np.random.default_rng(5), 20000, -8.0, 8.0)
    hits, want, info, nodes, recs, prims = check_rebuild(phip, oracle, gauss, Pb, T, rays, Pa=Pa)
    assert (want[:, 3].view(np.uint32) != A.PHIP_NO_HIT).mean() > 0.05
    assert info.n_triangle_refs == len(T)                                 # no split references in the new tree
    # every record is the record of its primitive on B, as a fresh host build makes it
    _, _, _, fresh, fresh_prims, _, rc = refit_trace(phip, Pb, None, T, np.zeros((0, 8), np.float32))
    by_prim = {int(p): fresh[i] for i, p in enumerate(fresh_prims) if p != A.PHIP_NO_HIT}
    assert all((recs[i, :11].view(np.uint32) == by_prim[int(p)][:11].view(np.uint32)).all() for i, p in enumerate(prims))
    # the reason the feature exists: on a tree built with spatial splits and refitted to B, the cost explodes; the rebuilt tree's does not (one formula: refitWideNode's)
    _, refit_info, _, _, _, _, rc = refit_trace(phip, Pa, Pb, T, np.zeros((0, 8), np.float32))
    assert rc == 0
    print("soup 6000: sah_cost refitted %.2f, rebuilt %.2f, fresh host build %.2f" % (refit_info.sah_cost, info.sah_cost, refit_trace(phip, Pb, None, T, np.zeros((0, 8), np.float32))[1].sah_cost))
    assert info.sah_cost < refit_info.sah_cost, (info.sah_cost, refit_info.sah_cost)


@pytest.mark.parametrize("n", [65, 70])
def test_rebuild_twin_on_the_smallest_scene_of_the_wide_tree_alone(phip, oracle, gauss, n):
    rng = np.random.default_rng(100 + n)
    P, T = soup(rng, n, 0.8, 4.0)
    check_rebuild(phip, oracle, gauss, P, T, rays_through(rng, 6000, -4.0, 4.0), camera=np.array([0.0, 0.0, -40.0], np.float32))


def test_rebuild_twin_on_300_copies_of_one_triangle(phip, oracle, gauss):
    """all keys equal: the run is told apart by its places in the sorted order, a balanced subtree"""
    rng = np.random.default_rng(31)
    one = np.array([[0.0, 0.0, 0.0], [1.0, 0.2, 0.1], [0.3, 1.1, -0.2]], np.float32)
    P = np.tile(one, (300, 1)); T = np.arange(900, dtype=np.uint32).reshape(300, 3)
    rays = rays_through(rng, 3000, -1.0, 2.0)
    d = np.array([0.45, 0.45, -0.03]) - rays[:1500, :3].astype(np.float64)
    rays[:1500, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    hits, want, info, _, _, _ = check_rebuild(phip, oracle, gauss, P, T, rays)
    assert (hits[:, 3].view(np.uint32) != A.PHIP_NO_HIT).sum() > 1000
    assert info.max_depth <= 1 + 9                                         # ceil(log2 300) = 9 binary levels below the root


def test_rebuild_twin_on_a_geometric_progression_along_one_axis(phip, oracle, gauss):
    """centres at x = 2^-k: every bit of the key's x part splits one triangle off -- the deepest tree 10 bits per axis allow, then one run of equal keys"""
    rng = np.random.default_rng(37)
    k = np.arange(40)
    c = np.stack([2.0 ** -k, np.zeros(40), np.zeros(40)], axis=1)
    tri = np.array([[0.0, -0.5, -0.5], [0.0, 0.5, -0.5], [0.0, 0.0, 0.5]]) * (2.0 ** -(k + 2))[:, None, None]
    P = (c[:, None, :] + tri).astype(np.float32).reshape(-1, 3); T = np.arange(120, dtype=np.uint32).reshape(40, 3)
    rays = rays_through(rng, 4000, -0.1, 1.1)
    rays[:, 1:3] *= 0.01; rays[:, 4:7] = np.array([1.0, 0.0, 0.0], np.float32) * np.where(rng.uniform(size=(4000, 1)) < 0.5, 1.0, -1.0)
    rays[:, 5:7] = rng.normal(scale=0.02, size=(4000, 2))
    rays[:, 4:7] /= np.linalg.norm(rays[:, 4:7], axis=1, keepdims=True)
    hits, want, info, _, _, _ = check_rebuild(phip, oracle, gauss, P, T, rays)
    assert (hits[:, 3].view(np.uint32) != A.PHIP_NO_HIT).mean() > 0.2
    assert info.max_depth <= 31 + 6                                       # 30 key bits, a run of at most 40 equal keys


def test_rebuild_twin_with_2_valid_triangles_of_40_and_with_none(phip, oracle, gauss):
    rng = np.random.default_rng(41)
    P, T = soup(rng, 40, 1.0, 3.0)
    flat = P.reshape(40, 3, 3).copy()
    keep = (7, 29)
    for i in range(40):
        if i not in keep:
            flat[i, 2] = flat[i, 0]                                       # two coincident vertices: no Wald record
    P2 = flat.reshape(-1, 3)
    rays = rays_through(rng, 4000, -3.0, 3.0)
    for j, i in enumerate(keep):
        d = flat[i].astype(np.float64).mean(axis=0) - rays[j * 1000:(j + 1) * 1000, :3].astype(np.float64)
        rays[j * 1000:(j + 1) * 1000, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    hits, want, info, nodes, _, prims = check_rebuild(phip, oracle, gauss, P2, T, rays, Pa=P)      # (created on the healthy soup, rebuilt on the collapsed one)
    assert sorted(prims) == list(keep) and info.n_nodes == 1 and (hits[:, 3].view(np.uint32) != A.PHIP_NO_HIT).sum() > 500
    # ... and the other way round: triangles that had no record get one
    hits, want, info, _, _, prims = check_rebuild(phip, oracle, gauss, P, T, rays, Pa=P2)
    assert len(prims) == 40
    # none: a single empty root, nothing is hit
    flat[list(keep), 2] = flat[list(keep), 0]
    hits, want, info, nodes, _, prims = check_rebuild(phip, oracle, gauss, flat.reshape(-1, 3), T, rays, Pa=P)
    assert info.n_nodes == 1 and info.n_triangle_refs == 0 and len(prims) == 0 and (hits[:, 3].view(np.uint32) == A.PHIP_NO_HIT).all() and (nodes[0, 3] >> 24) == 0 and not nodes[0, 6:8].any()


def test_host_builder_is_what_it_was(phip, gauss):
    """the slot assignment of buildWide is a function the rebuild's collapse shares now: the host builder's trees are the bits recorded before it moved"""
    golden = json.load(open(os.path.join(HERE, "golden", "host_builder_trees.json")))
    sb = S.cornell_box(32, 32, gauss); d = sb.desc()
    Ps, Ts = soup(np.random.default_rng(17), 6000, 0.3, 8.0)
    for name, P, T in (("cornell_box", sb.flat_positions(), np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).copy()), ("soup_6000_seed17", Ps, Ts)):
        _, info, nodes, recs, prims, _, rc = refit_trace(phip, P, None, T, np.zeros((0, 8), np.float32))
        assert rc == 0
        bi = A.phip_accel_info(); box = np.zeros(6, np.float32)
        Pc = np.ascontiguousarray(P, np.float32).reshape(-1, 3); Tc = np.ascontiguousarray(T, np.uint32).reshape(-1, 3)
        assert phip.phip_debug_host_build_bvh(Pc.ctypes.data_as(FP), len(Pc), Tc.ctypes.data_as(U32P), len(Tc), C.byref(bi), box.ctypes.data_as(FP)) == 0
        got = dict(n_nodes=int(bi.n_nodes), n_leaves=int(bi.n_leaves), n_triangle_refs=int(bi.n_triangle_refs), max_depth=int(bi.max_depth),
                   sah_cost_bits=int(np.float32(bi.sah_cost).view(np.uint32)), scene_box_bits=[int(x) for x in box.view(np.uint32)],
                   nodes_sha256=hashlib.sha256(nodes.tobytes()).hexdigest(), records_sha256=hashlib.sha256(recs.tobytes()).hexdigest(), prims_sha256=hashlib.sha256(prims.tobytes()).hexdigest())
        assert got == golden[name], name

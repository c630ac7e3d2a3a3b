"""phip_scene_update on the CPU: the ABI, and the refit itself through phip_debug_host_refit_trace_wide -- the tree is built on positions A and refitted to positions B
(and a camera) by the __host__ __device__ functions the kernels of k_update.h run (refit_hd.h), then walked by the CPU twin of the wide traversal.  The arbiter is the
oracle's sweep over all triangles of B: a refitted tree has conservative boxes, the closest hit does not depend on the structure, so (t, u, v, prim) are the same bits.
No GPU needed."""
import ctypes as C
import os

import numpy as np

from mitsuba_amd import _abi as A, _ffi, scene as S

FP, U32P = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def refit_trace(phip, Pa, Pb, T, rays, camera=None, Pc=None, want_tree=True):
    """(hits, info, nodes[n, 20] u32, records[n, 12] f32, rec_prim[n] u32, n_degenerate, rc)"""
    Pa = np.ascontiguousarray(Pa, np.float32).reshape(-1, 3); T = np.ascontiguousarray(T, np.uint32).reshape(-1, 3)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(FP)
    keep = [np.ascontiguousarray(a, np.float32) if a is not None else None for a in (Pb, Pc, camera)]
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    hits = np.zeros((len(r), 4), np.float32)
    info = A.phip_accel_info(); ndeg = C.c_uint32(0)
    args = lambda n_rays, nodes, recs, prims: phip.phip_debug_host_refit_trace_wide(
        Pa.ctypes.data_as(FP), ptr(keep[0]), ptr(keep[1]), len(Pa), T.ctypes.data_as(U32P), len(T), ptr(keep[2]),
        r.ctypes.data_as(C.POINTER(A.phip_ray)), n_rays, hits.ctypes.data_as(C.POINTER(A.phip_hit)), C.byref(info), nodes, recs, prims, C.byref(ndeg))
    rc = args(0, None, None, None)                    # sizes
    if rc != 0:
        return None, info, None, None, None, 0, rc
    nodes = np.zeros((info.n_nodes, 20), np.uint32); recs = np.zeros((info.n_triangle_refs, 12), np.float32); prims = np.zeros(info.n_triangle_refs, np.uint32)
    rc = args(len(r), nodes.ctypes.data_as(U32P), recs.ctypes.data_as(FP), prims.ctypes.data_as(U32P))
    return hits, info, nodes, recs, prims, ndeg.value, rc


def soup(rng, n, size, extent):
    c = rng.uniform(-extent, extent, (n, 1, 3))
    P = (c + rng.normal(scale=size, size=(n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return P, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def rays_through(rng, n, lo, hi):
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = o; rays[:, 3] = 0.0; rays[:, 4:7] = d; rays[:, 7] = np.inf      # (mint 0: oracle_trace_bruteforce is the plain sweep, without the kd-tree's adaptive epsilon)
    return rays


def oracle_bruteforce(oracle, gauss, P, T, rays):
    sb = S.SceneBuilder()
    sb.mesh(P, T, sb.diffuse((0.5, 0.5, 0.5)))
    sb.perspective((0, 0, -40), (0, 0, 0), (0, 1, 0), 45.0)
    sb.hdrfilm(8, 8, gauss)
    osc = oracle.OracleScene(sb.desc())
    h, _, _ = osc.trace(rays, True, False, bruteforce=True)
    osc.close()
    return h


def check_records(phip, Pb, T, recs, prims):
    """every record of the refitted tree = the record a fresh build (the host builder's waldLoad) makes of its primitive on B"""
    _, _, _, fresh, fresh_prims, _, rc = refit_trace(phip, Pb, None, T, np.zeros((0, 8), np.float32))
    assert rc == 0
    by_prim = {int(p): fresh[i] for i, p in enumerate(fresh_prims) if p != A.PHIP_NO_HIT}
    n = 0
    for i, p in enumerate(prims):
        if p == A.PHIP_NO_HIT:
            continue
        want = by_prim.get(int(p))
        if want is None:                           # degenerate on B: the never-hit record
            assert recs[i, 0].view(np.uint32) == 3 and recs[i, 10].view(np.uint32) == A.PHIP_NO_HIT
        else:
            assert (recs[i].view(np.uint32) == want.view(np.uint32)).all(), (i, p)
            n += 1
    return n


def check_boxes(Pb, T, nodes, prims, camera=None):
    """every dequantised child box contains the padded bounds (Builder::pad) of the triangles below it.  The pad is re-stated here in double.  The code computes it in float:
    its terms carry 2^-23 relative rounding each (allowed for: 1e-3 of the pad), and mn - pad / mx + pad are rounded to float at the magnitude of the coordinate
    (allowed for: one float ulp of the larger |coordinate|).  The quantisation itself is outwards and in double: no allowance"""
    tri = Pb.astype(np.float64)[T.astype(np.int64)]                    # (n, 3, 3)
    tmn, tmx = tri.min(axis=1), tri.max(axis=1)
    ext = (tmx.max(axis=0) - tmn.min(axis=0)).max()
    cam_pad = 4.8e-7 * np.abs(np.asarray(camera, np.float64)).max() if camera is not None else 0.0
    n = len(nodes)
    sub_mn = np.full((n, 3), np.inf); sub_mx = np.full((n, 3), -np.inf)
    checked = 0
    for idx in range(n - 1, -1, -1):                                   # breadth-first order: children have larger indices
        nd = nodes[idx]
        p = nd[0:3].view(np.float32).astype(np.float64)
        e = np.array([(nd[3] >> (8 * a)) & 0xff for a in range(3)], np.int64)
        step = np.ldexp(1.0, e - 127)
        imask = int(nd[3] >> 24); child_base, tri_base = int(nd[4]), int(nd[5])
        meta = [(int(nd[6 + s // 4]) >> (8 * (s % 4))) & 0xff for s in range(8)]
        q = [[(int(nd[8 + 2 * c + s // 4]) >> (8 * (s % 4))) & 0xff for s in range(8)] for c in range(6)]      # qlo.xyz, qhi.xyz
        for s in range(8):
            if meta[s] == 0:
                continue
            lo = p + np.array([q[0][s], q[1][s], q[2][s]]) * step
            hi = p + np.array([q[3][s], q[4][s], q[5][s]]) * step
            if imask & (1 << s):
                child = child_base + bin(imask & ((1 << s) - 1)).count("1")
                assert child > idx
                mn, mx = sub_mn[child], sub_mx[child]
            else:
                cnt, off = bin(meta[s] >> 5).count("1"), meta[s] & 31
                ps = [int(prims[tri_base + off + k]) for k in range(cnt)]
                ps = [x for x in ps if x != A.PHIP_NO_HIT]
                if not ps:
                    continue
                mn, mx = tmn[ps].min(axis=0), tmx[ps].max(axis=0)
                pad = 1e-5 * np.maximum(np.abs(mn), np.abs(mx)) + 1e-7 * (mx - mn) + 2e-6 * ext + cam_pad
                slack = 1e-3 * pad + np.spacing(np.maximum(np.abs(mn), np.abs(mx)).astype(np.float32)).astype(np.float64)
                mn, mx = mn - pad + slack, mx + pad - slack
            assert (lo <= mn).all() and (hi >= mx).all(), (idx, s, lo, mn, hi, mx)
            sub_mn[idx] = np.minimum(sub_mn[idx], mn); sub_mx[idx] = np.maximum(sub_mx[idx], mx)
            checked += 1
    return checked


def test_abi_of_phip_scene_update(phip, have_gpu):
    assert hasattr(phip, "phip_scene_update")
    assert phip.phip_abi_sizeof(11) == C.sizeof(A.phip_update_desc)
    assert phip.phip_abi_sizeof(12) == C.sizeof(A.phip_update_info)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "phip.h")).read()
    assert "int  phip_scene_update(phip_scene *scene, const phip_update_desc *update, phip_update_info *out_info" in header
    assert A.PHIP_ABI_VERSION == 7                                # entry points only: no struct of the ABI changed
    if not have_gpu:
        # no CPU fallback: the call fails loudly before it looks at the scene
        never_read = C.create_string_buffer(64)
        u = A.phip_update_desc(); info = A.phip_update_info()
        rc = phip.phip_scene_update(C.cast(never_read, C.c_void_p), C.byref(u), C.byref(info))
        assert rc == A.PHIP_ERR_DEVICE
        assert phip.phip_last_error()
    assert phip.phip_scene_update(None, None, None) == A.PHIP_ERR_INVALID


def test_refit_twin_on_a_triangle_soup(phip, oracle, gauss):
    """6000 triangles (past SPATIAL_MIN_TRIS: split references, several records per triangle); B = A + a smooth displacement of about a tenth of the extent"""
    rng = np.random.default_rng(17)
    extent = 8.0
    Pa, T = soup(rng, 6000, 0.3, extent)
    Pb = (Pa + 0.1 * 2 * extent * np.sin(Pa[:, [1, 2, 0]] * (2 * np.pi / (2 * extent)) + np.array([0.3, 1.1, 2.0]))).astype(np.float32)
    rays = rays_through(rng, 20000, -extent, extent)
    hits, info, nodes, recs, prims, ndeg, rc = refit_trace(phip, Pa, Pb, T, rays)
    assert rc == 0, phip.phip_last_error()
    assert info.n_triangle_refs > len(T)                          # split references exist
    assert ndeg == 0
    want = oracle_bruteforce(oracle, gauss, Pb, T, rays)
    assert (want[:, 3].view(np.uint32) != A.PHIP_NO_HIT).mean() > 0.05
    assert (hits.view(np.uint32) == want.view(np.uint32)).all()
    assert check_records(phip, Pb, T, recs, prims) == len(prims)
    assert check_boxes(Pb, T, nodes, prims) >= info.n_nodes


def test_refit_twin_on_the_cornell_box_with_a_far_camera(phip, oracle, gauss):
    """the tall block moves, the camera sits 400 scene extents away: the pad's camera term is the refit's, not the build's"""
    sb = S.cornell_box(32, 32, gauss)
    desc = sb.desc()
    T = np.ctypeslib.as_array(desc.indices, shape=(desc.n_triangles, 3)).copy()
    Pa = sb.flat_positions()
    for sid in range(11, 16):
        sb.positions[sid] = (sb.positions[sid] + np.array([-60.0, 0.0, -90.0], np.float32)).astype(np.float32)
    Pb = sb.flat_positions()
    extent = 559.2
    camera = np.array([278.0, 273.0, -400.0 * extent], np.float32)
    rng = np.random.default_rng(23)
    rays = rays_through(rng, 20000, 1.0, 548.0)
    far = rays_through(rng, 4000, 0.0, 1.0)                       # rays from the camera into the room
    target = rng.uniform(0.0, 550.0, (len(far), 3))
    d = target - camera.astype(np.float64)
    far[:, :3] = camera; far[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([rays, far])
    hits, info, nodes, recs, prims, ndeg, rc = refit_trace(phip, Pa, Pb, T, rays, camera=camera)
    assert rc == 0, phip.phip_last_error()
    want = oracle_bruteforce(oracle, gauss, Pb, T, rays)
    assert (want[-len(far):, 3].view(np.uint32) != A.PHIP_NO_HIT).mean() > 0.5
    assert (hits.view(np.uint32) == want.view(np.uint32)).all()
    assert check_records(phip, Pb, T, recs, prims) == len(prims) == len(T)
    assert check_boxes(Pb, T, nodes, prims, camera=camera) >= info.n_nodes


def test_refit_twin_with_a_triangle_collapsed_to_a_line_and_restored(phip, oracle, gauss):
    rng = np.random.default_rng(29)
    Pa, T = soup(rng, 300, 1.0, 5.0)
    victim = 41
    Pb = Pa.copy()
    Pb[T[victim, 2]] = 0.5 * (Pb[T[victim, 0]] + Pb[T[victim, 1]])                 # on the line through the other two: zero area
    Pb[T[victim, 2]] = Pb[T[victim, 0]]                                           # ... exactly: two coincident vertices
    centre = Pa[T[victim]].astype(np.float64).mean(axis=0)
    rays = rays_through(rng, 4000, -5.0, 5.0)
    d = centre - rays[:2000, :3].astype(np.float64)                               # half of the rays aim at the victim
    rays[:2000, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    base = oracle_bruteforce(oracle, gauss, Pa, T, rays)
    assert (base[:, 3].view(np.uint32) == victim).sum() > 100
    # collapsed: the never-hit record
    hits, info, nodes, recs, prims, ndeg, rc = refit_trace(phip, Pa, Pb, T, rays)
    assert rc == 0, phip.phip_last_error()
    assert ndeg == 1
    i = int(np.flatnonzero(prims == victim)[0])
    assert recs[i, 0].view(np.uint32) == 3 and recs[i, 10].view(np.uint32) == A.PHIP_NO_HIT
    assert not (hits[:, 3].view(np.uint32) == victim).any()
    assert (hits.view(np.uint32) == oracle_bruteforce(oracle, gauss, Pb, T, rays).view(np.uint32)).all()
    # restored: the side table still knows the record's primitive, and it hits again
    hits, info, nodes, recs, prims, ndeg, rc = refit_trace(phip, Pa, Pb, T, rays, Pc=Pa)
    assert rc == 0 and ndeg == 0
    assert (hits.view(np.uint32) == base.view(np.uint32)).all()
    assert check_records(phip, Pa, T, recs, prims) == len(prims)
    # the converse is refused: a triangle that was degenerate when the tree was built has no record to refit
    hits, info, nodes, recs, prims, ndeg, rc = refit_trace(phip, Pb, Pa, T, rays)
    assert rc == A.PHIP_ERR_UNSUPPORTED
    assert b"1 triangles" in _ffi.debug_lib().phip_last_error()          # (the hook's library keeps its own error text)

"""phip_scene_rebuild on the GPU: create(A) -> rebuild(B) must be create(B), bit for bit -- sample buffers and films as uint32 and the counters samples, closest_rays,
shadow_rays, path_vertices, invalid_samples, on the device paths the scene admits -- and the oracle's render of B.  The tree is a new one, built on the device, so
node, leaf and record counts may differ from both the creation's and a fresh creation's; the closest hit does not depend on the structure.  Films are 48 x 48 at 4 spp
(the atrium: 64 x 64 at 1 spp)."""
import numpy as np
import pytest

from mitsuba_amd import _abi as A, scene as S
from test_gpu_parity import gpu, random_rays, soup  # noqa: F401  (the fixture)
from test_gpu_scene_update import LIGHT, assert_oracle, assert_same_renders, move_shapes, render, same_bits, soup_scene

pytestmark = pytest.mark.gpu

WIDE_PATHS = (0, A.PHIP_FLAG_NO_FUSED, A.PHIP_FLAG_FUSED_ANY)
STACK_LEVELS = 52


def check_tree(gs, info, n_valid=None):
    a = gs.accel_info()
    assert a.sah_cost == info.sah_cost and info.sah_cost > 1.0 and info.kernel_ms > 0 and info.update_ms >= info.kernel_ms * 0.5
    assert 1 <= a.max_depth <= STACK_LEVELS and a.n_nodes >= 1 and a.n_leaves >= 1
    if n_valid is not None:
        assert a.n_triangle_refs == n_valid                     # one record per non-degenerate triangle: no split references
    return a


def squash_sphere(sb):
    move_shapes(sb, [16], offset=(40.0, 60.0, -30.0), scale=(1.0, 0.6, 1.2))


def test_split_soup_rebuilt_on_moved_vertices(gpu, oracle, gauss):
    """6000 triangles: the creation splits references, the rebuild does not; phip_trace afterwards"""
    rng = np.random.default_rng(17)
    P, T = soup(rng, 6000, size=0.3, extent=8.0)
    sb = soup_scene(gauss, P, T)
    gs = gpu.Scene(sb.desc())
    assert gs.accel_info().n_triangle_refs > 6000
    p = sb.positions[0]
    sb.positions[0] = (p + 1.6 * np.sin(p[:, [1, 2, 0]] * (np.pi / 8.0) + np.array([0.3, 1.1, 2.0]))).astype(np.float32)
    info = gs.rebuild(positions=sb.flat_positions())
    check_tree(gs, info, 6000)
    desc_b = sb.desc(); fresh = gpu.Scene(desc_b)
    integ = gpu.PathHIP(maxDepth=4)
    film, smp, counters = assert_same_renders(gpu, gs, fresh, integ, 4, WIDE_PATHS)
    assert np.isfinite(film).all() and counters[0] == 48 * 48 * 4
    assert_oracle(oracle, desc_b, gs, integ, 4, smp)
    rays = random_rays(rng, 50000, -9, 9, mint=0.0)
    gh, go, _ = gs.rayIntersect(rays, True, True)
    fh, fo, _ = fresh.rayIntersect(rays, True, True)
    assert same_bits(gh, fh) and (go == fo).all()
    osc = oracle.OracleScene(desc_b)
    bh, _, _ = osc.trace(rays[:5000], True, False, bruteforce=True)
    assert same_bits(gh[:5000], bh)
    osc.close()


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_cornell_spheres_sphere_moved_and_squashed(gpu, oracle, gauss, integrator):
    """1088 triangles with vertex normals: k_mega on the (new) 8-wide tree"""
    sb = S.cornell_spheres(48, 48, gauss)
    gs = gpu.Scene(sb.desc())
    squash_sphere(sb)
    info = gs.rebuild(positions=sb.flat_positions(), normals=sb.flat_normals(), camera=sb.camera)
    a = check_tree(gs, info, sb.desc().n_triangles)
    assert a.fused_traversal >= 4
    desc_b = sb.desc(); fresh = gpu.Scene(desc_b)
    integ = gpu.DirectHIP(shadingSamples=2) if integrator == "direct" else gpu.PathHIP(maxDepth=6)
    _, smp, _ = assert_same_renders(gpu, gs, fresh, integ, 4, WIDE_PATHS)
    if integrator == "path":
        assert_oracle(oracle, desc_b, gs, integ, 4, smp)


def test_rebuild_without_arguments_after_a_large_update(gpu, gauss):
    """the split soup refitted far from where it was built, then rebuilt where it is: the cost comes down, the renders stay the update's bits"""
    rng = np.random.default_rng(17)
    P, T = soup(rng, 6000, size=0.3, extent=8.0)
    sb = soup_scene(gauss, P, T)
    gs = gpu.Scene(sb.desc())
    p = sb.positions[0]
    sb.positions[0] = (p + 1.6 * np.sin(p[:, [1, 2, 0]] * (np.pi / 8.0) + np.array([0.3, 1.1, 2.0]))).astype(np.float32)
    refit = gs.update(positions=sb.flat_positions())
    integ = gpu.PathHIP(maxDepth=4)
    before = render(gpu, gs, integ, 4)
    info = gs.rebuild()
    print("soup: sah_cost refitted %.2f rebuilt %.2f; update_ms %.2f rebuild_ms %.2f (kernels %.2f)" % (refit.sah_cost, info.sah_cost, refit.update_ms, info.update_ms, info.kernel_ms))
    assert info.sah_cost < refit.sah_cost, (info.sah_cost, refit.sah_cost)
    check_tree(gs, info, 6000)
    after = render(gpu, gs, integ, 4)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2] == after[2]


def test_a_triangle_that_was_degenerate_at_creation_gets_its_record(gpu, oracle, gauss):
    """the degenerate-at-creation triangle of test_errors_leave_the_scene_unchanged, on a scene of the 8-wide tree (the Cornell box itself has the packed leaf table: below)"""
    rng = np.random.default_rng(17)
    P, T = soup(rng, 300, size=1.0, extent=5.0)
    broken = P.copy(); broken[T[41, 1]] = broken[T[41, 0]]                    # two coincident vertices: no Wald record
    sb = soup_scene(gauss, broken, T)
    gs = gpu.Scene(sb.desc())
    assert gs.accel_info().n_triangle_refs == 299
    with pytest.raises(Exception) as e:
        gs.update(positions=P)
    assert e.value.code == A.PHIP_ERR_UNSUPPORTED and "1 triangles" in str(e.value)
    info = gs.rebuild(positions=P)
    assert info.n_degenerate == 0
    check_tree(gs, info, 300)
    sb.positions[0] = P
    desc = sb.desc(); fresh = gpu.Scene(desc)
    integ = gpu.PathHIP(maxDepth=4)
    _, smp, _ = assert_same_renders(gpu, gs, fresh, integ, 4, WIDE_PATHS)
    assert_oracle(oracle, desc, gs, integ, 4, smp)
    # the bitmap is the new tree's: an update back (the triangle collapses: served, counted) and forth (it returns)
    assert gs.update(positions=broken).n_degenerate == 1
    assert gs.update(positions=P).n_degenerate == 0
    assert_same_renders(gpu, gs, fresh, integ, 4, (0,))


def test_refusals_leave_the_scene_unchanged(gpu, gauss):
    import torch
    sb = S.cornell_spheres(48, 48, gauss)
    gs = gpu.Scene(sb.desc())
    nonormals = gpu.Scene(soup_scene(gauss, *soup(np.random.default_rng(3), 100, size=1.0, extent=5.0)).desc())
    integ = gpu.PathHIP(maxDepth=6)
    before, info_before = render(gpu, gs, integ, 4), gs.accel_info()
    P = sb.flat_positions()
    bad = P.copy(); bad[40, 1] = np.nan
    lf = sum(len(p) for p in sb.positions[:LIGHT[0]])
    flat = P.copy(); flat[lf:lf + len(sb.positions[LIGHT[0]])] = flat[lf]     # the light collapsed to a point: an area emitter without area
    for scene, kw, code in ((gs, dict(positions=bad), A.PHIP_ERR_INVALID), (gs, dict(positions=flat), A.PHIP_ERR_INVALID),
                            (nonormals, dict(normals=np.zeros((300, 3), np.float32)), A.PHIP_ERR_INVALID)):
        with pytest.raises(Exception) as e:
            scene.rebuild(**kw)
        assert getattr(e.value, "code", None) == code, (kw.keys(), e.value)
    # a foreign device pointer: host memory passed as device memory
    u = A.phip_update_desc(); u.positions = P.ctypes.data; u.device_pointers = 1
    import ctypes as C
    assert gs._L.phip_scene_rebuild(gs._h, C.byref(u), None) == A.PHIP_ERR_INVALID
    with pytest.raises(ValueError):
        gs.rebuild(positions=torch.from_numpy(P).cuda().double())
    after, info_after = render(gpu, gs, integ, 4), gs.accel_info()
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2] == after[2]
    assert (info_before.n_nodes, info_before.sah_cost, info_before.n_triangle_refs) == (info_after.n_nodes, info_after.sah_cost, info_after.n_triangle_refs)


def test_torch_tensor_on_a_side_stream_and_a_chain_back(gpu, gauss):
    import torch
    sb = S.cornell_spheres(48, 48, gauss)
    desc_a = sb.desc()
    Pa, Na = sb.flat_positions(), sb.flat_normals()
    untouched, dev = gpu.Scene(desc_a), gpu.Scene(desc_a)
    squash_sphere(sb)
    Pb, Nb = sb.flat_positions(), sb.flat_normals()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tp = torch.from_numpy(Pa).cuda() + torch.from_numpy(Pb - Pa).cuda()      # produced on the caller's stream
        tn = torch.from_numpy(Nb).cuda()
    info = dev.rebuild(positions=tp, normals=tn, stream=stream)
    assert info.kernel_ms > 0
    host = gpu.Scene(desc_a)
    host.rebuild(positions=tp.cpu().numpy(), normals=Nb)
    integ = gpu.PathHIP(maxDepth=6)
    assert_same_renders(gpu, dev, host, integ, 4, (0,))
    a, b = dev.accel_info(), host.accel_info()
    assert (a.n_nodes, a.n_leaves, a.max_depth, a.sah_cost) == (b.n_nodes, b.n_leaves, b.max_depth, b.sah_cost)      # the tree is a function of the input
    # A -> B -> A: the untouched creation, bit for bit
    dev.rebuild(positions=torch.from_numpy(Pa).cuda(), normals=torch.from_numpy(Na).cuda())
    assert_same_renders(gpu, dev, untouched, integ, 4, WIDE_PATHS)


def test_multi_device_replicas_are_refreshed(gpu, gauss):
    sb = S.cornell_spheres(48, 48, gauss)
    gs = gpu.Scene(sb.desc())
    integ = gpu.PathHIP(maxDepth=6)
    kw = dict(flags=A.PHIP_FLAG_ALIAS_DEVICES, devices=[0, 0])
    stale = gpu.HDRFilm(48, 48); assert integ.render(gs, stale, 4, **kw)          # the replica exists, of A
    move_shapes(sb, [17], offset=(-50.0, -80.0, 30.0), scale=(0.7, 1.2, 1.0))
    gs.rebuild(positions=sb.flat_positions(), normals=sb.flat_normals())
    fresh = gpu.Scene(sb.desc())
    a, b = gpu.HDRFilm(48, 48), gpu.HDRFilm(48, 48)
    assert integ.render(gs, a, 4, **kw) and integ.render(fresh, b, 4, **kw)
    assert same_bits(a.storage, b.storage) and not same_bits(a.storage, stale.storage)


def test_a_small_scene_is_served_by_the_update(gpu, oracle, gauss):
    """the Cornell box: 32 records, the packed leaf table -- the counts stay, and so does the update's refusal of its degenerate-at-creation triangle"""
    sb = S.cornell_box(48, 48, gauss)
    gs, twin = gpu.Scene(sb.desc()), gpu.Scene(sb.desc())
    before = gs.accel_info()
    move_shapes(sb, range(11, 16), offset=(-40.0, 0.0, -60.0), rotate_y_deg=25.0)
    info = gs.rebuild(positions=sb.flat_positions())
    twin.update(positions=sb.flat_positions())
    after = gs.accel_info()
    for f in ("n_nodes", "n_leaves", "n_triangle_refs", "max_depth", "fits_lds", "fused_traversal"):
        assert getattr(after, f) == getattr(before, f), f
    assert after.fits_lds == 1 and info.sah_cost == twin.accel_info().sah_cost
    integ = gpu.PathHIP(maxDepth=6)
    _, smp, _ = assert_same_renders(gpu, gs, twin, integ, 4)
    assert_oracle(oracle, sb.desc(), gs, integ, 4, smp)
    broken = S.cornell_box(48, 48, gauss)
    good = broken.positions[7].copy()
    broken.positions[7][1] = broken.positions[7][0]
    small = gpu.Scene(broken.desc())
    broken.positions[7] = good
    with pytest.raises(Exception) as e:
        small.rebuild(positions=broken.flat_positions())
    assert e.value.code == A.PHIP_ERR_UNSUPPORTED


def test_rebuild_of_the_atrium_is_cheaper_than_its_build(gpu, gauss):
    """251 k triangles: a rebuild that is not cheaper than the host build is not the feature"""
    sb = S.atrium(64, 64, gauss, detail=1.0)
    gs = gpu.Scene(sb.desc())
    created = gs.accel_info()
    build_ms = created.build_ms
    rng = np.random.default_rng(3)
    for i in rng.choice(len(sb.positions), len(sb.positions) // 3, replace=False):
        if sb.shapes[i]["emitter"] < 0:
            sb.positions[i] = (sb.positions[i] + rng.uniform(-0.05, 0.05, 3)).astype(np.float32)
    info = gs.rebuild(positions=sb.flat_positions(), normals=sb.flat_normals())
    a = check_tree(gs, info)
    print("atrium: build_ms %.1f rebuild update_ms %.2f kernel_ms %.3f; sah_cost created %.2f rebuilt %.2f; nodes %d -> %d, depth %d -> %d"
          % (build_ms, info.update_ms, info.kernel_ms, created.sah_cost, info.sah_cost, created.n_nodes, a.n_nodes, created.max_depth, a.max_depth))
    assert info.update_ms < build_ms, (info.update_ms, build_ms)
    fresh = gpu.Scene(sb.desc())
    integ = gpu.PathHIP(maxDepth=6)
    assert_same_renders(gpu, gs, fresh, integ, 1, paths=(0,))

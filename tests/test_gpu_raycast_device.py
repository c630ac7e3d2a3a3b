"""phip_trace_device on the GPU (Scene.rayIntersectDevice): rays in, hits, occlusion and surface records out, all in device memory, through the persistent ray
server (k_raycast_p) and k_surfaces.  The closest hit does not depend on the structure or on the order of the tests (winsTie), so everything is compared as
uint32, bit for bit: hits and occlusion with phip_trace on the same rays and -- on the small scene -- with the oracle's sweep over all triangles, the surface
records with the host twin of k_surfaces (tests/test_raycast_device_host.py holds that twin to float64 numpy).  No test here passes a non-finite ray."""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, scene as S
from test_gpu_parity import gpu, random_rays, soup  # noqa: F401  (gpu: the fixture)
from test_gpu_shade_trace_wide import sphere_box, SIZES
from test_gpu_scene_update import move_shapes
from test_raycast_device_host import host_surfaces

pytestmark = pytest.mark.gpu


def u32(t):
    """a result tensor (or None) as a uint32 numpy array"""
    if t is None:
        return None
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint32)


def cast(gs, rays, closest=True, shadow=False, surfaces=False, stream=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()
    h, o, s, st = gs.rayIntersectDevice(t, closest, shadow, surfaces, stream)
    return u32(h), u32(o), u32(s), st


def assert_same_as_host_path(phip, gs, desc, rays, want_surfaces=True):
    """all three outputs of one device call against phip_trace on the same rays and the host twin of k_surfaces on ITS hits"""
    hh, ho, _ = gs.rayIntersect(rays, True, True)
    h, o, s, st = cast(gs, rays, True, True, want_surfaces)
    assert (h == hh.view(np.uint32)).all(), "%d of %d hits differ from phip_trace" % ((h != hh.view(np.uint32)).any(axis=1).sum(), len(rays))
    assert (o == ho).all()
    assert st.closest_rays == len(rays) == st.shadow_rays
    if want_surfaces:
        want = host_surfaces(phip, desc, rays, hh)
        assert (s == want).all(), "%d of %d surface records differ from the host twin" % ((s != want).any(axis=1).sum(), len(rays))
    return hh, ho, st


@pytest.fixture(scope="module")
def cornell(gpu, phip, oracle, gauss):
    """the Cornell box (32 triangles) with the reference answers of 64 * 7 + 13 rays, computed once: phip_trace, the oracle's sweep, the host twin's records"""
    desc = S.cornell_box(32, 32, gauss).desc()
    gs = gpu.Scene(desc)
    rays = random_rays(np.random.default_rng(21), 64 * 7 + 13, -100, 650)      # some start outside the scene box; a few of those miss it
    hh, ho, _ = gs.rayIntersect(rays, True, True)
    osc = oracle.OracleScene(desc); osc.set_bruteforce(True)
    oh, oo, _ = osc.trace(rays, True, True)
    osc.close()
    assert (hh.view(np.uint32)[:, 3] == A.PHIP_NO_HIT).sum() > 0 and ho.sum() > 0 and (ho == 0).sum() > 0
    yield gs, rays, hh.view(np.uint32), ho, oh.view(np.uint32), oo, host_surfaces(phip, desc, rays, hh)
    gs.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 64 * 7 + 13])
def test_cornell_box_every_ray_count_and_every_output(cornell, n):
    gs, rays, hh, ho, oh, oo, hs = cornell
    for closest, shadow, surfaces in ((True, False, False), (False, True, False), (True, False, True), (True, True, True)):
        h, o, s, st = cast(gs, rays[:n], closest, shadow, surfaces)
        assert (h is None) == (not closest) and (o is None) == (not shadow) and (s is None) == (not surfaces)
        if closest:
            assert h.shape == (n, 4) and (h == hh[:n]).all() and (h == oh[:n]).all()
        if shadow:
            assert o.shape == (n,) and (o == ho[:n]).all() and (o == oo[:n]).all()
        if surfaces:
            assert s.shape == (n, 16) and (s == hs[:n]).all()
        assert st.closest_rays == (n if closest else 0) and st.shadow_rays == (n if shadow else 0)


def soup_scene(gauss, P, T):
    sb = S.SceneBuilder()
    sb.mesh(P, T, sb.twosided(sb.diffuse((0.5, 0.5, 0.5)), sb.diffuse((0.2, 0.2, 0.2))))
    sb.perspective((0, 0, -40), (0, 0, 0), (0, 1, 0), 45.0)
    sb.hdrfilm(32, 32, gauss)
    return sb.desc()


def test_rays_of_very_unequal_cost_refill_lanes_mid_chunk(gpu, phip, gauss):
    """every other lane's ray is over at its load (it starts outside the scene box and points away), the others walk a soup of 20 000 triangles: the idle half of
    every wave is refilled from the next chunk while the other half is still in flight"""
    rng = np.random.default_rng(22)
    P, T = soup(rng, 20000)
    desc = soup_scene(gauss, P, T)
    gs = gpu.Scene(desc)
    n = 5000 * 64 + 1
    rays = random_rays(rng, n, -12, 12, mint=0.0)
    out = rays[1::2]
    out[:, :3] = np.sign(out[:, 4:7] + 1e-30) * rng.uniform(20.0, 30.0, (len(out), 3)).astype(np.float32)      # outside the box, every component pointing away
    hh, ho, st = assert_same_as_host_path(phip, gs, desc, rays)
    assert (hh.view(np.uint32)[1::2, 3] == A.PHIP_NO_HIT).all() and (hh.view(np.uint32)[::2, 3] != A.PHIP_NO_HIT).mean() > 0.3
    assert st.closest_node_visits > 0 and st.closest_triangle_tests > 0 and st.trace_kernel_ms > 0
    gs.close()


def test_one_call_large_enough_for_the_static_deal_and_the_draw_counters(gpu, phip, gauss):
    """DrawCounter deals floor(60 % of the chunks / waves of the grid) chunks per wave statically and hands out the rest by its counters.  The grid is at most
    WIDE_WAVES = 7 blocks of 4 waves per CU; with 2 x that many chunks (+ 4, + a partial one) every wave of any grid up to that size takes one static chunk at
    least, and 40 % of the chunks or more are drawn."""
    import torch
    rng = np.random.default_rng(23)
    P, T = soup(rng, 2000)
    desc = soup_scene(gauss, P, T)
    gs = gpu.Scene(desc)
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 7 * 4
    n = 64 * (2 * waves + 4) + 17
    assert (n + 63) // 64 * 60 // 100 >= waves
    rays = random_rays(rng, n, -12, 12, mint=0.0)
    assert_same_as_host_path(phip, gs, desc, rays, want_surfaces=False)
    gs.close()


def test_deep_tree_spills_the_group_stacks_past_their_lds_entries(gpu, phip, gauss):
    """the spine of test_deep_wide_tree_spills_its_group_stack (tests/test_gpu_parity.py): triangles of geometrically growing size along a line make the wide tree far
    deeper than the six group entries a lane keeps in LDS, so the persistent grid's spill region is written and read"""
    rng = np.random.default_rng(5)
    n = 6000
    i = np.arange(n)
    size = 1e-3 * 1.0035 ** i
    centre = np.stack([size * 3.0, np.zeros(n), size * 3.0], 1)
    tri = rng.normal(size=(n, 3, 3)) * size[:, None, None] * 0.7 + centre[:, None, :]
    P = tri.reshape(-1, 3).astype(np.float32)
    T = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    sb = S.SceneBuilder()
    sb.mesh(P, T, sb.twosided(sb.diffuse((0.7, 0.6, 0.5))))
    ext = float(np.abs(P).max())
    sb.perspective((0.3 * ext, 0.5 * ext, -2.0 * ext), (0.3 * ext, 0.0, 0.3 * ext), (0, 1, 0), 50.0, near=1e-4 * ext, far=10 * ext)
    sb.hdrfilm(32, 32, gauss)
    desc = sb.desc()
    gs = gpu.Scene(desc)
    assert gs.accel_info().max_depth >= 10
    rays = random_rays(rng, 4096, -0.2 * ext, 1.2 * ext, mint=0.0)
    rays[:2048, :3] *= 0.01                                      # half of them among the small triangles
    hh, _, _ = assert_same_as_host_path(phip, gs, desc, rays)
    assert (hh.view(np.uint32)[:, 3] != A.PHIP_NO_HIT).sum() > 100
    gs.close()


def test_after_update_and_after_rebuild(gpu, phip, gauss):
    """the sphere box with its spheres moved: the updated and the rebuilt scene answer as a scene created from the new arrays; a second call after the rebuild
    finds the ray cast's plan and buffers on the new tree"""
    sb = sphere_box(gauss, "albedo", *SIZES["104"])
    gs = gpu.Scene(sb.desc())
    rays = random_rays(np.random.default_rng(24), 20000, 0, 550)
    before = cast(gs, rays, True, True, True)
    move_shapes(sb, [16], offset=(60.0, 40.0, -20.0), scale=(1.0, 0.7, 1.2))
    move_shapes(sb, [17], offset=(-80.0, -120.0, -60.0), rotate_y_deg=30.0)
    desc_b = sb.desc()
    fresh = gpu.Scene(desc_b)
    want = cast(fresh, rays, True, True, True)
    assert (want[0] != before[0]).any()
    gs.update(positions=sb.flat_positions(), normals=sb.flat_normals())
    for step in ("update", "rebuild", "second call"):
        got = cast(gs, rays, True, True, True)
        for a, b in zip(got[:3], want[:3]):
            assert (a == b).all(), step
        assert got[3].closest_rays == len(rays)
        if step == "update":
            gs.rebuild()
    assert (want[2] == host_surfaces(phip, desc_b, rays, want[0].view(np.float32))).all()
    gs.close(); fresh.close()


def test_rays_produced_on_a_side_stream(gpu, cornell):
    import torch
    gs, rays, hh, ho, _, _, hs = cornell
    big = np.tile(rays, (200, 1))                                 # enough for the sum to be in flight when the call is made
    half = torch.from_numpy(big * np.float32(0.5)).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = half + half                                           # produced on the caller's stream (x 0.5, + itself: exact)
    h, o, s, st = gs.rayIntersectDevice(t, True, True, True, stream=stream)
    assert (t.cpu().numpy().view(np.uint32) == big.view(np.uint32)).all()
    assert (u32(h) == np.tile(hh, (200, 1))).all() and (u32(o) == np.tile(ho, 200)).all() and (u32(s) == np.tile(hs, (200, 1))).all()


def test_errors_leave_the_scene_usable(gpu, phip, cornell):
    import torch
    gs, rays, hh, ho, _, _, hs = cornell
    n = len(rays)
    t = torch.from_numpy(rays).cuda()
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda"); surf = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    call = lambda r, h, o, s: phip.phip_trace_device(gs._h, r, n, h, o, s, None, None)
    host = np.ascontiguousarray(rays)
    assert call(host.ctypes.data, hits.data_ptr(), None, None) == A.PHIP_ERR_INVALID and phip.phip_last_error()      # a numpy pointer
    assert call(t.data_ptr(), np.zeros((n, 4), np.float32).ctypes.data, None, None) == A.PHIP_ERR_INVALID
    assert call(t.data_ptr(), None, None, surf.data_ptr()) == A.PHIP_ERR_INVALID                                       # surfaces without closest
    with pytest.raises(Exception) as e:
        gs.rayIntersectDevice(t, closest=False, surfaces=True)
    assert getattr(e.value, "code", None) == A.PHIP_ERR_INVALID
    wide = torch.empty((n * 8 + 4,), dtype=torch.float32, device="cuda")
    view = wide[1:1 + n * 8]                                       # a view offset by 4 bytes
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == 4
    assert call(view.data_ptr(), hits.data_ptr(), None, None) == A.PHIP_ERR_INVALID
    assert call(t.data_ptr(), wide[1:1 + n * 4].data_ptr(), None, None) == A.PHIP_ERR_INVALID
    for bad in (t.double(), torch.from_numpy(np.tile(rays, (1, 2))).cuda()[:, :8], torch.from_numpy(rays), t.reshape(-1)):
        with pytest.raises(ValueError):                            # float64, non-contiguous, on the host, not (n, 8)
            gs.rayIntersectDevice(bad)
    h, o, s, st = cast(gs, rays, True, True, True)
    assert (h == hh).all() and (o == ho).all() and (s == hs).all()

"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs.  Bar: per-sample radiance bit-identical for (almost) every sample, and relative
L2 of the developed image <= 1e-3 (BASELINE.json north_star tolerance)."""
import ctypes as C

import os
import numpy as np
import pytest

from conftest import rel_l2
from mitsuba_amd import _abi as A, scene as S

pytestmark = pytest.mark.gpu

TOL_REL_L2 = 1e-3      # north_star: <= 1e-3 relative L2 vs the CPU reference at equal spp


@pytest.fixture(scope="module")
def gpu(phip):
    if phip.phip_device_count() <= 0:
        pytest.fail("no HIP device visible: " + phip.phip_last_error().decode())
    from mitsuba_amd import integrator
    return integrator


def random_rays(rng, n, lo, hi, mint=1e-4):
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = o; rays[:, 3] = mint; rays[:, 4:7] = d; rays[:, 7] = np.inf
    return rays


def soup(rng, n, size=1.0, extent=10.0):
    c = rng.uniform(-extent, extent, (n, 1, 3))
    p = (c + rng.normal(scale=size, size=(n, 3, 3))).astype(np.float32).reshape(-1, 3)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    return p, idx


def compare_render(gpu, oracle, desc, spp, min_identical=0.9999, integrator=None, render_kw=None, paths_min_identical=1.0, **ikw):
    """paths_min_identical: share of the samples on which the scene's device paths (fused / vertex-traced / wavefront) must agree with each other bit for bit -- 1.0 everywhere
    but for the camera 3000 scene extents away (test_far_camera_*), where distances are quantised to an eighth of a scene unit"""
    render_kw = dict(render_kw or {})
    flags_extra = render_kw.pop("flags_extra", 0)            # e.g. PHIP_FLAG_NO_MEGA: which device path renders (not a parameter of the image)
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    gs = Scene(desc)
    integ = (integrator or PathHIP)(**ikw)
    film = HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER | flags_extra, **render_kw)
    gsmp = integ.samples(gs, spp)
    osc = oracle.OracleScene(desc)
    p = integ.params(gs, spp, **render_kw)           # the same phip_render_params the GPU call received (minus the sample-buffer flag)
    ofilm, osmp, ost = osc.render(p, want_samples=True)
    same = (gsmp.view(np.uint32) == osmp.view(np.uint32)).all(axis=-1)
    if desc.n_triangles <= 512 and not same.all():
        # the oracle's kd-tree (= the reference's) and a BVH may disagree on a ray through an edge: an exact-distance tie decided by
        # the kd-tree's leaf order, or a silhouette hit lost at a split plane (HISTORY.md 2.1: ~1e-7 of the samples).  path_hip returns
        # the structure-independent answer, so the bar applies against the oracle answering ray queries by a sweep over all triangles
        assert same.mean() >= min(min_identical, 0.9999), "only %.5f%% of the samples are bit-identical to the kd-tree oracle" % (100 * same.mean())
        osc.set_bruteforce(True)
        ofilm, osmp, ost = osc.render(p, want_samples=True)
        same = (gsmp.view(np.uint32) == osmp.view(np.uint32)).all(axis=-1)
    elif not same.all() and integrator is None and len(np.argwhere(~same)) <= 400:
        # big scenes (a sweep over 250 k triangles per ray for every sample is out of reach): the FEW samples on which path_hip and the
        # kd-tree oracle differ are re-evaluated one by one with the oracle answering its ray queries by that sweep -- each must then
        # be path_hip's value bit for bit: what separates the two is the reference's kd-tree (a silhouette hit lost at a split plane, an
        # exact-distance tie decided by leaf order: HISTORY.md 2.1), not the renderer
        idx = np.argwhere(~same)
        osc.set_bruteforce(True)
        n_equal = sum(int((osc.path_sample(p, int(x), int(y), int(k)).view(np.uint32) == gsmp[y, x, k].view(np.uint32)).all()) for y, x, k in idx)
        osc.set_bruteforce(False)
        print("%d of %d samples differ from the kd-tree oracle; with the oracle answering by a sweep over all triangles %d of them are bit-identical to the GPU"
              % (len(idx), same.size, n_equal))
        assert n_equal == len(idx), (len(idx), n_equal)
    g, o = film.develop(), oracle.develop(ofilm)
    r = rel_l2(g, o) if np.abs(o).max() > 0 else float(np.abs(g).max())
    st = integ.stats
    assert st.samples == gs.width * gs.height * spp == ost.samples
    assert same.mean() >= min_identical, "only %.5f%% of the samples are bit-identical" % (100 * same.mean())
    assert r <= TOL_REL_L2, r
    assert rel_l2(film.storage, ofilm) <= TOL_REL_L2
    assert np.isfinite(film.storage).all()
    # the work counters are the reference's statistics ("Normal rays traced", "Average path length")
    assert abs(int(st.closest_rays) - int(ost.closest_rays)) <= max(4, 1e-4 * ost.closest_rays)
    assert abs(int(st.path_vertices) - int(ost.path_vertices)) <= max(4, 1e-4 * ost.path_vertices)
    assert st.invalid_samples == ost.invalid_samples
    if st.fused or st.vertex_traced:
        # the scene fits LDS, so the fused kernel (k_mega) rendered it -- or its tree is the packed leaf table and k_shade_trace ran the iterations:
        # the wavefront kernels (k_shade -> k_shadow_p -> k_trace) must give the same bits
        film2 = HDRFilm(gs.width, gs.height)
        assert integ.render(gs, film2, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER | A.PHIP_FLAG_NO_FUSED, **render_kw)
        assert not integ.stats.fused and not integ.stats.vertex_traced
        wsmp = integ.samples(gs, spp)
        agree = (wsmp.view(np.uint32) == gsmp.view(np.uint32)).all(axis=-1).mean()
        assert agree >= paths_min_identical, "fused and wavefront paths differ (%.6f of the samples agree)" % agree
        if paths_min_identical >= 1.0:
            assert (film2.storage.view(np.uint32) == film.storage.view(np.uint32)).all()
            assert integ.stats.samples == st.samples and integ.stats.path_vertices == st.path_vertices
            assert integ.stats.closest_rays == st.closest_rays and integ.stats.shadow_rays == st.shadow_rays
        # ... and the wavefront kernels against the oracle on their own
        assert (wsmp.view(np.uint32) == osmp.view(np.uint32)).all(axis=-1).mean() >= min_identical
    ai = gs.accel_info()
    if not st.fused and ai.fused_traversal >= 4 and not (flags_extra & (A.PHIP_FLAG_NO_FUSED | A.PHIP_FLAG_NO_MEGA)):
        # round 6: the scene's tree is past the size where the fused kernel is the default (PHIP_FUSED_WIDE_MAX_NODES), but k_mega can walk it from memory
        # (k_wide_wave.h): the same bits, the same counters
        film3 = HDRFilm(gs.width, gs.height)
        assert integ.render(gs, film3, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER | A.PHIP_FLAG_FUSED_ANY | flags_extra, **render_kw)
        assert integ.stats.fused
        fsmp = integ.samples(gs, spp)
        assert (fsmp.view(np.uint32) == gsmp.view(np.uint32)).all(), "the fused kernel on the 8-wide tree and the wavefront kernels differ"
        assert (film3.storage.view(np.uint32) == film.storage.view(np.uint32)).all()
        assert integ.stats.samples == st.samples and integ.stats.path_vertices == st.path_vertices
        assert integ.stats.closest_rays == st.closest_rays and integ.stats.shadow_rays == st.shadow_rays
    gs.close(); osc.close()
    return same.mean(), r


def test_raycast_cornell_bit_identical(gpu, oracle, gauss):
    desc = S.cornell_box(64, 64, gauss).desc()
    gs = gpu.Scene(desc); osc = oracle.OracleScene(desc)
    rays = random_rays(np.random.default_rng(1), 100000, 0, 550)
    gh, go, _ = gs.rayIntersect(rays, True, True)
    oh, oo, _ = osc.trace(rays, True, True)
    assert (gh.view(np.uint32) == oh.view(np.uint32)).all()
    assert (go == oo).all()


def test_raycast_triangle_soup_vs_oracle_and_bruteforce(gpu, oracle, gauss):
    """the test_kd workload shape (random chords through a mesh), structure-independent answer"""
    rng = np.random.default_rng(2)
    p, idx = soup(rng, 20000)
    sb = S.SceneBuilder()
    m = sb.diffuse((0.5, 0.5, 0.5))
    sb.mesh(p, idx, m)
    sb.perspective((0, 0, -40), (0, 0, 0), (0, 1, 0), 45.0)
    sb.hdrfilm(32, 32, gauss)
    desc = sb.desc()
    gs = gpu.Scene(desc); osc = oracle.OracleScene(desc)
    rays = random_rays(rng, 50000, -12, 12, mint=0.0)
    gh, go, gst = gs.rayIntersect(rays, True, True)
    oh, oo, _ = osc.trace(rays, True, True)
    bh, _, _ = osc.trace(rays[:2000], True, False, bruteforce=True)
    same = (gh.view(np.uint32) == oh.view(np.uint32)).all(axis=1)
    assert same.mean() > 0.9999, same.mean()
    assert (go == oo).mean() > 0.9999
    assert ((gh[:2000].view(np.uint32) == bh.view(np.uint32)).all(axis=1)).mean() > 0.999
    assert gst.closest_node_visits > 0 and gst.closest_triangle_tests > 0


@pytest.mark.parametrize("cfg", [
    dict(maxDepth=4), dict(maxDepth=-1), dict(maxDepth=1), dict(maxDepth=2), dict(maxDepth=-1, rrDepth=2),
    dict(maxDepth=6, strictNormals=True), dict(maxDepth=5, hideEmitters=True),
])
def test_cornell_render_matches_oracle(gpu, oracle, gauss, cfg):
    desc = S.cornell_box(96, 96, gauss).desc()
    compare_render(gpu, oracle, desc, 8, **cfg)


def test_cornell_c1_config(gpu, oracle, gauss):
    """BASELINE.json configs[0]: Cornell 256x256, 16 spp, maxDepth=4"""
    desc = S.cornell_box(256, 256, gauss).desc()
    same, r = compare_render(gpu, oracle, desc, 16, maxDepth=4)
    print("C1: identical %.6f rel L2 %.3e" % (same, r))


def test_ragged_image_and_crop_window(gpu, oracle, gauss):
    sb = S.cornell_box(150, 70, gauss)          # not a multiple of the block size
    compare_render(gpu, oracle, sb.desc(), 4, maxDepth=5)
    sb = S.cornell_box(128, 128, gauss)
    sb.hdrfilm(128, 128, gauss, crop=(37, 21, 50, 45))
    compare_render(gpu, oracle, sb.desc(), 4, maxDepth=5)


@pytest.mark.parametrize("bs", [8, 16, 64])
def test_block_sizes(gpu, oracle, gauss, bs):
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    desc = S.cornell_box(100, 60, gauss).desc()
    gs = Scene(desc); gs.setBlockSize(bs)
    integ = PathHIP(maxDepth=4); film = HDRFilm(100, 60)
    assert integ.render(gs, film, 4)
    osc = oracle.OracleScene(desc)
    ofilm, _, _ = osc.render(A.default_render_params(spp=4, max_depth=4, block_size=bs))
    assert rel_l2(film.storage, ofilm) < 1e-5


def test_shards_sum_to_the_whole_image(gpu, oracle, gauss):
    """block sharding (multi-GPU path): the sum of all shards' films equals the unsharded render"""
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    desc = S.cornell_box(160, 96, gauss).desc()
    gs = Scene(desc)
    integ = PathHIP(maxDepth=5)
    whole = HDRFilm(160, 96); assert integ.render(gs, whole, 4)
    acc = HDRFilm(160, 96)
    n = 3
    for r in range(n):
        part = HDRFilm(160, 96)
        assert integ.render(gs, part, 4, shard_index=r, shard_count=n)
        assert part.storage[..., 4].sum() > 0
        acc.put(part.storage)
        osc = oracle.OracleScene(desc)
        ofilm, _, _ = osc.render(A.default_render_params(spp=4, max_depth=5, shard_index=r, shard_count=n))
        assert rel_l2(part.storage, ofilm) < 1e-5
    assert rel_l2(acc.storage, whole.storage) < 1e-6
    assert np.abs(acc.storage[..., 4] - whole.storage[..., 4]).max() < 1e-4


def test_seed_changes_the_image_and_is_reproducible(gpu, gauss):
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    gs = Scene(S.cornell_box(64, 64, gauss).desc())
    integ = PathHIP(maxDepth=4)
    a = HDRFilm(64, 64); b = HDRFilm(64, 64); c = HDRFilm(64, 64)
    integ.render(gs, a, 4, seed=1); integ.render(gs, b, 4, seed=1); integ.render(gs, c, 4, seed=2)
    assert (a.storage == b.storage).all()          # deterministic: no float atomics on the film
    assert not (a.storage == c.storage).all()


def test_empty_scene_and_no_emitters(gpu, oracle, gauss):
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    sb = S.SceneBuilder()
    sb.diffuse((0.5, 0.5, 0.5))
    sb.perspective((0, 0, -5), (0, 0, 0), (0, 1, 0), 45.0)
    sb.hdrfilm(40, 24, gauss)
    gs = Scene(sb.desc())
    film = HDRFilm(40, 24)
    assert PathHIP().render(gs, film, 2)
    assert (film.storage[..., :4] == 0).all() and (film.storage[..., 4] > 0).all()
    # geometry but no light: alpha only
    sb = S.SceneBuilder(); m = sb.diffuse((0.5, 0.5, 0.5))
    sb.quad((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0), m, facing=(0, 0, -1))
    sb.perspective((0, 0, -5), (0, 0, 0), (0, 1, 0), 45.0)
    sb.hdrfilm(40, 24, gauss)
    compare_render(gpu, oracle, sb.desc(), 2, min_identical=1.0)


def test_error_behaviour(gpu, phip, gauss):
    """integrator.cpp:219-224 messages; bad arguments return an error code, never crash"""
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    from mitsuba_amd import _ffi
    with pytest.raises(RuntimeError, match="rrDepth"):
        PathHIP(rrDepth=0)
    with pytest.raises(RuntimeError, match="maxDepth"):
        PathHIP(maxDepth=0)
    gs = Scene(S.cornell_box(32, 32, gauss).desc())
    p = A.default_render_params(spp=0)
    out = np.zeros((32, 32, 5), np.float32)
    assert phip.phip_render(gs._h, C.byref(p), _ffi.fptr(out), None) == A.PHIP_ERR_INVALID
    p = A.default_render_params(spp=1, max_depth=0)
    assert phip.phip_render(gs._h, C.byref(p), _ffi.fptr(out), None) == A.PHIP_ERR_INVALID
    assert b"maxDepth" in phip.phip_last_error()
    p = A.default_render_params(spp=1, shard_index=2, shard_count=2)
    assert phip.phip_render(gs._h, C.byref(p), _ffi.fptr(out), None) == A.PHIP_ERR_INVALID
    d = S.cornell_box(32, 32, gauss).desc()
    d.abi_version = 99
    assert not phip.phip_scene_create(C.byref(d), 0)
    d = S.cornell_box(32, 32, gauss).desc()
    assert not phip.phip_scene_create(C.byref(d), 99)


def test_cancel_returns_false(gpu, gauss):
    import threading, time
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    gs = Scene(S.cornell_box(1024, 1024, gauss).desc())
    integ = PathHIP(maxDepth=-1)
    film = HDRFilm(1024, 1024)
    assert integ.render(gs, film, 1)         # (warm-up: allocations, so that the timed render below is all kernel time)
    integ._scene = gs
    t = threading.Timer(0.05, integ.cancel); t.start()
    ok = integ.render(gs, film, 2048)        # 2.1 G samples: ~0.7 s at 3 G samples/s -- the request arrives in the middle
    t.join()
    assert ok is False                       # SamplingIntegrator::render returns false when cancelled
    film2 = HDRFilm(1024, 1024)
    assert integ.render(gs, film2, 1) is True   # the scene is reusable afterwards


def test_atrium_sponza_class_matches_oracle(gpu, oracle, gauss):
    """BASELINE.json configs[2] scene (reduced film): ~250k triangles, twosided diffuse + roughconductor, smooth normals"""
    desc = S.atrium(240, 136, gauss).desc()
    same, r = compare_render(gpu, oracle, desc, 4, min_identical=0.999, maxDepth=8)
    print("atrium: identical %.6f rel L2 %.3e" % (same, r))


def test_glass_room_matches_oracle(gpu, oracle, gauss):
    """BASELINE.json configs[3] scene (reduced film): dielectric chains, maxDepth=16"""
    desc = S.glass_room(240, 136, gauss).desc()
    same, r = compare_render(gpu, oracle, desc, 4, min_identical=0.999, maxDepth=16)
    print("glass_room: identical %.6f rel L2 %.3e" % (same, r))


def test_material_zoo_matches_oracle(gpu, oracle, gauss):
    """every BSDF variant on the path in one Cornell box: ggx / anisotropic / non-visible sampling, dielectric, twosided(front, back)"""
    from test_oracle_path import sphere_uvs
    sb = S.cornell_box(128, 128, gauss)
    cu = dict(eta=S.CU_ETA, k=S.CU_K)
    mats = [sb.twosided(sb.roughconductor(alpha=0.2, distribution="ggx", **cu)),
            sb.twosided(sb.roughconductor(alpha=0.05, alpha_v=0.3, **cu)),
            sb.twosided(sb.roughconductor(alpha=0.15, sample_visible=False, **cu), sb.diffuse((0.2, 0.7, 0.3))),
            sb.roughconductor(alpha=0.3, **cu),
            sb.dielectric(1.33, 1.0)]
    for i, m in enumerate(mats):
        P, T, N = S.sphere_mesh((90 + 95 * i, 420 - 60 * (i % 2), 150 + 60 * i), 45.0, 24, 12)
        sb.mesh(P, T, m, normals=N, uvs=sphere_uvs(N))           # anisotropic BSDFs need texture coordinates (trimesh.cpp:683-693)
    compare_render(gpu, oracle, sb.desc(), 8, min_identical=0.999, maxDepth=8)


def test_constant_environment_matches_oracle(gpu, oracle, gauss):
    """the `constant` environment emitter (constant.cpp; path.cpp:136-143, 233-265)"""
    # (a) smooth-shaded spheres (diffuse, twosided diffuse -> uniform-sphere NEE, copper, glass) on a floor, environment only
    sb = S.SceneBuilder()
    floor = sb.diffuse((0.4, 0.45, 0.5))
    mats = [sb.diffuse((0.7, 0.3, 0.2)), sb.twosided(sb.diffuse((0.2, 0.6, 0.3))),
            sb.roughconductor(alpha=0.2, eta=S.CU_ETA, k=S.CU_K), sb.dielectric(1.5, 1.0)]
    sb.quad((-6, 0, -6), (6, 0, -6), (6, 0, 6), (-6, 0, 6), floor, facing=(0, 1, 0))
    for i, m in enumerate(mats):
        P, T, N = S.sphere_mesh((-3 + 2 * i, 0.8, 0.5 * (i % 2)), 0.8, 24, 12)
        sb.mesh(P, T, m, normals=N)
    sb.constant((0.9, 1.0, 1.2))
    sb.perspective((0, 3, -9), (0, 0.5, 0), (0, 1, 0), 40.0)
    sb.hdrfilm(160, 96, gauss)
    same, r = compare_render(gpu, oracle, sb.desc(), 8, min_identical=0.999, maxDepth=8)
    print("env spheres: identical %.6f rel L2 %.3e" % (same, r))
    compare_render(gpu, oracle, sb.desc(), 4, min_identical=0.999, maxDepth=8, hideEmitters=True)
    compare_render(gpu, oracle, sb.desc(), 4, min_identical=0.999, maxDepth=3, strictNormals=True)
    # (b) Cornell box (area light) + environment with a different sampling weight: two emitters in the selection PDF
    sb = S.cornell_box(128, 128, gauss)
    sb.constant((0.3, 0.3, 0.5), sampling_weight=0.5)
    compare_render(gpu, oracle, sb.desc(), 8, min_identical=0.9999, maxDepth=6)
    # (c) nothing but the environment
    sb = S.SceneBuilder(); sb.diffuse((0.5, 0.5, 0.5)); sb.constant((0.25, 0.5, 1.0))
    sb.perspective((0, 0, -5), (0, 0, 0), (0, 1, 0), 45.0); sb.hdrfilm(40, 24, gauss)
    compare_render(gpu, oracle, sb.desc(), 2, min_identical=1.0)


def test_environment_error_behaviour(gpu, phip, gauss):
    sb = S.SceneBuilder(); sb.diffuse((0.5, 0.5, 0.5)); sb.constant((1, 1, 1)); sb.constant((2, 2, 2))
    sb.perspective((0, 0, -5), (0, 0, 0), (0, 1, 0), 45.0); sb.hdrfilm(8, 8, gauss)
    d = sb.desc()
    assert not phip.phip_scene_create(C.byref(d), 0)
    assert b"one environment emitter" in phip.phip_last_error()


@pytest.mark.parametrize("stddev", [0.25, 0.5, 1.0, 1.5])
def test_reconstruction_filter_widths(gpu, oracle, gauss, stddev):
    """filters of reach 1 .. 6 pixels: k_film_tiled<2>, k_film_tiled<4> and the generic k_film gather
    (rfilter.cpp:38-57 discretisation, imageblock.h:124-204 splat); also a box-like table"""
    from mitsuba_amd import _ffi
    ft = _ffi.gaussian_filter(stddev)
    sb = S.cornell_box(96, 80, ft)
    compare_render(gpu, oracle, sb.desc(), 4, min_identical=1.0, maxDepth=4)
    if stddev == 0.5:
        box = (0.5, [1.0] * 31 + [0.0])       # box filter: radius 0.5, constant table (rfilters/box.cpp)
        sb = S.cornell_box(96, 80, box)
        compare_render(gpu, oracle, sb.desc(), 4, min_identical=1.0, maxDepth=4)


def test_large_emitter_mesh_and_many_materials(gpu, oracle, gauss):
    """tables that do not fit the LDS staging of k_shade: a 1 200-triangle smooth-shaded mesh light (area CDF and
    emitter records stay in global memory) plus a flat-shaded one, and 60 materials (> MATERIAL_LDS_MAX)"""
    sb = S.cornell_box(128, 128, gauss)
    black = sb.diffuse((0, 0, 0))
    P, T, N = S.sphere_mesh((278, 300, 280), 40.0, 30, 20)
    sb.mesh(P, T, black, normals=N, radiance=(6.0, 5.0, 3.0))
    P, T, N = S.sphere_mesh((120, 120, 150), 25.0, 12, 8)
    sb.mesh(P, T, black, radiance=(2.0, 4.0, 8.0), sampling_weight=0.3)
    rng = np.random.default_rng(5)
    for i in range(60):
        m = sb.diffuse(tuple(rng.uniform(0.1, 0.9, 3))) if i % 3 else sb.twosided(sb.roughconductor(alpha=float(rng.uniform(0.05, 0.4)), eta=S.CU_ETA, k=S.CU_K))
        P, T, N = S.sphere_mesh((60 + 45 * (i % 10), 40 + 60 * (i // 10), 420 + 8 * (i % 7)), 18.0, 10, 6)
        sb.mesh(P, T, m, normals=N if i % 2 else None)
    compare_render(gpu, oracle, sb.desc(), 8, min_identical=0.999, maxDepth=6)


def test_envmap_matches_oracle(gpu, oracle, phip, gauss):
    """SURVEY 8(f) row 1, second half: the `envmap` emitter's illumination (envmap.cpp:516-632, 380-394)"""
    from test_oracle_path import _sky, _rot
    tex = _sky(96, 48)

    def scene(to_world=None, weight=1.0, extra_light=False, res=(160, 96)):
        sb = S.SceneBuilder()
        floor = sb.diffuse((0.4, 0.45, 0.5))
        mats = [sb.diffuse((0.7, 0.3, 0.2)), sb.twosided(sb.diffuse((0.2, 0.6, 0.3))),
                sb.roughconductor(alpha=0.2, eta=S.CU_ETA, k=S.CU_K), sb.dielectric(1.5, 1.0)]
        sb.quad((-6, 0, -6), (6, 0, -6), (6, 0, 6), (-6, 0, 6), floor, facing=(0, 1, 0))
        for i, m in enumerate(mats):
            P, T, N = S.sphere_mesh((-3 + 2 * i, 0.8, 0.5 * (i % 2)), 0.8, 24, 12)
            sb.mesh(P, T, m, normals=N)
        if extra_light:
            sb.quad((-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1), sb.diffuse((0, 0, 0)), facing=(0, -1, 0), radiance=(8, 8, 6))
        sb.envmap(tex, scale=0.8, to_world=to_world, sampling_weight=weight)
        sb.perspective((0, 3, -9), (0, 0.5, 0), (0, 1, 0), 40.0)
        sb.hdrfilm(res[0], res[1], gauss)
        return sb
    same, r = compare_render(gpu, oracle, scene().desc(), 8, min_identical=0.999, maxDepth=8, hideEmitters=True)
    print("envmap: identical %.6f rel L2 %.3e" % (same, r))
    compare_render(gpu, oracle, scene(_rot((1, 0.3, 0.2), 70.0), 0.5, True).desc(), 8, min_identical=0.999, maxDepth=6, hideEmitters=True)
    compare_render(gpu, oracle, scene(_rot((0, 1, 0), 200.0)).desc(), 4, min_identical=0.999, maxDepth=3, hideEmitters=True, strictNormals=True)
    # directly visible background: refused unless the deviation is asked for
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    gs = Scene(scene(res=(64, 40)).desc())
    integ = PathHIP(maxDepth=4); film = HDRFilm(64, 40)
    with pytest.raises(RuntimeError, match="hideEmitters"):
        integ.render(gs, film, 2)
    assert integ.render(gs, film, 2, flags=A.PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND)
    osc = oracle.OracleScene(scene(res=(64, 40)).desc())
    ofilm = osc.render(A.default_render_params(spp=2, max_depth=4, flags=A.PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND))[0]
    assert rel_l2(film.storage, ofilm) < 1e-5


def test_envmap_filtered_background_matches_oracle(gpu, oracle, gauss):
    """directly visible environment pixels: camera-ray differentials (perspective.cpp:159-163,293-294, scaled by
    1/sqrt(spp), integrator.cpp:144-145) and the EWA-filtered lookup over the MIP pyramid (envmap.cpp:395-407,
    mipmap.h:629-833): trilinear fallback, anisotropy clamp, EWA ellipse -- all exercised by a 1024 x 512 map seen
    through a coarse film"""
    from test_oracle_path import _sky, _rot
    rng = np.random.default_rng(3)
    tex = (_sky(1024, 512) * rng.uniform(0.5, 1.5, (512, 1024, 1))).astype(np.float32)
    for res, fov, spp, R in (((48, 32), 70.0, 1, None), ((64, 40), 100.0, 4, _rot((1, 0.3, 0.2), 70.0)), ((40, 40), 25.0, 16, _rot((0, 0, 1), 90.0))):
        sb = S.SceneBuilder(); m = sb.diffuse((0.5, 0.4, 0.3))
        P, T, N = S.sphere_mesh((0, 0, 0), 1.0, 16, 8)
        sb.mesh(P, T, m, normals=N)
        sb.envmap(tex, scale=1.5, to_world=R, pyramid=True)
        sb.perspective((0, 0.5, -5), (0, 0, 0), (0, 1, 0), fov)
        sb.hdrfilm(res[0], res[1], gauss)
        same, r = compare_render(gpu, oracle, sb.desc(), spp, min_identical=0.999, maxDepth=4)
        print("envmap background %s fov %g: identical %.6f rel L2 %.3e" % (res, fov, same, r))


def test_bitmap_textures_match_oracle(gpu, oracle, gauss):
    """bitmap reflectance textures (EWA / trilinear / bilinear / nearest, wrap modes, uv scale and
    offset), UV tangents in the shading frame (also for untextured, anisotropic materials), first-vertex UV partials"""
    from test_oracle_path import sphere_uvs, checker
    rng = np.random.default_rng(11)
    noise = rng.uniform(0.05, 0.95, (96, 160, 3)).astype(np.float32)
    chk = checker(256, 32)

    def scene(res=(160, 112), light=True):
        sb = S.SceneBuilder()
        t_floor = sb.bitmap(chk, filter_type="ewa", uscale=6.0, vscale=6.0)
        t_tri = sb.bitmap(noise, filter_type="trilinear", wrap="mirror", wrap_v="clamp", uscale=2.0, uoffset=0.3)
        t_bil = sb.bitmap(noise, filter_type="bilinear", wrap="zero", wrap_v="one", uscale=1.5, vscale=1.5, voffset=-0.2)
        t_near = sb.bitmap(chk[:64, :48], filter_type="nearest", max_anisotropy=4.0)
        t_ewa4 = sb.bitmap(noise[:50, :70], filter_type="ewa", max_anisotropy=2.0, uscale=3.0)
        floor = sb.diffuse(texture=t_floor)
        sb.quad((-8, 0, -8), (8, 0, -8), (8, 0, 8), (-8, 0, 8), floor, facing=(0, 1, 0), uvs=True)
        mats = [sb.diffuse(texture=t_tri), sb.twosided(sb.diffuse(texture=t_bil)), sb.twosided(sb.diffuse(texture=t_near), sb.diffuse((0.3, 0.3, 0.3))),
                sb.diffuse(texture=t_ewa4), sb.roughconductor(alpha=0.05, alpha_v=0.3, eta=S.CU_ETA, k=S.CU_K), sb.diffuse((0.6, 0.5, 0.4))]
        for i, m in enumerate(mats):
            P, T, N = S.sphere_mesh((-5 + 2 * i, 0.8, 0.4 * (i % 2)), 0.8, 24, 12)
            smooth = i % 2 == 0
            sb.mesh(P, T, m, normals=N if smooth else None, uvs=sphere_uvs(N))           # texcoords: the frame uses the UV tangents
        if light:
            sb.quad((-2, 5, -2), (2, 5, -2), (2, 5, 2), (-2, 5, 2), sb.diffuse((0, 0, 0)), facing=(0, -1, 0), radiance=(10, 10, 9))
        sb.constant((0.4, 0.5, 0.7))
        sb.perspective((0, 3.5, -11), (0, 0.4, 0), (0, 1, 0), 42.0)
        sb.hdrfilm(res[0], res[1], gauss)
        return sb
    for spp, md in ((1, 2), (8, 6)):
        same, r = compare_render(gpu, oracle, scene().desc(), spp, min_identical=0.999, maxDepth=md)
        print("textures spp %d: identical %.6f rel L2 %.3e" % (spp, same, r))
    compare_render(gpu, oracle, scene(res=(64, 48)).desc(), 4, min_identical=0.999, maxDepth=4, strictNormals=True)


def test_reference_built_pyramids_and_pin_scenes(gpu, oracle, gauss):
    """the scenes on which the oracle is pinned to the reference itself (tests/ref_scenes.py), with the MIP pyramids the
    reference's own TMIPMap built (Lanczos-resampled, half precision; tests/golden/ref_renders.npz): GPU against the
    oracle on the parity stream, path tracer and `direct`"""
    import os
    import ref_scenes as RS
    from test_golden import _golden_mip, G
    from mitsuba_amd.integrator import DirectHIP
    fixture = np.load(os.path.join(G, "ref_renders.npz"))
    for build in (RS.envmap, RS.textures, RS.roughness_maps, RS.zoo, RS.const_env):
        desc = build(gauss, _golden_mip(fixture, build.__name__)).desc()
        same, r = compare_render(gpu, oracle, desc, 4, min_identical=0.999, maxDepth=6)
        print("%s: identical %.6f rel L2 %.3e" % (build.__name__, same, r))
        compare_render(gpu, oracle, desc, 2, min_identical=0.999, integrator=DirectHIP, emitterSamples=2, bsdfSamples=2)


def test_random_scenes_fuzz_against_the_oracle(gpu, oracle, gauss):
    """the fuzz scenes on which the oracle is pinned to the reference (ref_scenes.random_scene): GPU against the oracle on
    the parity stream, path tracer and `direct` with random parameters"""
    import ref_scenes as RS
    from mitsuba_amd.integrator import Scene, PathHIP, DirectHIP, HDRFilm
    import os
    worst = 1.0
    n_scenes = int(os.environ.get("PHIP_FUZZ_SCENES", "600"))         # 2000 were run once during development: all bit-identical
    for seed in range(n_scenes):
        sb, kw = RS.random_scene(gauss, seed, res=(48, 32) if seed % 2 else "random", mip=RS.box_mip)
        desc = sb.desc()
        if kw.get("integrator") == A.PHIP_INTEGRATOR_DIRECT:
            integ = DirectHIP(emitterSamples=kw["emitter_samples"], bsdfSamples=kw["bsdf_samples"], strictNormals=bool(kw["strict_normals"]))
        else:
            integ = PathHIP(maxDepth=kw["max_depth"], rrDepth=kw["rr_depth"], strictNormals=bool(kw["strict_normals"]), hideEmitters=bool(kw["hide_emitters"]))
        gs = Scene(desc)
        film = HDRFilm(gs.width, gs.height)
        gs.setBlockSize([8, 16, 32, 64][seed % 4])
        assert integ.render(gs, film, 4, flags=A.PHIP_FLAG_SAMPLE_BUFFER)
        gsmp = integ.samples(gs, 4)
        osc = oracle.OracleScene(desc)
        ofilm, osmp, _ = osc.render(integ.params(gs, 4), want_samples=True)
        assert rel_l2(film.storage, ofilm) <= 1e-5 or np.abs(ofilm).max() == 0
        same = (gsmp.view(np.uint32) == osmp.view(np.uint32)).all(axis=-1).mean()
        worst = min(worst, same)
        assert same >= 0.995, (seed, kw, same)            # exact-t ties between soup triangles may resolve differently
        assert np.isfinite(gsmp).all() == np.isfinite(osmp).all()
        gs.close(); osc.close()
    print("fuzz: worst fraction of bit-identical samples over %d scenes: %.6f" % (n_scenes, worst))


def test_c2_at_full_size_against_the_oracle(gpu, oracle, gauss):
    """BASELINE.json configs[1] AT FULL SIZE (Cornell box 1024x1024, 256 spp = 268 M samples, progressive passes of the fused
    kernel) against the oracle on every host core.
    (1) The oracle answering ray queries by a sweep over every triangle (the structure-independent closest hit, which is what a
        BVH returns): the films agree to the order of the float additions -- not one of the 268 M samples took another path or
        was lost / duplicated between passes -- and the work counters are equal.
    (2) The oracle with the reference's kd-tree: a handful of samples differ, the ones whose ray passes through a silhouette edge
        that is also a kd-tree split plane (tests/test_ref_pin.py::test_kd_tree_loses_a_silhouette_edge_hit_that_a_bvh_finds);
        the image stays 30 times inside the north star's tolerance.
    (About a minute of the oracle on the GPU box's 256 hardware threads.)"""
    import os
    if (os.cpu_count() or 1) < 32 and not os.environ.get("PHIP_FULLSIZE_ORACLE"):
        pytest.skip("2 x 268 M samples of the CPU oracle: needs the GPU box's host cores (PHIP_FULLSIZE_ORACLE=1 forces it)")
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    desc = S.cornell_box(1024, 1024, gauss).desc()
    gs = Scene(desc); integ = PathHIP()
    film = HDRFilm(1024, 1024)
    assert integ.render(gs, film, 256)
    st = integ.stats
    g = film.develop()
    osc = oracle.OracleScene(desc)
    out = {}
    for mode in ("sweep", "kd-tree"):
        osc.set_bruteforce(mode == "sweep")
        ofilm, _, ost = osc.render(integ.params(gs, 256))
        o = oracle.develop(ofilm)
        d = np.abs(g - o); big = (d > 1e-4 * np.maximum(1.0, np.abs(o))).any(-1)
        r = rel_l2(g, o)
        print("C2 at full size, GPU (fused=%d) vs the oracle (%s): rel L2 %.3e, max abs diff %.3e, %d pixels off by more than 1e-4; path vertices %d / %d, "
              "closest rays %d / %d, shadow rays %d / %d" % (st.fused, mode, r, d.max(), big.sum(), st.path_vertices, ost.path_vertices,
                                                            st.closest_rays, ost.closest_rays, st.shadow_rays, ost.shadow_rays))
        ys, xs = np.nonzero(big)
        for y, x in list(zip(ys, xs))[:6]:
            print("   pixel (%d, %d): GPU %s oracle %s" % (x, y, g[y, x], o[y, x]))
        out[mode] = (r, int(big.sum()), abs(int(st.path_vertices) - int(ost.path_vertices)), abs(int(st.closest_rays) - int(ost.closest_rays)),
                     abs(int(st.shadow_rays) - int(ost.shadow_rays)))
        assert st.samples == ost.samples == 1024 * 1024 * 256
    r, nbig, dv, dc, ds = out["sweep"]
    # (shadow rays: the reference casts the visibility ray inside sampleEmitterDirect, before it evaluates the BSDF; path_hip skips it
    #  when the BSDF value is zero -- a path that slipped inside one of the boxes sees their faces from behind: ~1e-6 of the rays)
    assert nbig == 0 and r <= 2e-6 and dv == 0 and dc == 0 and ds <= 1e-5 * st.shadow_rays, out
    r, nbig, dv, dc, ds = out["kd-tree"]
    assert r <= 1e-4 and nbig <= 256 and dv <= 64, out
    gs.close(); osc.close()


def test_ld_sampler_matches_oracle(gpu, phip, oracle, gauss):
    """PHIP_SAMPLER_LD (the construction of ldsampler on the counter-based generator): per-sample radiance bit-identical to the oracle --
    which is pinned to Mitsuba's own `path` fed with the same points (tests/test_ref_pin.py::test_ld_sampler_on_the_reference) -- on
    the fused kernel and the wavefront kernels, with dielectrics (request order shifts), an early Russian roulette, several passes
    (sample_offset) and a seed; the error cases"""
    import ref_scenes as RS
    from mitsuba_amd.integrator import Scene, PathHIP, DirectHIP, HDRFilm
    ld = dict(sampler=A.PHIP_SAMPLER_LD)
    same, r = compare_render(gpu, oracle, S.cornell_box(64, 64, gauss).desc(), 16, min_identical=1.0, render_kw=ld)
    same, r = compare_render(gpu, oracle, S.cornell_box(48, 40, gauss).desc(), 8, min_identical=1.0, render_kw=dict(ld, seed=3), rrDepth=2)
    same, r = compare_render(gpu, oracle, S.glass_room(64, 36, gauss, detail=0.2).desc(), 8, min_identical=0.9999, render_kw=ld, maxDepth=12, rrDepth=3)
    same, r = compare_render(gpu, oracle, RS.zoo(gauss, None).desc(), 4, min_identical=0.9999, render_kw=ld, maxDepth=8)
    same, r = compare_render(gpu, oracle, S.atrium(64, 36, gauss, detail=0.3).desc(), 4, min_identical=0.999, render_kw=ld, maxDepth=6)
    # two passes of 8 of 16 samples = one render of 16
    desc = S.cornell_box(32, 32, gauss).desc()
    gs = Scene(desc); integ = PathHIP()
    whole = HDRFilm(32, 32); assert integ.render(gs, whole, 16, **ld)
    parts = HDRFilm(32, 32)
    assert integ.render(gs, parts, 8, sample_offset=0, sample_total=16, **ld)
    p = integ.params(gs, 8, flags=A.PHIP_FLAG_ACCUMULATE, sample_offset=8, sample_total=16, **ld)
    acc = parts.storage.copy()
    st = A.phip_stats()
    assert phip.phip_render(gs._h, C.byref(p), acc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)) == 0
    assert rel_l2(acc, whole.storage) < 1e-6
    # a sample count that is not a power of two
    from mitsuba_amd._ffi import PhipError
    with pytest.raises(PhipError):
        integ.render(gs, HDRFilm(32, 32), 12, **ld)
    gs.close()
    # `direct`: sample arrays and single samples
    for e, b in ((1, 1), (3, 2), (0, 2), (4, 1)):
        compare_render(gpu, oracle, RS.zoo(gauss, None).desc(), 8, min_identical=0.9999, integrator=DirectHIP, render_kw=ld, emitterSamples=e, bsdfSamples=b)
    compare_render(gpu, oracle, S.cornell_box(40, 40, gauss).desc(), 16, min_identical=1.0, integrator=DirectHIP, render_kw=ld, emitterSamples=2, bsdfSamples=3)


def test_sobol_and_stratified_samplers_match_oracle(gpu, phip, oracle, gauss):
    """PHIP_SAMPLER_SOBOL (the reference's `sobol` plugin restated: per-pixel enumeration of the global sequence, dimensions by call order) and
    PHIP_SAMPLER_STRATIFIED (the construction of `stratified`, addressable): per-sample radiance bit-identical to the oracle, which
    tests/test_ref_pin.py pins to the reference's own `path` + `sobol` and to `path` on the glue sampler -- diffuse, microfacet and dielectric
    scenes, a film that is not square (resolution = the next power of two of the larger side), progressive passes; and the error cases"""
    import ref_scenes as RS
    from conftest import sobol_tables
    from mitsuba_amd.integrator import Scene, PathHIP, DirectHIP, HDRFilm
    from mitsuba_amd._ffi import PhipError
    for desc, spp, kw, mi in ((S.cornell_box(64, 64, gauss).desc(), 16, {}, 1.0), (S.cornell_box(48, 40, gauss).desc(), 8, dict(rrDepth=2), 1.0),
                              (S.glass_room(64, 36, gauss, detail=0.2).desc(), 8, dict(maxDepth=12, rrDepth=3), 0.9999),
                              (RS.zoo(gauss, None).desc(), 4, dict(maxDepth=8), 0.9999), (S.atrium(64, 36, gauss, detail=0.3).desc(), 4, dict(maxDepth=6), 0.999)):
        w, h = desc.film.crop_width, desc.film.crop_height
        compare_render(gpu, oracle, desc, spp, min_identical=mi, render_kw=dict(sobol=sobol_tables(w, h)), **kw)
        compare_render(gpu, oracle, desc, spp if int(np.sqrt(spp)) ** 2 == spp else 4, min_identical=mi, render_kw=dict(sampler=A.PHIP_SAMPLER_STRATIFIED, seed=5), **kw)
    # scenes with an environment emitter / bitmap textures (the QMC build of the shading kernel with both features)
    from test_golden import _golden_mip, G
    fixture = np.load(os.path.join(G, "ref_renders.npz"))
    for build in (RS.envmap, RS.textures, RS.const_env):
        desc = build(gauss, _golden_mip(fixture, build.__name__)).desc()
        compare_render(gpu, oracle, desc, 4, min_identical=0.999, render_kw=dict(sobol=sobol_tables(desc.film.crop_width, desc.film.crop_height)), maxDepth=6)
        compare_render(gpu, oracle, desc, 4, min_identical=0.999, render_kw=dict(sampler=A.PHIP_SAMPLER_STRATIFIED), maxDepth=6)
    # the Sobol' stream differs from the counter stream and from a film of another resolution (the pixel enumeration depends on it)
    desc = S.cornell_box(32, 32, gauss).desc()
    gs = Scene(desc); integ = PathHIP()
    a, b, c = HDRFilm(32, 32), HDRFilm(32, 32), HDRFilm(32, 32)
    assert integ.render(gs, a, 16, sobol=sobol_tables(32, 32)) and integ.render(gs, b, 16) and integ.render(gs, c, 16, sampler=A.PHIP_SAMPLER_STRATIFIED)
    assert 1e-3 < rel_l2(a.storage, b.storage) < 0.2 and 1e-3 < rel_l2(c.storage, b.storage) < 0.2
    # two passes of 8 of 16 samples = one render of 16 (the sequence index of a sample is its global number)
    for kw in (dict(sobol=sobol_tables(32, 32)), dict(sampler=A.PHIP_SAMPLER_STRATIFIED)):
        whole = HDRFilm(32, 32); assert integ.render(gs, whole, 16, **kw)
        parts = HDRFilm(32, 32); assert integ.render(gs, parts, 8, sample_offset=0, sample_total=16, **kw)
        p = integ.params(gs, 8, flags=A.PHIP_FLAG_ACCUMULATE, sample_offset=8, sample_total=16, **kw)
        acc = parts.storage.copy(); st = A.phip_stats()
        assert phip.phip_render(gs._h, C.byref(p), acc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)) == 0
        assert rel_l2(acc, whole.storage) < 1e-6
    # errors: a wrong resolution, no tables, rrDepth 1 (sobol.cpp:241-242 is restated for rrDepth >= 2), a stratified count that is no square
    with pytest.raises(PhipError): integ.render(gs, HDRFilm(32, 32), 16, sobol=sobol_tables(64, 64))
    with pytest.raises(PhipError): integ.render(gs, HDRFilm(32, 32), 16, sampler=A.PHIP_SAMPLER_SOBOL)
    with pytest.raises(PhipError): PathHIP(rrDepth=1).render(gs, HDRFilm(32, 32), 16, sobol=sobol_tables(32, 32))
    with pytest.raises(PhipError): integ.render(gs, HDRFilm(32, 32), 8, sampler=A.PHIP_SAMPLER_STRATIFIED)
    gs.close()
    # round 5: `stratified` with `direct` -- single samples (the sample's next 2D requests) and sample arrays (one Latin hypercube per array)
    for desc, spp, e, b in ((S.cornell_box(48, 40, gauss).desc(), 16, 1, 1), (S.cornell_box(48, 40, gauss).desc(), 4, 3, 2), (S.cornell_mixed(48, 40, gauss).desc(), 9, 2, 1),
                            (S.atrium(64, 36, gauss, detail=0.3).desc(), 4, 2, 2), (S.cornell_box(32, 32, gauss).desc(), 4, 0, 3)):
        compare_render(gpu, oracle, desc, spp, min_identical=0.999, integrator=DirectHIP, render_kw=dict(sampler=A.PHIP_SAMPLER_STRATIFIED, seed=3), emitterSamples=e, bsdfSamples=b)


def test_qmc_samplers_on_a_crop_window_off_the_films_origin_match_oracle(gpu, oracle, gauss):
    """round 5: the sequence samplers on a crop window that does not start at the film's origin (refused until then; the reference's blocks and sampler positions are
    relative to the crop window: tests/test_ref_pin.py::test_qmc_samplers_on_a_crop_window_off_the_films_origin)"""
    from conftest import sobol_tables, qmc_tables
    sb = S.cornell_box(160, 120, gauss)
    sb.hdrfilm(160, 120, gauss, crop=(61, 35, 48, 40))
    desc = sb.desc()
    for kw in (dict(sobol=sobol_tables(48, 40)), dict(sampler=A.PHIP_SAMPLER_HALTON, qmc=qmc_tables(-1)), dict(sampler=A.PHIP_SAMPLER_HAMMERSLEY, qmc=qmc_tables(-1))):
        same, r = compare_render(gpu, oracle, desc, 8, min_identical=1.0, render_kw=kw, maxDepth=6)
        assert same == 1.0


def test_halton_and_hammersley_samplers_match_oracle(gpu, phip, oracle, gauss):
    """PHIP_SAMPLER_HALTON / _HAMMERSLEY (the reference's `halton` / `hammersley` plugins restated: tests/test_ref_pin.py pins the oracle to Mitsuba's own
    `path` + those plugins): per-sample radiance bit-identical to the oracle -- Faure permutations, none, pseudorandom ones; microfacet, dielectric,
    environment-map and textured scenes; a film wider than 128 pixels (positions enter modulo 128); progressive passes; the error cases"""
    import ref_scenes as RS
    from conftest import qmc_tables
    from test_golden import _golden_mip, G
    from mitsuba_amd.integrator import Scene, PathHIP, DirectHIP, HDRFilm
    from mitsuba_amd._ffi import PhipError
    fixture = np.load(os.path.join(G, "ref_renders.npz"))
    for desc, spp, kw, mi in ((S.cornell_box(64, 64, gauss).desc(), 16, dict(maxDepth=10), 1.0), (S.cornell_box(150, 40, gauss).desc(), 5, dict(maxDepth=8, rrDepth=2), 1.0),
                              (S.glass_room(64, 36, gauss, detail=0.2).desc(), 8, dict(maxDepth=10, rrDepth=3), 0.9999),
                              (RS.zoo(gauss, None).desc(), 4, dict(maxDepth=8), 0.9999), (S.atrium(64, 36, gauss, detail=0.3).desc(), 4, dict(maxDepth=6), 0.999),
                              (RS.envmap(gauss, _golden_mip(fixture, "envmap")).desc(), 4, dict(maxDepth=6), 0.999),
                              (RS.textures(gauss, _golden_mip(fixture, "textures")).desc(), 4, dict(maxDepth=6), 0.999)):
        for kind in (A.PHIP_SAMPLER_HALTON, A.PHIP_SAMPLER_HAMMERSLEY):
            for scramble in (-1, 0, 7):
                compare_render(gpu, oracle, desc, spp, min_identical=mi, render_kw=dict(sampler=kind, qmc=qmc_tables(scramble)), **kw)
    desc = S.cornell_box(32, 32, gauss).desc()
    gs = Scene(desc); integ = PathHIP(maxDepth=8)
    for kind in (A.PHIP_SAMPLER_HALTON, A.PHIP_SAMPLER_HAMMERSLEY):
        kw = dict(sampler=kind, qmc=qmc_tables(-1))
        # two passes of 8 of 16 samples = one render of 16 (hammersley: the set is that of the whole render's sample count)
        whole = HDRFilm(32, 32); assert integ.render(gs, whole, 16, **kw)
        parts = HDRFilm(32, 32); assert integ.render(gs, parts, 8, sample_offset=0, sample_total=16, **kw)
        p = integ.params(gs, 8, flags=A.PHIP_FLAG_ACCUMULATE, sample_offset=8, sample_total=16, **kw)
        acc = parts.storage.copy(); st = A.phip_stats()
        assert phip.phip_render(gs._h, C.byref(p), acc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)) == 0
        assert rel_l2(acc, whole.storage) < 1e-6
        ctr = HDRFilm(32, 32); assert integ.render(gs, ctr, 16)
        assert 1e-3 < rel_l2(whole.storage, ctr.storage) < 0.3
        # the device copies of the tables are keyed by CONTENT: the plugin refills its permutation vector in place when `scramble` changes
        # (same address, same size), and phip.h only promises "read during the call"
        primes, faure = qmc_tables(-1); _, rnd = qmc_tables(7)
        buf = faure.copy()
        a = HDRFilm(32, 32); assert integ.render(gs, a, 16, sampler=kind, qmc=(primes, buf))
        buf[:] = rnd
        b = HDRFilm(32, 32); assert integ.render(gs, b, 16, sampler=kind, qmc=(primes, buf))
        fresh = HDRFilm(32, 32); assert integ.render(gs, fresh, 16, sampler=kind, qmc=(primes, rnd))
        assert (b.storage == fresh.storage).all() and (a.storage == whole.storage).all() and not (a.storage == b.storage).all()
        # errors: no tables, rrDepth 1, `direct`
        with pytest.raises(PhipError): integ.render(gs, HDRFilm(32, 32), 16, sampler=kind)
        with pytest.raises(PhipError): PathHIP(rrDepth=1).render(gs, HDRFilm(32, 32), 16, **kw)
    # hammersley has no sample arrays (hammersley.cpp:293-300)
    with pytest.raises(PhipError): DirectHIP(emitterSamples=2, bsdfSamples=1).render(gs, HDRFilm(32, 32), 16, sampler=A.PHIP_SAMPLER_HAMMERSLEY, qmc=qmc_tables(-1))
    gs.close()


def test_direct_with_the_qmc_samplers_matches_oracle(gpu, phip, oracle, gauss):
    """`direct` on the reference's sequence samplers (the oracle is pinned to Mitsuba's own `direct` + `sobol` / `halton` / `hammersley`:
    tests/test_ref_pin.py::test_direct_with_the_reference_qmc_samplers_is_reproduced_bit_for_bit): sample arrays (dimensions 5.. of "sample j of
    the pixel") and single samples (dimensions (2, 3), then (5, 6)) in every combination, per-sample radiance bit-identical; scenes with microfacet /
    dielectric BSDFs, an environment map and textures (the QMC build of k_shade_direct with both features); progressive passes"""
    import ref_scenes as RS
    from conftest import sobol_tables, qmc_tables
    from test_golden import _golden_mip, G
    from mitsuba_amd.integrator import Scene, DirectHIP, HDRFilm
    fixture = np.load(os.path.join(G, "ref_renders.npz"))
    scenes = [(S.cornell_box(40, 36, gauss).desc(), 1.0), (RS.zoo(gauss, None).desc(), 0.9999),
              (RS.envmap(gauss, _golden_mip(fixture, "envmap")).desc(), 0.999), (RS.textures(gauss, _golden_mip(fixture, "textures")).desc(), 0.999)]
    for desc, mi in scenes:
        w, h = desc.film.crop_width, desc.film.crop_height
        for e, b in ((1, 1), (3, 2), (0, 2), (4, 1)):
            compare_render(gpu, oracle, desc, 4, min_identical=mi, integrator=DirectHIP, render_kw=dict(sobol=sobol_tables(w, h)), emitterSamples=e, bsdfSamples=b)
            compare_render(gpu, oracle, desc, 4, min_identical=mi, integrator=DirectHIP, render_kw=dict(sampler=A.PHIP_SAMPLER_HALTON, qmc=qmc_tables(7)), emitterSamples=e, bsdfSamples=b)
        compare_render(gpu, oracle, desc, 4, min_identical=mi, integrator=DirectHIP, render_kw=dict(sampler=A.PHIP_SAMPLER_HAMMERSLEY, qmc=qmc_tables(-1)), emitterSamples=1, bsdfSamples=1)
    # two passes of 4 of 8 samples = one render of 8 (array element k * count + i with k the sample's global number)
    desc = S.cornell_box(32, 32, gauss).desc()
    gs = Scene(desc); integ = DirectHIP(emitterSamples=3, bsdfSamples=2)
    for kw in (dict(sobol=sobol_tables(32, 32)), dict(sampler=A.PHIP_SAMPLER_HALTON, qmc=qmc_tables(-1))):
        whole = HDRFilm(32, 32); assert integ.render(gs, whole, 8, **kw)
        parts = HDRFilm(32, 32); assert integ.render(gs, parts, 4, sample_offset=0, sample_total=8, **kw)
        p = integ.params(gs, 4, flags=A.PHIP_FLAG_ACCUMULATE, sample_offset=4, sample_total=8, **kw)
        acc = parts.storage.copy(); st = A.phip_stats()
        assert phip.phip_render(gs._h, C.byref(p), acc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)) == 0
        assert rel_l2(acc, whole.storage) < 1e-6
    gs.close()


def _sheets_scene(gauss, w=96, h=96, n=15):
    """15 diffuse sheets one behind the other (30 triangles, staggered so that camera rays end on different ones) and a two-triangle light in front of
    them: a tree of at most 32 Wald records in at most 32 leaves, i.e. the fused kernel's flat table -- and EVERY ray enters (nearly) every leaf box."""
    sb = S.SceneBuilder()
    rng = np.random.default_rng(3)
    for i in range(n):
        m = sb.diffuse(tuple(rng.uniform(0.3, 0.8, 3)))
        s = 100.0 - 75.0 * i / n
        ox, oy = 14.0 * (i % 4) - 20.0, 9.0 * (i % 3) - 9.0
        z = 150.0 * i / n
        sb.quad((ox - s, oy - s, z), (ox + s, oy - s, z), (ox + s, oy + s, z), (ox - s, oy + s, z), m, facing=(0, 0, -1))
    black = sb.diffuse((0, 0, 0))
    sb.quad((-60, 130, -150), (60, 130, -150), (60, 170, -120), (-60, 170, -120), black, facing=(0, -1, 1), radiance=(30.0, 25.0, 20.0))
    sb.perspective((0, 0, -260), (0, 0, 0), (0, 1, 0), 50.0, near=1.0, far=1e4)
    sb.hdrfilm(w, h, gauss)
    return sb


def test_fused_kernel_work_list_overflow_matches_oracle(gpu, oracle, gauss):
    """k_mega deals the Wald tests of a wave through a work list of 512 (ray, record) pairs (k_traverse.h: traverseFlat2W); the Cornell box never fills it
    (64 x 3.1).  Here every ray enters the boxes of ~30 records: ~1900 pairs per wave, four rounds with the lanes that did not fit -- closest hits, shadow rays
    and their work counters must be what the per-lane loop and the oracle give."""
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    sb = _sheets_scene(gauss)
    desc = sb.desc()
    assert desc.n_triangles == 32
    same, r = compare_render(gpu, oracle, desc, 16, min_identical=1.0, maxDepth=6)
    assert same == 1.0
    # the scene took the fused kernel (compare_render then also held it against the wavefront kernels), and a ray tests many records
    gs = Scene(desc); integ = PathHIP(maxDepth=6); film = HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, 4)
    st = integ.stats
    # (5 tests per ray on average -- 330 pairs per wave; the camera rays of a wave, which all enter every box from the front, bring ~1900)
    assert st.fused and st.closest_triangle_tests >= 4 * st.closest_rays, (st.fused, st.closest_triangle_tests, st.closest_rays)
    gs.close()


@pytest.mark.parametrize("extra", [1, 3])
def test_cornell_with_33_to_64_records_keeps_the_dealt_traversal(gpu, oracle, gauss, extra):
    """Round 5: a Cornell box with a third (.. fifth) block has 42 (.. 62) Wald records; trees of up to 64 records keep the fused kernel's
    packed leaf table with record masks -- two words -- and the Wald tests dealt over the wave (k_traverse.h: traverseFlat2W<.., R64>; phip_accel_info.fused_traversal == 3).
    Per-sample identity with the oracle, and (compare_render) fused == wavefront."""
    from mitsuba_amd.integrator import Scene
    desc = S.cornell_box(96, 96, gauss, extra_blocks=extra).desc()
    assert 32 < desc.n_triangles <= 64
    gs = Scene(desc); info = gs.accel_info().as_dict(); gs.close()
    assert info["fits_lds"] == 1 and info["fused_traversal"] == 3, info
    for cfg in (dict(maxDepth=-1), dict(maxDepth=5, strictNormals=True)):
        same, r = compare_render(gpu, oracle, desc, 8, min_identical=1.0, **cfg)
        assert same == 1.0


def _spine_scene(gauss, w=32, h=32, n=60):
    """60 triangles of geometrically growing size strung out along a diagonal, each enclosing box containing all the smaller ones, and a two-triangle light: 62 Wald
    records whose SAH tree is one long spine -- the deepest binary tree the builder makes of so few triangles"""
    rng = np.random.default_rng(11)
    size = 1e-2 * 1.3 ** np.arange(n)                            # almost seven orders of magnitude
    centre = np.stack([size * 3.0, np.zeros(n), size * 3.0], 1)
    tri = rng.normal(size=(n, 3, 3)) * size[:, None, None] * 0.7 + centre[:, None, :]
    P = tri.reshape(-1, 3).astype(np.float32)
    T = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    sb = S.SceneBuilder()
    sb.mesh(P, T, sb.twosided(sb.diffuse((0.7, 0.6, 0.5))))
    ext = float(np.abs(P).max())
    black = sb.diffuse((0, 0, 0))
    sb.quad((-ext, 2 * ext, -ext), (ext, 2 * ext, -ext), (ext, 2 * ext, ext), (-ext, 2 * ext, ext), black, facing=(0, -1, 0), radiance=(8.0, 8.0, 8.0))
    sb.perspective((0.3 * ext, 0.5 * ext, -2.0 * ext), (0.3 * ext, 0.0, 0.3 * ext), (0, 1, 0), 50.0, near=1e-4 * ext, far=10 * ext)
    sb.hdrfilm(w, h, gauss)
    return sb


def test_deep_tree_of_at_most_64_records_keeps_the_packed_leaf_table(gpu, oracle, gauss):
    """The packed leaf table has no stack, so the depth of the tree its leaves come from decides nothing: a spine of 62 records is served by the fused kernel like
    every other scene of its size (HISTORY.md, "The 4-wide tree leaves the host": such a scene used to fall to the wavefront kernels).  Bit-identical samples on
    every device path."""
    from mitsuba_amd.integrator import Scene
    desc = _spine_scene(gauss).desc()
    assert desc.n_triangles == 62
    gs = Scene(desc); info = gs.accel_info().as_dict(); gs.close()
    assert info["fits_lds"] == 1 and info["fused_traversal"] == 3, info
    compare_render(gpu, oracle, desc, 4)


def test_fused_kernel_64_record_work_list_overflow_matches_oracle(gpu, oracle, gauss):
    """the overflow scene of the test above with 64 sheets: every record bit of BOTH mask words set for the camera rays, ~3800 pairs per wave"""
    sb = _sheets_scene(gauss, n=31)
    desc = sb.desc()
    assert desc.n_triangles == 64
    from mitsuba_amd.integrator import Scene
    gs = Scene(desc); info = gs.accel_info().as_dict(); gs.close()
    assert info["fused_traversal"] == 3, info
    same, r = compare_render(gpu, oracle, desc, 8, min_identical=1.0, maxDepth=6)
    assert same == 1.0


def test_deep_wide_tree_spills_its_group_stack(gpu, oracle, gauss):
    """k_rays_w keeps WIDE_STACK_LDS = 6 group entries per lane in LDS and spills deeper ones to HBM.  A scene whose SAH tree is a long spine -- triangles
    of geometrically growing size along a line, each enclosing box containing all the smaller ones -- makes the wide tree far deeper than six levels: closest hits
    (phip_trace, against a sweep over all triangles) and a render (k_rays_w: per-sample identity with the oracle) go through the spill path."""
    rng = np.random.default_rng(5)
    n = 6000
    i = np.arange(n)
    size = 1e-3 * 1.0035 ** i                                    # seven orders of magnitude of triangle sizes
    centre = np.stack([size * 3.0, np.zeros(n), size * 3.0], 1)    # ... strung out along a diagonal, the big ones far from the small ones
    tri = rng.normal(size=(n, 3, 3)) * size[:, None, None] * 0.7 + centre[:, None, :]
    P = tri.reshape(-1, 3).astype(np.float32)
    T = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    sb = S.SceneBuilder()
    sb.mesh(P, T, sb.twosided(sb.diffuse((0.7, 0.6, 0.5))))
    ext = float(np.abs(P).max())
    black = sb.diffuse((0, 0, 0))
    sb.quad((-ext, 2 * ext, -ext), (ext, 2 * ext, -ext), (ext, 2 * ext, ext), (-ext, 2 * ext, ext), black, facing=(0, -1, 0), radiance=(8.0, 8.0, 8.0))
    sb.perspective((0.3 * ext, 0.5 * ext, -2.0 * ext), (0.3 * ext, 0.0, 0.3 * ext), (0, 1, 0), 50.0, near=1e-4 * ext, far=10 * ext)
    sb.hdrfilm(64, 48, gauss)
    desc = sb.desc()
    gs = gpu.Scene(desc); osc = oracle.OracleScene(desc)
    info = gs.accel_info().as_dict()
    assert info["node_bytes"] == 80 and info["max_depth"] >= 10, info          # the wide tree, deeper than the LDS part of the stack
    rays = random_rays(rng, 40000, -0.2 * ext, 1.2 * ext, mint=0.0)
    rays[:20000, :3] *= 0.01                                     # half of them among the small triangles
    gh, go, _ = gs.rayIntersect(rays, True, True)
    bh, _, _ = osc.trace(rays, True, False, bruteforce=True)
    assert (gh.view(np.uint32) == bh.view(np.uint32)).all(axis=1).mean() > 0.9999
    oh, oo, _ = osc.trace(rays, True, True)
    assert (go == oo).mean() > 0.9999
    gs.close(); osc.close()
    compare_render(gpu, oracle, desc, 4, min_identical=0.999, maxDepth=5)


def test_far_camera_keeps_every_leaf_box_of_the_flat_table(gpu, oracle, gauss):
    """the fused kernel's pass 1 computes slab distances as c rcp - o rcp, whose cancellation error grows with |o|; a camera hundreds of scene extents
    away (a telephoto view of the Cornell box) must not lose leaf boxes -- the host pads the table's half extents for the camera position (phip.hip)"""
    for dist, fov in ((60.0, 1.0), (400.0, 0.15), (3000.0, 0.02), (20000.0, 0.003)):
        sb = S.cornell_box(64, 64, gauss)
        sb.perspective(origin=(278.0, 273.0, -560.0 * dist), target=(278.0, 273.0, 0.0), up=(0, 1, 0), fov_x_deg=fov, near=10.0, far=560.0 * dist * 2.0)
        # 3000 extents: a hit distance of 1.7 M scene units is quantised to 1 / 8 of a unit, and the Wald test accepts rays that pass a silhouette by a few hundredths of a
        # unit -- on any axis, whatever axis the camera is far away on.  Until round 6 the boxes were padded per axis by the camera's coordinate on THAT axis, and the
        # packed leaf table lost one primary ray in 32768 samples (0.03 units beside the tall block; the 8-wide tree kept it by the slack of its quantised boxes): every
        # axis is padded by the camera's largest coordinate now (bvh.h: buildBVH), and every device path is held to bit identity at every distance again
        same, r = compare_render(gpu, oracle, sb.desc(), 8, min_identical=0.9999, maxDepth=5)
        print("camera %g scene extents away: identical %.6f rel L2 %.3e" % (dist, same, r))


def test_cornell_mixed_matches_oracle(gpu, oracle, gauss):
    """bench.py's `cornell_mixed_*` workload: the Cornell box with a rough-copper and a glass block -- 32 triangles, all three leaf BSDF
    models; a tree of 32 Wald records, so k_shade_trace (one kernel per iteration: vertex + shadow ray + next ray on the packed leaf table in LDS)"""
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    desc = S.cornell_mixed(128, 128, gauss).desc()
    gs = Scene(desc); integ = PathHIP(maxDepth=6); film = HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, 2)
    assert integ.stats.fused == 1 and integ.stats.vertex_traced == 0, integ.stats.as_dict()      # round 5: the fused kernel serves all three leaf BSDF models on the packed leaf table
    assert integ.render(gs, film, 2, flags=A.PHIP_FLAG_NO_MEGA)
    assert integ.stats.vertex_traced == 1 and integ.stats.fused == 0 and integ.stats.trace_kernel_ms == 0, integ.stats.as_dict()
    gs.close()
    for cfg in (dict(maxDepth=-1), dict(maxDepth=8, strictNormals=True)):
        # k_mega == oracle == the three-kernel iterations (compare_render) ...
        same, r = compare_render(gpu, oracle, desc, 8, min_identical=0.9999, **cfg)
        print("cornell_mixed %s: identical %.6f rel L2 %.3e" % (cfg, same, r))
        # ... == k_shade_trace (PHIP_FLAG_NO_MEGA; compare_render again holds it against the three-kernel iterations)
        same, r = compare_render(gpu, oracle, desc, 8, min_identical=0.9999, render_kw=dict(flags_extra=A.PHIP_FLAG_NO_MEGA), **cfg)
    # a ragged film: the edge blocks' ids outside the image are drawn and skipped (k_mega's count of the block's live ids must take them back, or its waves never leave)
    same, r = compare_render(gpu, oracle, S.cornell_mixed(100, 70, gauss).desc(), 6, min_identical=0.9999, maxDepth=-1)


def test_cornell_mixed_paths_change_lanes_not_values(gpu, gauss):
    """In k_mega<MM_ALL> paths change lanes and waves through LDS: with the counter stream a path that hits copper goes to the block's serving wave through a
    mailbox and comes back through another (MEGA_MAILBOX); the QMC build deals the block's paths to its lanes by BSDF model before every vertex (MEGA_CLASS_DEAL:
    the sequence index travels along).  At a size where every lane carries ~16 paths one after another, every sample of the frame is bit-identical to the
    three-kernel iterations, whatever the sampler and the integrator -- and none is lost (the statistics count them)"""
    from conftest import sobol_tables, qmc_tables
    from mitsuba_amd.integrator import Scene, PathHIP, VolPathSimpleHIP, HDRFilm
    w = h = 512; spp = 16
    gs = Scene(S.cornell_mixed(w, h, gauss).desc())
    for name, cls, kw in (("ctr", PathHIP, {}), ("sobol", PathHIP, dict(sobol=sobol_tables(w, h))), ("halton", PathHIP, dict(sampler=A.PHIP_SAMPLER_HALTON, qmc=qmc_tables(-1))),
                          ("volpath_simple", VolPathSimpleHIP, {})):
        integ = cls(maxDepth=-1); film = HDRFilm(w, h); film2 = HDRFilm(w, h)
        assert integ.render(gs, film, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER, **kw)
        assert integ.stats.fused == 1, name
        a = integ.samples(gs, spp).copy(); va = integ.stats.path_vertices
        assert integ.render(gs, film2, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER | A.PHIP_FLAG_NO_FUSED, **kw)
        assert integ.stats.fused == 0 and integ.stats.vertex_traced == 0, name
        b = integ.samples(gs, spp)
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), (name, float((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).mean()))
        assert (film.storage.view(np.uint32) == film2.storage.view(np.uint32)).all() and va == integ.stats.path_vertices and integ.stats.samples == w * h * spp
    gs.close()


@pytest.mark.parametrize("cfg", [
    dict(maxDepth=-1), dict(maxDepth=1), dict(maxDepth=2), dict(maxDepth=3), dict(maxDepth=-1, rrDepth=2),
    dict(maxDepth=6, strictNormals=True), dict(maxDepth=5, hideEmitters=True),
])
def test_volpath_simple_cornell_matches_oracle(gpu, oracle, gauss, cfg):
    """Round 5: the sibling integrator `volpath_simple` on media-free scenes -- PHIP_INTEGRATOR_VOLPATH_SIMPLE, a uniform
    branch of shadeVertex -- on the fused kernel (and, through compare_render, the wavefront kernels): per-sample identity with the oracle's restatement of
    volpath_simple.cpp:88-318, which tests/test_ref_pin.py pins on the reference's own plugin"""
    from mitsuba_amd.integrator import VolPathSimpleHIP
    desc = S.cornell_box(96, 96, gauss).desc()
    compare_render(gpu, oracle, desc, 8, integrator=VolPathSimpleHIP, **cfg)


def test_volpath_simple_materials_emitters_textures_match_oracle(gpu, oracle, gauss):
    """... on glass and copper (emitted radiance behind delta bounces: the mixed Cornell box, k_shade_trace), on the big-scene kernels (atrium, glass room), under
    a constant environment with hideEmitters, on bitmap textures"""
    from mitsuba_amd.integrator import VolPathSimpleHIP
    import ref_scenes as RS
    from test_golden import _golden_mip, G
    fixture = np.load(os.path.join(G, "ref_renders.npz"))
    mip_of = lambda scene: _golden_mip(fixture, scene)
    for name, desc, spp, kw in (("cornell_mixed", S.cornell_mixed(96, 96, gauss).desc(), 8, dict(maxDepth=-1)),
                                ("cornell_mixed md 4 strict", S.cornell_mixed(96, 96, gauss).desc(), 8, dict(maxDepth=4, strictNormals=True)),
                                ("atrium", S.atrium(160, 90, gauss).desc(), 4, dict(maxDepth=8)),
                                ("glass room", S.glass_room(160, 90, gauss).desc(), 4, dict(maxDepth=16)),
                                ("constant environment", RS.const_env(gauss, None).desc(), 8, dict(maxDepth=6, rrDepth=2)),
                                ("constant environment, hidden", RS.const_env(gauss, None).desc(), 8, dict(maxDepth=4, hideEmitters=True, strictNormals=True)),
                                ("envmap", RS.envmap(gauss, mip_of("envmap")).desc(), 4, dict(maxDepth=6)),
                                ("textures", RS.textures(gauss, mip_of("textures")).desc(), 4, dict(maxDepth=6))):
        same, r = compare_render(gpu, oracle, desc, spp, min_identical=0.999, integrator=VolPathSimpleHIP, **kw)
        print("volpath_simple, %s: identical %.6f rel L2 %.3e" % (name, same, r))


def test_ray_kernel_work_list_overflow_matches_oracle(gpu, oracle, gauss):
    """k_rays_w deals the triangle tests of an iteration through a work list of 256 pairs per wave (k_wide.h: WIDE_DEAL); lanes whose pairs do not fit wait
    for the next iteration.  A haystack of long overlapping triangles (every leaf group holds many records, every ray enters many leaves) overflows it all the
    time; results and per-sample radiance must still be the oracle's."""
    rng = np.random.default_rng(17)
    n = 3000
    c = rng.uniform(-3.0, 3.0, (n, 1, 3))
    axis = rng.normal(size=(n, 1, 3)); axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    t = np.array([-9.0, 9.0, 0.0]).reshape(1, 3, 1)
    side = rng.normal(scale=0.6, size=(n, 3, 3))
    P = (c + t * axis + side).astype(np.float32).reshape(-1, 3)          # needles ~18 long, ~1 wide, through a ball of radius 3
    T = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    sb = S.SceneBuilder()
    sb.mesh(P, T, sb.twosided(sb.diffuse((0.6, 0.55, 0.5))))
    black = sb.diffuse((0, 0, 0))
    sb.quad((-8, 14, -8), (8, 14, -8), (8, 14, 8), (-8, 14, 8), black, facing=(0, -1, 0), radiance=(12.0, 11.0, 10.0))
    sb.perspective((0, 2, -26), (0, 0, 0), (0, 1, 0), 40.0, near=0.1, far=1e3)
    sb.hdrfilm(64, 48, gauss)
    desc = sb.desc()
    from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
    gs = Scene(desc)
    info = gs.accel_info().as_dict()
    assert info["node_bytes"] == 80, info                                 # the compressed wide tree, i.e. k_rays_w
    integ = PathHIP(maxDepth=5); film = HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, 2, flags=A.PHIP_FLAG_NO_FUSED)
    st = integ.stats
    assert not st.fused and st.closest_triangle_tests >= 12 * st.closest_rays, (st.closest_triangle_tests, st.closest_rays)
    # round 6: a tree of this size runs the fused kernel by default -- its triangle rounds are the same rounds on the same 256-entry list (k_wide_wave.h)
    assert integ.render(gs, film, 2)
    assert integ.stats.fused and integ.stats.closest_triangle_tests >= 12 * integ.stats.closest_rays, (integ.stats.closest_triangle_tests, integ.stats.closest_rays)
    gs.close()
    compare_render(gpu, oracle, desc, 4, min_identical=0.999, maxDepth=5)


def test_cornell_spheres_run_the_fused_kernel_on_the_wide_tree(gpu, oracle, gauss):
    """Round 6: the scenes between the LDS-resident boxes and the atrium -- the Cornell box with two tessellated spheres, 1 k triangles, a tree of
    ~110 compressed 8-wide nodes that lives in L2 -- run k_mega with the tree in memory (phip_accel_info.fused_traversal 4; k_wide_wave.h): a lane owns its path,
    the wave's rays walk the tree with the group stack in LDS and their Wald tests dealt over the wave.  Every sample bit-identical to the oracle AND to the
    wavefront kernels (compare_render renders both), counters included; diffuse spheres and glass + copper (the mailbox build), strictNormals, a ragged film,
    the reference's sobol / halton streams (the QMC builds: the class deal instead of the mailboxes), volpath_simple."""
    from conftest import sobol_tables, qmc_tables
    from mitsuba_amd.integrator import Scene, PathHIP, VolPathSimpleHIP, HDRFilm
    for materials in (False, True):
        desc = S.cornell_spheres(96, 96, gauss, materials=materials).desc()
        gs = Scene(desc); ai = gs.accel_info(); integ = PathHIP(maxDepth=6); film = HDRFilm(gs.width, gs.height)
        assert ai.fits_lds == 0 and ai.fused_traversal == 4 and ai.n_nodes <= A.PHIP_FUSED_WIDE_MAX_NODES, (ai.fits_lds, ai.fused_traversal, ai.n_nodes)
        assert integ.render(gs, film, 2)
        assert integ.stats.fused == 1 and integ.stats.trace_kernel_ms == 0 and integ.stats.iterations == 1, integ.stats.as_dict()
        assert integ.render(gs, film, 2, flags=A.PHIP_FLAG_NO_FUSED)
        assert integ.stats.fused == 0 and integ.stats.iterations > 1
        gs.close()
        for cfg in (dict(maxDepth=-1), dict(maxDepth=7, strictNormals=True), dict(maxDepth=2), dict(maxDepth=5, hideEmitters=True)):
            same, r = compare_render(gpu, oracle, desc, 8, min_identical=0.9999, **cfg)
            print("cornell_spheres(materials=%s) %s: identical %.6f rel L2 %.3e" % (materials, cfg, same, r))
        compare_render(gpu, oracle, desc, 4, min_identical=0.9999, render_kw=dict(sobol=sobol_tables(96, 96)), maxDepth=8)
        compare_render(gpu, oracle, desc, 4, min_identical=0.9999, render_kw=dict(sampler=A.PHIP_SAMPLER_HALTON, qmc=qmc_tables(-1)), maxDepth=8)
        compare_render(gpu, oracle, desc, 4, min_identical=0.9999, integrator=VolPathSimpleHIP, maxDepth=8)
    # a ragged film (ids outside the image are drawn and skipped), finer spheres (4.5 k triangles)
    compare_render(gpu, oracle, S.cornell_spheres(100, 70, gauss, nlon=48, nlat=24).desc(), 4, min_identical=0.9999, maxDepth=-1)


def test_fused_kernel_that_gives_up_degrades_to_the_wavefront_kernels(gpu, gauss, tmp_path):
    """k_mega bounds every wait of its mailbox protocol and the depth of its task stacks; a wave that gives up poisons its sample count.  The host
    used to refuse the frame (a hard error); now it re-renders the pass on the kernels that have no such protocol and logs a warning.  A fault-injection build
    (-DMEGA_MB_FAULT=1: the first wave of every fused launch reports that it gave up) must deliver the frame of the product build, bit for bit -- on the LDS-resident
    mixed box (the mailbox build), on the Cornell box (the build of the metric) and on the spheres (the tree in memory), also over several passes."""
    import subprocess, sys
    from mitsuba_amd import _ffi
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available: the fault-injection library cannot be built")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the library with the fault compiled in: __graft_entry__.build() made it in the build container and it travelled with the snapshot (the call returns at once when
    # the file carries the current build id; otherwise it is built here, whole -- the product's objects do not travel to the GPU box: .gpurunignore)
    lib = _ffi.build_test_variant("fault")
    script = r"""
import sys, os
sys.path.insert(0, %r)
import numpy as np
from mitsuba_amd import _ffi, _abi as A, scene as S
from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
ft = _ffi.gaussian_filter(0.5)
out = {}
for name, sb, spp in (("mixed", S.cornell_mixed(96, 96, ft), 8), ("box", S.cornell_box(64, 64, ft), 8), ("spheres", S.cornell_spheres(96, 96, ft), 4)):
    gs = Scene(sb.desc()); integ = PathHIP(maxDepth=6); film = HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER)
    out[name + "_samples"] = integ.samples(gs, spp).copy(); out[name + "_film"] = film.storage.copy(); out[name + "_fused"] = np.array([integ.stats.fused, integ.stats.samples])
    gs.close()
np.savez(sys.argv[1], **out)
""" % root
    # several passes: the fault build poisons EVERY launch, so the job's first pass gives up and the whole job runs on the wavefront kernels, pass by pass (a later pass
    # that gives up: test_late_fused_pass_that_gives_up_continues_the_job)
    multi = {"PHIP_MAX_PASS_SAMPLES": str(96 * 96 * 3)}
    res = {}
    for tag, e in (("product", {}), ("fault", {"PHIP_LIB": lib}), ("product_multi", multi), ("fault_multi", dict(multi, PHIP_LIB=lib))):
        f = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", script, f], env=dict(os.environ, **e), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res[tag] = (np.load(f), r.stderr)
        assert ("warning: the fused kernel gave up" in r.stderr) == tag.startswith("fault"), (tag, r.stderr[-500:])
    for a, b in (("product", "fault"), ("product_multi", "fault_multi")):
        prod, fault = res[a][0], res[b][0]
        for name in ("mixed", "box", "spheres"):
            assert prod[name + "_fused"][0] == 1 and fault[name + "_fused"][0] == 0, name                    # the product ran k_mega, the fault build ended on the wavefront kernels
            assert prod[name + "_fused"][1] == fault[name + "_fused"][1], name                                 # every sample counted once
            assert (prod[name + "_film"].view(np.uint32) == fault[name + "_film"].view(np.uint32)).all(), (a, name)
            assert (prod[name + "_samples"].view(np.uint32) == fault[name + "_samples"].view(np.uint32)).all(), (a, name)


def test_task_stack_of_the_fused_kernel_spills_to_memory(gpu, gauss, tmp_path):
    """The shared task stack of a wave (k_wide_wave.h: traceWidePool) holds WP_CAP = 256 entries in LDS; what does not fit goes to the wave's slice of the spill buffer in
    memory (written by one lane, read by another: agent-scope accesses), and an iteration pops fewer tasks when the stack could not take their children.  A library
    built with 32-entry stacks (-DWP_CAP=32u: nearly every push of the big scenes spills) must render the frames of the product, bit for bit -- the atrium and the glass
    room under PHIP_FLAG_FUSED_ANY (ten node visits per ray), the spheres, `direct`."""
    import subprocess, sys
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available: the small-stack library cannot be built")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from mitsuba_amd import _ffi
    lib = _ffi.build_test_variant("cap32")        # (prebuilt by __graft_entry__.build(), as the fault-injection library above)
    script = r"""
import sys, os
sys.path.insert(0, %r)
import numpy as np
from mitsuba_amd import _ffi, _abi as A, scene as S
from mitsuba_amd.integrator import Scene, PathHIP, DirectHIP, HDRFilm
ft = _ffi.gaussian_filter(0.5)
out = {}
for name, sb, spp, integ in (("atrium", S.atrium(96, 54, ft, detail=0.3), 4, PathHIP(maxDepth=6)), ("glass", S.glass_room(96, 54, ft, detail=0.3), 4, PathHIP(maxDepth=10)),
                             ("spheres", S.cornell_spheres(96, 96, ft), 4, PathHIP(maxDepth=6)), ("direct", S.cornell_spheres(96, 96, ft), 4, DirectHIP(shadingSamples=2))):
    gs = Scene(sb.desc()); film = HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER | A.PHIP_FLAG_FUSED_ANY)
    assert integ.stats.fused == 1, name
    out[name] = integ.samples(gs, spp).copy(); out[name + "_film"] = film.storage.copy()
    gs.close()
np.savez(sys.argv[1], **out)
""" % root
    res = {}
    for tag, e in (("product", {}), ("cap32", {"PHIP_LIB": lib})):
        f = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", script, f], env=dict(os.environ, **e), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "warning" not in r.stderr, r.stderr[-800:]           # (no pass gave up: the stack spilled, it did not overflow)
        res[tag] = np.load(f)
    for name in ("atrium", "glass", "spheres", "direct"):
        assert (res["product"][name].view(np.uint32) == res["cap32"][name].view(np.uint32)).all(), name
        assert (res["product"][name + "_film"].view(np.uint32) == res["cap32"][name + "_film"].view(np.uint32)).all(), name


# ---- a fused pass that gives up (k_mega.h: the ST_GAVE_UP row; phip.hip: the continuation on the wavefront kernels; k_wide_wave.h: the bounded task stack) ----
# One child process per library (PHIP_LIB is read when the library is loaded); inside it the fault knobs of the fault-injection build (PHIP_TEST_FAULT_WAVES / _PASS /
# _SHORT) and PHIP_MAX_PASS_SAMPLES are read at every render call, so that one child renders every case of a test.  Each case is announced on stderr, so that the
# library's warnings can be told apart by case.
_GIVE_UP_CHILD = r"""
import sys, os, json
import ctypes as C
sys.path.insert(0, %r)
import numpy as np
from mitsuba_amd import _ffi, _abi as A, scene as S
from mitsuba_amd.integrator import Scene, PathHIP, DirectHIP, VolPathSimpleHIP, HDRFilm
ft = _ffi.gaussian_filter(0.5)
KNOBS = ("PHIP_TEST_FAULT_WAVES", "PHIP_TEST_FAULT_PASS", "PHIP_TEST_FAULT_SHORT", "PHIP_MAX_PASS_SAMPLES")
def scene(kind):
    if kind == "mixed": return S.cornell_mixed(96, 96, ft), PathHIP(maxDepth=6), 0
    if kind == "box": return S.cornell_box(64, 64, ft), PathHIP(maxDepth=6), 0
    if kind == "spheres": return S.cornell_spheres(96, 96, ft), PathHIP(maxDepth=6), 0
    if kind == "direct": return S.cornell_spheres(96, 96, ft), DirectHIP(shadingSamples=2), 0
    if kind == "volpath": return S.cornell_spheres(96, 96, ft), VolPathSimpleHIP(maxDepth=8), 0
    if kind == "atrium": return S.atrium(96, 54, ft, detail=0.3), PathHIP(maxDepth=6), A.PHIP_FLAG_FUSED_ANY
    if kind == "ragged": return S.cornell_spheres(100, 70, ft), PathHIP(maxDepth=6), 0
    raise ValueError(kind)
def setenv(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
out = {}
for c in json.loads(sys.argv[2]):
    name, spp = c["name"], c["spp"]
    sys.stderr.write("@@case %%s\n" %% name); sys.stderr.flush()
    sb, integ, flags = scene(c["scene"])
    gs = Scene(sb.desc())
    prog = []
    record = lambda user, dev, done, total: prog.append((done, total))
    if c.get("progressive"):
        # 3 + 5 samples in two calls, the second accumulated onto the first (test_progressive_passes_add_up_to_the_single_render); the knobs apply to the second call
        L = _ffi.lib(); block = np.zeros((gs.height, gs.width, 5), np.float32); st = A.phip_stats()
        setenv(c.get("env_first", {}))
        p = integ.params(gs, 3, flags=flags, sample_offset=0, sample_total=8)
        assert L.phip_render(gs._h, C.byref(p), _ffi.fptr(block), C.byref(st)) == 0
        first_fused = st.fused
        setenv(c.get("env", {}))
        p = integ.params(gs, 5, flags=flags | A.PHIP_FLAG_ACCUMULATE, sample_offset=3, sample_total=8, progress=record)
        assert L.phip_render(gs._h, C.byref(p), _ffi.fptr(block), C.byref(st)) == 0
        assert first_fused == 1, name
        out[name + "_film"] = block
        stats = st
    else:
        setenv(c.get("env", {}))
        film = HDRFilm(gs.width, gs.height)
        kw = dict(shard_index=c["shard"][0], shard_count=c["shard"][1]) if "shard" in c else {}
        if "devices" in c:
            kw["devices"] = c["devices"]; flags |= A.PHIP_FLAG_ALIAS_DEVICES
        else:
            flags |= A.PHIP_FLAG_SAMPLE_BUFFER; kw["progress"] = record
        assert integ.render(gs, film, spp, flags=flags, **kw)
        if flags & A.PHIP_FLAG_SAMPLE_BUFFER:
            out[name + "_samples"] = integ.samples(gs, spp).copy()
        out[name + "_film"] = film.storage.copy()
        stats = integ.stats
    out[name + "_stats"] = np.array([stats.fused, stats.samples], np.int64)
    out[name + "_progress"] = np.array(prog, np.int64).reshape(-1, 2)
    setenv({})
    gs.close()
np.savez(sys.argv[1], **out)
"""


def _give_up_runs(tmp_path, runs):
    """runs: {tag: (library path or None for the product, [case, ...])} -> {tag: (arrays, {case name: that case's stderr})}"""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for tag, (lib, cases) in runs.items():
        f = str(tmp_path / (tag + ".npz"))
        env = dict(os.environ)
        for k in ("PHIP_LIB", "PHIP_TEST_FAULT_WAVES", "PHIP_TEST_FAULT_PASS", "PHIP_TEST_FAULT_SHORT", "PHIP_MAX_PASS_SAMPLES"):
            env.pop(k, None)
        if lib:
            env["PHIP_LIB"] = lib
        r = subprocess.run([sys.executable, "-c", _GIVE_UP_CHILD % root, f, json.dumps(cases)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (tag, r.stdout[-2000:] + r.stderr[-3000:])
        logs = {}
        for part in r.stderr.split("@@case ")[1:]:
            head, _, body = part.partition("\n")
            logs[head.strip()] = body
        assert sorted(logs) == sorted(c["name"] for c in cases), (tag, r.stderr[-2000:])
        res[tag] = (np.load(f), logs)
    return res


def _assert_progress(prog, what):
    """the progress values of one call: never decreasing, against one total, the last one the total"""
    assert len(prog) >= 1, what
    done, total = prog[:, 0], prog[:, 1]
    assert (np.diff(done) >= 0).all(), (what, prog.tolist())
    assert (total == total[0]).all(), (what, prog.tolist())
    assert done[-1] == total[0], (what, prog.tolist())


def _assert_same_job(prod, other, name, ref=None, samples=True):
    """`name` of the other build rendered the product's frame of case `ref`: film, sample buffer and sample count bit for bit"""
    ref = ref or name
    assert (prod[ref + "_film"].view(np.uint32) == other[name + "_film"].view(np.uint32)).all(), (name, "film")
    if samples:
        assert prod[ref + "_samples"].shape == other[name + "_samples"].shape, name
        assert (prod[ref + "_samples"].view(np.uint32) == other[name + "_samples"].view(np.uint32)).all(), (name, "sample buffer")
    assert prod[ref + "_stats"][1] == other[name + "_stats"][1], (name, "stats.samples", prod[ref + "_stats"][1], other[name + "_stats"][1])


def _need_hipcc():
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available: the test libraries cannot be built")


GAVE_UP = "warning: the fused kernel gave up"
_GIVE_UP_SCENES = (("mixed", 8), ("box", 8), ("spheres", 4))        # the mailbox build, the build of the metric, the tree in memory


def test_fused_pass_that_gives_up_is_rendered_again_however_many_waves_gave_up(gpu, gauss, tmp_path):
    """A wave of k_mega that gave up used to add 2^62 to its ST_SAMPLES entry, and the host compared the pass's sum with rc.totalIds: four poisoned waves (one block)
    sum to 2^64 = 0 and the pass was accepted, with its dropped tasks or missing samples.  Now a wave that gave up sets its entry of a row of its own (ST_GAVE_UP), and
    a pass must also count exactly one sample per crop pixel and sample of the pass.  Under the fault-injection build, wave 0, the four waves of block 0 and every wave
    give up -- with all their samples counted, one short (a stuck mailbox) or only one short (no flag: the exact count must catch it) -- and every frame must be the
    product's, bit for bit: film, sample buffer, stats.samples, with fused == 0, the warning, and progress that ends at its total."""
    _need_hipcc()
    from mitsuba_amd import _ffi
    lib = _ffi.build_test_variant("fault")
    prod_cases = [dict(name=n, scene=n, spp=spp) for n, spp in _GIVE_UP_SCENES] + \
                 [dict(name=n, scene=n, spp=4) for n in ("direct", "volpath")]
    cases = []
    for n, spp in _GIVE_UP_SCENES:
        for waves in ("wave0", "block", "all"):
            cases.append(dict(name="%s_%s" % (n, waves), scene=n, spp=spp, ref=n, env=dict(PHIP_TEST_FAULT_WAVES=waves)))
        for waves in ("block", "all"):
            cases.append(dict(name="%s_%s_short" % (n, waves), scene=n, spp=spp, ref=n, env=dict(PHIP_TEST_FAULT_WAVES=waves, PHIP_TEST_FAULT_SHORT="1")))
        cases.append(dict(name="%s_block_count_only" % n, scene=n, spp=spp, ref=n, env=dict(PHIP_TEST_FAULT_WAVES="block", PHIP_TEST_FAULT_SHORT="2")))
    for n in ("direct", "volpath"):
        cases.append(dict(name=n + "_all", scene=n, spp=4, ref=n, env=dict(PHIP_TEST_FAULT_WAVES="all")))
    res = _give_up_runs(tmp_path, {"product": (None, prod_cases), "fault": (lib, cases)})
    prod, plog = res["product"]
    fault, flog = res["fault"]
    for c in prod_cases:
        assert "warning" not in plog[c["name"]], (c["name"], plog[c["name"]][-800:])
        assert prod[c["name"] + "_stats"][0] == 1, c["name"]                          # the product ran k_mega
        _assert_progress(prod[c["name"] + "_progress"], c["name"])
    for c in cases:
        name = c["name"]
        assert GAVE_UP in flog[name], (name, flog[name][-800:])
        assert fault[name + "_stats"][0] == 0, name                                   # the frame came from the wavefront kernels
        _assert_same_job(prod, fault, name, c["ref"])
        _assert_progress(fault[name + "_progress"], name)
        assert fault[name + "_progress"][-1, 1] == prod[c["ref"] + "_progress"][-1, 1], name


def test_late_fused_pass_that_gives_up_continues_the_job(gpu, gauss, tmp_path):
    """A job of several passes (PHIP_MAX_PASS_SAMPLES) whose pass 1 or 2 gives up: the host renders the rest of the job on the wavefront kernels as a continuation --
    the same passes, the caller's sample buffer at the caller's spp (it used to be reallocated for the remaining samples and cleared, and phip_get_samples refused the
    caller's size), stats.samples and progress over the whole job.  Also the second call of a progressive 3 + 5 render (PHIP_FLAG_ACCUMULATE: the film holds the
    caller's samples) whose second pass gives up.  Every frame must be the product's multi-pass frame, bit for bit."""
    _need_hipcc()
    from mitsuba_amd import _ffi
    lib = _ffi.build_test_variant("fault")
    ids = {"mixed": 96 * 96, "box": 64 * 64, "spheres": 96 * 96}            # sample ids per sample of the whole film (block size 32: the films are whole blocks)
    prod_cases, cases = [], []
    for n, spp in _GIVE_UP_SCENES:
        multi = dict(PHIP_MAX_PASS_SAMPLES=str(ids[n] * (spp // 4)))         # four passes
        prod_cases.append(dict(name=n, scene=n, spp=spp, env=multi))
        for k in ("1", "2"):
            for waves in ("wave0", "all"):
                cases.append(dict(name="%s_pass%s_%s" % (n, k, waves), scene=n, spp=spp, ref=n, env=dict(multi, PHIP_TEST_FAULT_WAVES=waves, PHIP_TEST_FAULT_PASS=k)))
    multi = dict(PHIP_MAX_PASS_SAMPLES=str(ids["box"] * 2))                 # 3 = 2 + 1 and 5 = 2 + 2 + 1 samples
    prod_cases.append(dict(name="progressive", scene="box", spp=5, progressive=True, env_first=multi, env=multi))
    cases.append(dict(name="progressive", scene="box", spp=5, ref="progressive", progressive=True, env_first=dict(multi, PHIP_TEST_FAULT_WAVES="none"),
                      env=dict(multi, PHIP_TEST_FAULT_WAVES="all", PHIP_TEST_FAULT_PASS="1")))
    res = _give_up_runs(tmp_path, {"product": (None, prod_cases), "fault": (lib, cases)})
    prod, plog = res["product"]
    fault, flog = res["fault"]
    for c in prod_cases:
        assert "warning" not in plog[c["name"]], (c["name"], plog[c["name"]][-800:])
        assert prod[c["name"] + "_stats"][0] == 1, c["name"]
        _assert_progress(prod[c["name"] + "_progress"], c["name"])
    for c in cases:
        name = c["name"]
        log = flog[name]
        assert log.count(GAVE_UP) == 1, (name, log[-800:])                     # one pass gave up; the continuation does not run k_mega again
        first = 3 + int(c["env"]["PHIP_TEST_FAULT_PASS"]) * 2 if c.get("progressive") else int(c["env"]["PHIP_TEST_FAULT_PASS"]) * (c["spp"] // 4)
        assert "samples %d.. of the job" % first in log, (name, log[-800:])       # ... and it was the pass asked for, not the first
        assert fault[name + "_stats"][0] == 0, name
        _assert_same_job(prod, fault, name, c["ref"], samples=not c.get("progressive"))
        prog = fault[name + "_progress"]
        _assert_progress(prog, name)
        assert prog[-1, 1] == prod[c["ref"] + "_progress"][-1, 1], name
        assert len(prog) >= 2 and prog[0, 0] > 0, (name, prog.tolist())            # the passes before the one that gave up were reported, and kept


def test_task_stack_overflow_stops_the_wave_and_the_pass_is_rendered_again(gpu, gauss, tmp_path):
    """traceWidePool (k_wide_wave.h) with task stacks of 64 entries in LDS and 64 in the spill buffer (the `overflow` library): the tree-in-memory scenes outgrow them.
    A push past the stack used to be dropped while the stack's count still grew, and the pops went on to read past the wave's slice of the spill buffer -- words that
    became node indices.  Now the wave stops at the overflow, reports that it gave up, and the host renders the pass again: each scene prints the task-stack warning,
    reports fused == 0 and delivers the product's frame bit for bit; no other warning appears."""
    _need_hipcc()
    from mitsuba_amd import _ffi
    lib = _ffi.build_test_variant("overflow")
    names = ("atrium", "spheres", "direct", "volpath")
    cases = [dict(name=n, scene=n, spp=4) for n in names]
    res = _give_up_runs(tmp_path, {"product": (None, cases), "overflow": (lib, cases)})
    prod, plog = res["product"]
    small, slog = res["overflow"]
    for n in names:
        assert "warning" not in plog[n] and prod[n + "_stats"][0] == 1, (n, plog[n][-800:])
        warnings = [l for l in slog[n].splitlines() if "warning" in l]
        assert warnings and all(GAVE_UP in l and "a task stack outgrew LDS + spill buffer" in l for l in warnings), (n, slog[n][-800:])
        assert small[n + "_stats"][0] == 0, n
        _assert_same_job(prod, small, n)
        _assert_progress(small[n + "_progress"], n)


def test_ragged_film_and_a_shard_keep_the_fused_pass(gpu, gauss, tmp_path):
    """The exact sample count a fused pass must reach is the crop pixels of the device's blocks times the pass's samples -- not rc.totalIds, which counts the ids of
    edge blocks outside the film (drawn and skipped).  A 100 x 70 film and one shard of three must stay on k_mega: fused == 1, no warning, every sample counted."""
    cases = [dict(name="ragged", scene="ragged", spp=4), dict(name="shard", scene="ragged", spp=4, shard=[1, 3]),
             dict(name="ragged_multi", scene="ragged", spp=4, env=dict(PHIP_MAX_PASS_SAMPLES=str(4 * 3 * 1024)))]
    res = _give_up_runs(tmp_path, {"product": (None, cases)})
    prod, plog = res["product"]
    for c in cases:
        n = c["name"]
        assert "warning" not in plog[n], (n, plog[n][-800:])
        assert prod[n + "_stats"][0] == 1, n
        _assert_progress(prod[n + "_progress"], n)
    assert prod["ragged_stats"][1] == prod["ragged_multi_stats"][1] == 100 * 70 * 4
    assert 0 < prod["shard_stats"][1] < 100 * 70 * 4
    assert prod["shard_progress"][-1, 1] == prod["shard_stats"][1]
    assert (prod["ragged_samples"].view(np.uint32) == prod["ragged_multi_samples"].view(np.uint32)).all()


def test_device_aliases_that_give_up_deliver_the_product_frame(gpu, gauss, tmp_path):
    """Two aliases of one device (devices=[0, 0], as test_multi_device_render_equals_the_single_device_frame): under the fault build with every wave giving up, each
    device's share is rendered again on the wavefront kernels, and the merged frame is the product's merged frame, bit for bit; stats.fused is 0 (the merge used to
    OR the devices' flags)."""
    _need_hipcc()
    from mitsuba_amd import _ffi
    lib = _ffi.build_test_variant("fault")
    cases = [dict(name=n, scene=n, spp=spp, devices=[0, 0]) for n, spp in _GIVE_UP_SCENES]
    fcases = [dict(c, env=dict(PHIP_TEST_FAULT_WAVES="all")) for c in cases]
    res = _give_up_runs(tmp_path, {"product": (None, cases), "fault": (lib, fcases)})
    prod, plog = res["product"]
    fault, flog = res["fault"]
    for c in cases:
        n = c["name"]
        assert "warning" not in plog[n] and prod[n + "_stats"][0] == 1, (n, plog[n][-800:])
        assert flog[n].count(GAVE_UP) == 2, (n, flog[n][-800:])                 # once per device
        assert fault[n + "_stats"][0] == 0, n
        _assert_same_job(prod, fault, n, samples=False)

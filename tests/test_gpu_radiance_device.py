"""phip_radiance_device on the GPU (PathHIP.radiance): path-traced radiance along rays the caller wrote to device memory.

The arbiter is phip_render with PHIP_FLAG_NO_FUSED | PHIP_FLAG_SAMPLE_BUFFER: a ray whose stream key is the index of a pixel draws that pixel's counter stream, so
the camera rays of a 48 x 48 film (block size 32: edge blocks occur), built on the host from the stream's jitter (phip_debug_host_ctr_block) and the host twin of the
device's camera (phip_debug_host_camera_ray), must come back with the render's per-sample radiance, bit for bit.  Every comparison is on the uint32 view."""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, scene as S
from film_reference import ctr_jitter
from test_gpu_parity import gpu  # noqa: F401  (the fixture)
from test_gpu_shade_trace_wide import sphere_box, SIZES
from test_gpu_scene_update import move_shapes

pytestmark = pytest.mark.gpu
W = H = 48
INTEGRATORS = {"path": "PathHIP", "volpath_simple": "VolPathSimpleHIP"}
SCENES = {"cornell": lambda g: S.cornell_box(W, H, g),                                  # diffuse only, the packed leaf table
          "mixed": lambda g: S.cornell_mixed(W, H, g),                                  # glass and copper: MM_ALL and the lane deal
          "spheres": lambda g: S.cornell_spheres(W, H, g, nlon=25, nlat=11)}            # two 500-triangle spheres: past 64 records, the 8-wide tree


def camera_rays(phip, desc, offset, seed=0):
    """(W * H, 8) float32: the camera ray of sample `offset` of every pixel, in pixel order"""
    jit = ctr_jitter(W, H, 1, seed, offset)[:, :, 0, :]
    rays = np.zeros((H * W, 8), np.float32)
    ray = A.phip_ray()
    for y in range(H):
        for x in range(W):
            phip.phip_debug_host_camera_ray(C.byref(desc.camera), C.byref(desc.film), np.float32(x) + jit[y, x, 0], np.float32(y) + jit[y, x, 1], C.byref(ray))
            rays[y * W + x] = list(ray.o) + [ray.mint] + list(ray.d) + [ray.maxt]
    return rays


def radiance(integ, gs, rays, spp=1, **kw):
    import torch
    ids = kw.pop("stream_ids", None)
    if ids is not None:
        ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()
    out = integ.radiance(gs, torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda(), spp, stream_ids=ids, **kw)
    return out.cpu().numpy().view(np.uint32), integ.stats


class Case:
    pass


@pytest.fixture(scope="module")
def cases(gpu, phip, gauss):
    """per scene: the device scene, its camera rays at sample offsets 0 and 3, and per integrator and offset the render's samples and statistics -- computed once"""
    out = {}
    for name, make in SCENES.items():
        c = Case()
        c.sb = make(gauss); c.desc = c.sb.desc(); c.gs = gpu.Scene(c.desc)
        c.rays = {off: camera_rays(phip, c.desc, off) for off in (0, 3)}
        c.render = {}
        for iname, cls in INTEGRATORS.items():
            integ = getattr(gpu, cls)()
            for off in (0, 3):
                film = gpu.HDRFilm(W, H)
                assert integ.render(c.gs, film, 1, flags=A.PHIP_FLAG_NO_FUSED | A.PHIP_FLAG_SAMPLE_BUFFER, sample_offset=off, sample_total=4)
                st = integ.stats
                c.render[iname, off] = (integ.samples(c.gs, 1).reshape(H * W, 4).copy(), (st.closest_rays, st.shadow_rays, st.path_vertices, st.invalid_samples, st.samples))
        out[name] = c
    yield out
    for c in out.values():
        c.gs.close()


def want_bits(samples):
    """the render's samples as the call returns them: a sample the film rejects (non-finite or negative) contributes zero"""
    s = samples.copy()
    bad = ~np.isfinite(s).all(axis=1) | (s < 0).any(axis=1)
    s[bad] = 0
    return s.view(np.uint32), int(bad.sum())


@pytest.mark.parametrize("iname", sorted(INTEGRATORS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_camera_rays_return_the_samples_of_the_render(gpu, cases, scene, iname):
    c = cases[scene]
    integ = getattr(gpu, INTEGRATORS[iname])()
    for off in (0, 3):
        samples, (closest, shadow, vertices, invalid, n) = c.render[iname, off]
        want, bad = want_bits(samples)
        got, st = radiance(integ, c.gs, c.rays[off], 1, sample_offset=off, sample_total=4)
        print(scene, iname, off, "differing floats:", int((got != want).sum()), "invalid:", st.invalid_samples, bad)
        assert got.shape == (H * W, 4) and (got == want).all()
        assert st.invalid_samples == bad == invalid
        assert (st.closest_rays, st.shadow_rays, st.path_vertices, st.samples) == (closest, shadow, vertices, n) and n == H * W


def test_order_and_batching_do_not_matter(gpu, cases):
    c = cases["mixed"]; integ = gpu.PathHIP()
    want, _ = want_bits(c.render["path", 0][0])
    perm = np.random.default_rng(31).permutation(H * W)
    got, _ = radiance(integ, c.gs, c.rays[0][perm], 1, stream_ids=perm, sample_total=4)
    assert (got == want[perm]).all()
    half = H * W // 2 + 7
    a, _ = radiance(integ, c.gs, c.rays[0][perm[:half]], 1, stream_ids=perm[:half], sample_total=4)
    b, _ = radiance(integ, c.gs, c.rays[0][perm[half:]], 1, stream_ids=perm[half:], sample_total=4)
    assert (np.concatenate([a, b]) == want[perm]).all()
    tail, _ = radiance(integ, c.gs, c.rays[0][1000:], 1, first_stream=1000, sample_total=4)       # first_stream without keys
    assert (tail == want[1000:]).all()


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257])
def test_ray_counts(gpu, cases, n):
    c = cases["spheres"]; integ = gpu.PathHIP()
    want, _ = want_bits(c.render["path", 0][0])
    got, st = radiance(integ, c.gs, c.rays[0][:n], 1, sample_total=4)
    assert got.shape == (n, 4) and (got == want[:n]).all() and st.samples == n


def mean_of(samples):
    """float64 sum in ascending k of the (zeroed where invalid) float32 samples, divided by their number, rounded once"""
    acc = np.zeros(samples[0].shape, np.float64)
    for s in samples:
        acc = acc + s.view(np.float32).astype(np.float64)
    return (acc / float(len(samples))).astype(np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def four_spp(gpu, cases):
    """the mixed box's camera rays of sample 0 with four samples each: from four calls of one sample, and from one call"""
    c = cases["mixed"]; integ = gpu.PathHIP()
    singles = [radiance(integ, c.gs, c.rays[0], 1, sample_offset=k, sample_total=4)[0] for k in range(4)]
    got, st = radiance(integ, c.gs, c.rays[0], 4, sample_total=4)
    return c, mean_of(singles), got, st


def test_four_samples_are_the_float64_mean_of_four_calls(four_spp):
    c, want, got, st = four_spp
    assert (got == want).all() and st.samples == 4 * H * W
    assert (want != c.render["path", 0][0].view(np.uint32)).any()           # (the other three samples count)


def test_several_passes_return_the_same_bits(gpu, four_spp, monkeypatch):
    c, want, _, st1 = four_spp
    monkeypatch.setenv("PHIP_MAX_PASS_SAMPLES", str(H * W + 5))             # one sample per ray and pass: four passes
    got, st = radiance(gpu.PathHIP(), c.gs, c.rays[0], 4, sample_total=4)
    assert (got == want).all()
    assert st.iterations > st1.iterations and (st.closest_rays, st.shadow_rays, st.path_vertices) == (st1.closest_rays, st1.shadow_rays, st1.path_vertices)
    monkeypatch.setenv("PHIP_MAX_PASS_SAMPLES", str(2 * H * W))            # two passes of two
    got, _ = radiance(gpu.PathHIP(), c.gs, c.rays[0], 4, sample_total=4)
    assert (got == want).all()


def test_misses_hidden_emitters_and_a_constant_environment(gpu, gauss, cases):
    c = cases["cornell"]
    out = np.zeros((3, 8), np.float32)
    out[:, :3] = (278, 273, 100); out[:, 3] = 1e-4; out[:, 7] = np.inf
    out[:, 4:7] = [(0, 0, -1), (0.1, 0.05, -1), (-0.2, 0.1, -1)]            # through the open front of the box
    out[:, 4:7] /= np.linalg.norm(out[:, 4:7], axis=1, keepdims=True)
    got, st = radiance(gpu.PathHIP(), c.gs, out, 2)
    assert (got == 0).all() and st.closest_rays == 6 and st.shadow_rays == 0 and st.samples == 6
    # from below the area light straight up.  The light's own surface is diffuse (reflectance 0.78), so a path goes on from it: with maxDepth 1 the sample is the
    # emitted radiance alone -- (17, 12, 4), and with hideEmitters exactly 0 at alpha 1 --, at full depth hideEmitters takes that term away and leaves the rest
    up = out[:1].copy(); up[0, :3] = (278, 273, 279.5); up[0, 4:7] = (0, 1, 0)
    lit, _ = radiance(gpu.PathHIP(maxDepth=1), c.gs, up, 1)
    assert (lit.view(np.float32)[0] == np.array((17, 12, 4, 1), np.float32)).all()
    hidden, _ = radiance(gpu.PathHIP(maxDepth=1, hideEmitters=True), c.gs, up, 1)
    assert (hidden.view(np.float32)[0] == np.array((0, 0, 0, 1), np.float32)).all()
    full, _ = radiance(gpu.PathHIP(), c.gs, up, 1)
    rest, _ = radiance(gpu.PathHIP(hideEmitters=True), c.gs, up, 1)
    assert (full.view(np.float32)[0, :3] >= np.array((17, 12, 4), np.float32)).all() and (rest.view(np.float32)[0, :3] < np.array((17, 12, 4), np.float32)).all()
    assert rest.view(np.float32)[0, 3] == 1
    sb = S.SceneBuilder()
    sb.constant((0.5, 0.6, 0.8))
    S.cornell_box(W, H, gauss, sb=sb)
    gs = gpu.Scene(sb.desc())
    env, _ = radiance(gpu.PathHIP(), gs, out, 2)
    assert (env.view(np.float32) == np.array((0.5, 0.6, 0.8, 0), np.float32)).all()
    gs.close()


@pytest.mark.parametrize("kind", ["albedo", "envmap"])
def test_textured_and_environment_lit_scenes(gpu, phip, gauss, kind):
    """Equality with the render is not claimed here: the render's camera ray carries differentials, so its first vertex reads a bitmap texture through the filtered
    MIP look-up and a directly visible envmap through the EWA filter, while a caller's ray has none and reads both at level 0, bilinearly, as every later vertex
    does (include/phip.h).  What holds: the call succeeds, is deterministic, and does not depend on the order of the rays."""
    sb = sphere_box(gauss, kind, *SIZES["104"], w=W, h=H)
    desc = sb.desc(); gs = gpu.Scene(desc); integ = gpu.PathHIP()
    rays = camera_rays(phip, desc, 0)
    a, st = radiance(integ, gs, rays, 2)
    b, _ = radiance(integ, gs, rays, 2)
    assert (a == b).all() and st.samples == 2 * H * W and np.isfinite(a.view(np.float32)).all() and (a.view(np.float32)[:, :3] > 0).any()
    perm = np.random.default_rng(32).permutation(H * W)
    p, _ = radiance(integ, gs, rays[perm], 2, stream_ids=perm)
    assert (p == a[perm]).all()
    gs.close()


def test_after_update_and_after_rebuild(gpu, phip, gauss):
    sb = S.cornell_spheres(W, H, gauss, nlon=25, nlat=11)
    gs = gpu.Scene(sb.desc()); integ = gpu.PathHIP()
    rays = camera_rays(phip, sb.desc(), 0)
    before, _ = radiance(integ, gs, rays, 1)
    move_shapes(sb, [16], offset=(60.0, 40.0, -20.0), scale=(1.0, 0.7, 1.2))
    move_shapes(sb, [17], offset=(-80.0, -120.0, -60.0), rotate_y_deg=30.0)
    fresh = gpu.Scene(sb.desc())
    want, wst = radiance(integ, fresh, rays, 1)
    assert (want != before).any()
    gs.update(positions=sb.flat_positions(), normals=sb.flat_normals())
    for step in ("update", "rebuild"):
        got, st = radiance(integ, gs, rays, 1)
        assert (got == want).all(), step
        assert (st.closest_rays, st.shadow_rays, st.path_vertices) == (wst.closest_rays, wst.shadow_rays, wst.path_vertices), step
        if step == "update":
            gs.rebuild()
    gs.close(); fresh.close()


def test_refusals_leave_the_scene_unchanged(gpu, phip, cases):
    import torch
    c = cases["cornell"]; integ = gpu.PathHIP()
    want, _ = want_bits(c.render["path", 0][0])
    n = H * W
    t = torch.from_numpy(c.rays[0]).cuda(); out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    host = np.ascontiguousarray(c.rays[0]); wide = torch.empty((n * 8 + 4,), dtype=torch.float32, device="cuda")

    def call(rays=None, d_out=None, count=n, **kw):
        p = integ.params(c.gs, 1, sample_total=4, **{k: v for k, v in kw.items() if k not in ("integrator", "sampler", "n_devices")})
        for k in ("integrator", "sampler", "n_devices"):
            if k in kw:
                setattr(p, k, kw[k])
        d = A.phip_radiance_desc(d_rays=t.data_ptr() if rays is None else rays, n=count, d_stream=None, first_stream=0, reserved=0, d_out=out.data_ptr() if d_out is None else d_out)
        rc = phip.phip_radiance_device(c.gs._h, C.byref(p), C.byref(d), None)
        if rc != 0:
            assert phip.phip_last_error()
            got, _ = radiance(integ, c.gs, c.rays[0], 1, sample_total=4)
            assert (got == want).all()
        return rc

    assert call() == 0 and (out.cpu().numpy().view(np.uint32) == want).all()
    assert call(integrator=A.PHIP_INTEGRATOR_DIRECT) == A.PHIP_ERR_UNSUPPORTED
    for sampler in (A.PHIP_SAMPLER_LD, A.PHIP_SAMPLER_SOBOL, A.PHIP_SAMPLER_STRATIFIED, A.PHIP_SAMPLER_HALTON, A.PHIP_SAMPLER_HAMMERSLEY):
        assert call(sampler=sampler) == A.PHIP_ERR_UNSUPPORTED
    assert call(n_devices=2) == A.PHIP_ERR_INVALID
    assert call(rays=host.ctypes.data) == A.PHIP_ERR_INVALID                                    # a host pointer
    assert call(d_out=np.zeros((n, 4), np.float32).ctypes.data) == A.PHIP_ERR_INVALID
    assert call(rays=wide[1:].data_ptr()) == A.PHIP_ERR_INVALID                                 # 4 bytes off
    assert call(d_out=wide[1:].data_ptr()) == A.PHIP_ERR_INVALID
    assert call(count=2 ** 32 - 255) == A.PHIP_ERR_INVALID
    assert call(flags=A.PHIP_FLAG_SAMPLE_BUFFER) == A.PHIP_ERR_INVALID
    assert call(d_out=0) == A.PHIP_ERR_INVALID                                                  # d_out NULL
    if torch.cuda.device_count() > 1:
        other = torch.empty((n, 4), dtype=torch.float32, device="cuda:1")
        assert call(d_out=other.data_ptr()) == A.PHIP_ERR_INVALID                               # another device's pointer
    assert call(count=0, rays=0, d_out=0) == 0                                                  # n == 0: nothing is touched
    for bad in (t.double(), torch.from_numpy(np.tile(c.rays[0], (1, 2))).cuda()[:, :8], torch.from_numpy(c.rays[0]), t.reshape(-1)):
        with pytest.raises(ValueError):
            integ.radiance(c.gs, bad, 1)

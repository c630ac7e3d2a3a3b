"""phip_camera_rays_device, the (key, sample) pairs of phip_radiance_device and phip_film_device on the GPU: a render in parts.

The film is a ragged 37 x 23 crop window at offset (5, 3) of a 64 x 40 film over the Cornell box: two ragged blocks per row and column at block size 32, edge
blocks at 8.  The arbiters:
    camera samples    the host twins of the stream and the camera (phip_debug_host_ctr_block, phip_debug_host_camera_ray), on the uint32 view
    pairs             phip_render(PHIP_FLAG_NO_FUSED | PHIP_FLAG_SAMPLE_BUFFER): the render's per-sample radiance and counters, bit for bit, from ONE radiance call
                      (the scenes and integrators of tests/test_gpu_radiance_device.py, which holds layout 0 as it was)
    film              tests/film_reference.py: the float64 sums of the same samples at the stream's positions and its derived bound (N + 16) 2^-24 A, no new
                      number; signed values v = a - b are held to S(a) - S(b) with A(a) + A(b) in the bound (every product w * v is one float32 number on both
                      sides where a - b is exact: |film - S| <= (N + 16) u sum |w v| <= (N + 16) u (A(a) + A(b)))."""
import ctypes as C

import numpy as np
import pytest

import film_reference as FR
from mitsuba_amd import _abi as A, scene as S
from test_gpu_parity import gpu  # noqa: F401  (the fixture)
from test_gpu_radiance_device import INTEGRATORS, SCENES, W as RW, H as RH, want_bits
from test_raycast_device_host import host_surfaces

pytestmark = pytest.mark.gpu
FILM, CROP = (64, 40), (5, 3, 37, 23)
W, H = CROP[2], CROP[3]


def cropped(name):
    filt = FR.filter_named(name)
    sb = S.cornell_box(FILM[0], FILM[1], filt)
    sb.hdrfilm(FILM[0], FILM[1], filt, crop=CROP)
    return sb.desc(), filt


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def twin_samples(phip, desc, w, h, pixels, spp, seed, offset):
    """(rays [n, 8], keys [n, 2], positions [n, 2]) of the samples offset .. offset + spp - 1 of `pixels`, pixel-major, from the host twins"""
    jit = FR.ctr_jitter(w, h, spp, seed, offset)
    n = len(pixels) * spp
    rays = np.zeros((n, 8), np.float32); keys = np.zeros((n, 2), np.uint32); pos = np.zeros((n, 2), np.float32)
    ray = A.phip_ray()
    for i, p in enumerate(pixels):
        x, y = int(p) % w, int(p) // w
        for k in range(spp):
            sx, sy = np.float32(x) + jit[y, x, k, 0], np.float32(y) + jit[y, x, k, 1]
            phip.phip_debug_host_camera_ray(C.byref(desc.camera), C.byref(desc.film), sx, sy, C.byref(ray))
            rays[i * spp + k] = list(ray.o) + [ray.mint] + list(ray.d) + [ray.maxt]
            keys[i * spp + k] = (p, offset + k); pos[i * spp + k] = (sx, sy)
    return rays, keys, pos


@pytest.fixture(scope="module")
def box(gpu):
    desc, filt = cropped("gauss_r2")
    gs = gpu.Scene(desc)
    assert (gs.width, gs.height) == (W, H)
    yield gs, desc
    gs.close()


# ---- 1. the camera samples ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset,seed", [(0, 0), (5, 0), (0, 7), (5, 7)])
def test_rays_keys_and_positions_equal_the_host_twins(phip, box, offset, seed):
    gs, desc = box
    rays, keys, pos = gs.camera_rays(3, seed=seed, sample_offset=offset, positions=True)
    wr, wk, wp = twin_samples(phip, desc, W, H, np.arange(W * H), 3, seed, offset)
    assert rays.shape == (W * H * 3, 8) and keys.shape == (W * H * 3, 2) and pos.shape == (W * H * 3, 2)
    assert (u32(keys) == wk).all() and (u32(pos) == wp.view(np.uint32)).all()
    assert (u32(rays) == wr.view(np.uint32)).all(), "%d rays differ" % (u32(rays) != wr.view(np.uint32)).any(axis=1).sum()
    only, none, _ = gs.camera_rays(3, seed=seed, sample_offset=offset, keys=False)           # the optional outputs left out
    assert none is None and (u32(only) == wr.view(np.uint32)).all()


def test_a_shuffled_subset_of_pixels_with_a_repeated_index(phip, box):
    gs, desc = box
    pixels = np.random.default_rng(41).permutation(W * H)[:100].astype(np.int32)
    pixels[57] = pixels[3]
    rays, keys, pos = gs.camera_rays(3, seed=7, sample_offset=5, pixels=dev(pixels), positions=True)
    wr, wk, wp = twin_samples(phip, desc, W, H, pixels, 3, 7, 5)
    assert rays.shape == (300, 8)
    assert (u32(rays) == wr.view(np.uint32)).all() and (u32(keys) == wk).all() and (u32(pos) == wp.view(np.uint32)).all()
    import torch
    e = gs.camera_rays(3, pixels=torch.empty((0,), dtype=torch.int32, device="cuda"))
    assert e[0].shape == (0, 8) and e[1].shape == (0, 2)


# ---- 2. the render's samples in one radiance call -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scenes(gpu, gauss):
    out = {}
    yield lambda name: out[name] if name in out else out.setdefault(name, gpu.Scene(SCENES[name](gauss).desc()))
    for gs in out.values():
        gs.close()


@pytest.mark.parametrize("iname", sorted(INTEGRATORS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_one_call_with_pairs_returns_the_samples_of_the_render(gpu, scenes, scene, iname):
    gs = scenes(scene); integ = getattr(gpu, INTEGRATORS[iname])()
    for spp, offset, total in ((3, 0, 3), (2, 3, 8)):
        film = gpu.HDRFilm(RW, RH)
        assert integ.render(gs, film, spp, flags=A.PHIP_FLAG_NO_FUSED | A.PHIP_FLAG_SAMPLE_BUFFER, sample_offset=offset, sample_total=total)
        st = integ.stats
        render = (st.closest_rays, st.shadow_rays, st.path_vertices, st.samples, st.invalid_samples)
        want, bad = want_bits(integ.samples(gs, spp).reshape(RW * RH * spp, 4))
        rays, keys, _ = gs.camera_rays(spp, sample_offset=offset)
        got = integ.radiance(gs, rays, 1, pairs=keys, sample_total=total)
        st = integ.stats
        print(scene, iname, spp, offset, "differing floats:", int((u32(got) != want).sum()), "invalid:", st.invalid_samples, bad)
        assert got.shape == (RW * RH * spp, 4) and (u32(got) == want).all()
        assert (st.closest_rays, st.shadow_rays, st.path_vertices, st.samples, st.invalid_samples) == render and st.samples == RW * RH * spp and bad == st.invalid_samples


def test_pairs_with_more_than_one_sample_per_ray_count_on_from_the_pair(gpu, scenes):
    """sample k of ray i draws (key, sample + k): the rays of sample 1 with spp = 2 are the mean of the one-sample calls of samples 1 and 2 along them"""
    from test_gpu_radiance_device import mean_of
    gs = scenes("mixed"); integ = gpu.PathHIP()
    rays, keys, _ = gs.camera_rays(1, sample_offset=1)
    singles = []
    for k in (1, 2):
        kk = keys.clone(); kk[:, 1] = k
        singles.append(u32(integ.radiance(gs, rays, 1, pairs=kk, sample_total=4)))
    got = integ.radiance(gs, rays, 2, pairs=keys, sample_total=4)
    assert (u32(got) == mean_of(singles)).all() and integ.stats.samples == 2 * RW * RH
    assert (singles[0] == u32(integ.radiance(gs, rays, 1, stream_ids=keys[:, 0].contiguous(), sample_offset=1, sample_total=4))).all()      # layout 0 says the same


# ---- 3. the film against the float64 reference ---------------------------------------------------------------------------------------------------

class Shot:
    """one filter's scene on the device and its renders at maxDepth 3 (the film has no bearing on the path), the sample buffer kept"""

    def __init__(self, gpu, name):
        self.desc, self.filt = cropped(name)
        self.gs = gpu.Scene(self.desc); self.integ = gpu.PathHIP(maxDepth=3); self.gpu = gpu; self.name = name

    def render(self, bs, spp, seed, offset):
        self.gs.setBlockSize(bs)
        film = self.gpu.HDRFilm(W, H)
        assert self.integ.render(self.gs, film, spp, seed=seed, flags=A.PHIP_FLAG_SAMPLE_BUFFER, sample_offset=offset, sample_total=16)
        return film.storage, self.integ.samples(self.gs, spp)

    def sums(self, samples, bs, seed, offset):
        return FR.film_sums(samples, FR.ctr_jitter(W, H, samples.shape[2], seed, offset), self.filt[0], self.filt[1], bs)

    def signed_sums(self, a, b, bs, seed, offset):
        """v = a - b with a, b >= 0 (NaN in both where the sample is rejected): S(a) - S(b), A(a) + A(b); the weight channel is that of either"""
        sa, sb = self.sums(a, bs, seed, offset), self.sums(b, bs, seed, offset)
        Ssum, Asum = sa.S - sb.S, sa.A + sb.A
        Ssum[..., 4] = sa.S[..., 4]; Asum[..., 4] = sa.A[..., 4]
        assert (sa.N == sb.N).all() and sa.rejected == sb.rejected
        return FR.FilmSums(Ssum, Asum, sa.N, sa.rejected)

    def film(self, values, bs, seed, offset, **kw):
        self.gs.setBlockSize(bs)
        out, st = self.gs.film(dev(values), values.shape[2], seed=seed, sample_offset=offset, **kw)
        assert st.samples == W * H * values.shape[2]
        return out.cpu().numpy(), st


@pytest.fixture(scope="module")
def shots(gpu):
    out = {}
    yield lambda name: out[name] if name in out else out.setdefault(name, Shot(gpu, name))
    for s in out.values():
        s.gs.close()


@pytest.mark.parametrize("bs", [8, 32])
@pytest.mark.parametrize("name", ["box", "gauss_r2", "gauss_r4", "gauss_r6"])
def test_the_film_of_the_renders_samples(shots, name, bs):
    shot = shots(name)
    for spp, seed, offset in ((5, 0, 0), (1, 7, 3)):
        rendered, samples = shot.render(bs, spp, seed, offset)
        ref = shot.sums(samples, bs, seed, offset)
        what = "%s bs %d spp %d offset %d" % (name, bs, spp, offset)
        film, st = shot.film(samples, bs, seed, offset)
        FR.check_film(film, ref, "phip_film_device " + what)
        assert st.invalid_samples == ref.rejected and np.abs(ref.S[..., :3]).max() > 0
        FR.check_film(rendered, ref, "phip_render " + what)                                 # ... so the two films differ by at most twice the bound
        assert (np.abs(film.astype(np.float64) - rendered.astype(np.float64)) <= 2 * FR.film_bound(ref)).all()
        again, _ = shot.film(samples, bs, seed, offset, flags=A.PHIP_FLAG_KERNEL_TIMING)
        assert (again.view(np.uint32) == film.view(np.uint32)).all()                        # deterministic


@pytest.mark.parametrize("name,bs", [("gauss_r2", 8), ("gauss_r6", 32)])
def test_two_calls_accumulate(shots, name, bs):
    shot = shots(name)
    _, samples = shot.render(bs, 5, 0, 2)
    first, second = np.ascontiguousarray(samples[:, :, :2]), np.ascontiguousarray(samples[:, :, 2:])
    ref = FR.add_sums(shot.sums(first, bs, 0, 2), shot.sums(second, bs, 0, 4))
    shot.gs.setBlockSize(bs)
    out, _ = shot.gs.film(dev(first), 2, sample_offset=2)
    out2, st = shot.gs.film(dev(second), 3, sample_offset=4, out=out, accumulate=True)
    assert out2 is out and st.samples == 3 * W * H
    FR.check_film(out.cpu().numpy(), ref, "two calls %s bs %d" % (name, bs))
    FR.check_film(shot.film(samples, bs, 0, 2)[0], shot.sums(samples, bs, 0, 2), "one call of the same samples")


# ---- 4. the validity check --------------------------------------------------------------------------------------------------------------------------

def test_planted_nan_and_negative_samples_are_rejected_whole_and_counted(shots):
    shot = shots("gauss_r2")
    _, samples = shot.render(32, 5, 0, 0)
    s = samples.copy()
    rng = np.random.default_rng(43)
    for i, bad in enumerate((np.nan, np.inf, -np.inf, -1.0, -1e-30)):
        for y, x in zip(rng.integers(0, H, 6), rng.integers(0, W, 6)):
            s[y, x, i, int(rng.integers(0, 4))] = bad
    s[0, 0, 0, 3] = np.nan; s[H - 1, W - 1, 4, 0] = -2.0                                    # the corners
    ref = shot.sums(s, 32, 0, 0)
    assert ref.rejected >= 25
    film, st = shot.film(s, 32, 0, 0)
    FR.check_film(film, ref, "planted samples")
    assert st.invalid_samples == ref.rejected and np.isfinite(film).all()


@pytest.mark.parametrize("name,bs", [("gauss_r2", 32), ("gauss_r6", 8)])
def test_signed_values_reject_only_what_is_not_finite(shots, name, bs):
    shot = shots(name)
    rng = np.random.default_rng(44)
    a = (rng.integers(0, 4096, (H, W, 3, 4)) / 1024.0).astype(np.float32)                  # multiples of 2^-10 below 4: a - b is exact
    b = (rng.integers(0, 4096, (H, W, 3, 4)) / 1024.0).astype(np.float32)
    nans = 0
    for y, x, k in zip(rng.integers(0, H, 9), rng.integers(0, W, 9), rng.integers(0, 3, 9)):
        nans += 0 if np.isnan(a[y, x, k, 0]) else 1
        a[y, x, k] = np.nan; b[y, x, k] = np.nan
    v = a - b
    assert (v[np.isfinite(v)] < 0).any()
    ref = shot.signed_sums(a, b, bs, 3, 1)
    film, st = shot.film(v, bs, 3, 1, signed=True)
    FR.check_film(film, ref, "signed %s bs %d" % (name, bs))
    assert st.invalid_samples == ref.rejected == nans                                       # only the NaNs
    _, st = shot.film(v, bs, 3, 1)                                                          # the film's own check counts the negative ones too
    assert st.invalid_samples == int((~np.isfinite(v).all(axis=-1) | (v < 0).any(axis=-1)).sum()) > nans


# ---- 5. a feature buffer end to end -------------------------------------------------------------------------------------------------------------------

def test_shading_normal_and_depth_on_the_film(phip, shots):
    shot = shots("gauss_r2"); gs = shot.gs
    spp, seed, bs = 2, 5, 32
    rays, _, _ = gs.camera_rays(spp, seed=seed, keys=False)
    hits, _, surf, _ = gs.rayIntersectDevice(rays, closest=True, surfaces=True)
    values = surf[:, [8, 9, 10, 3]].contiguous()                                            # (ns, t) of phip_surface
    gs.setBlockSize(bs)
    film, st = gs.film(values, spp, seed=seed, signed=True)
    words = host_surfaces(phip, shot.desc, rays.cpu().numpy(), hits.cpu().numpy())
    v = np.ascontiguousarray(words[:, [8, 9, 10, 3]]).view(np.float32).reshape(H, W, spp, 4)
    assert (u32(values).reshape(v.shape) == v.view(np.uint32)).all()
    bad = ~np.isfinite(v).all(axis=-1)
    a, b = np.maximum(v, 0), np.maximum(-v, 0)                                              # v = a - b, one of the two is zero
    a[bad] = np.nan; b[bad] = np.nan
    ref = shot.signed_sums(a, b, bs, seed, 0)
    FR.check_film(film.cpu().numpy(), ref, "normal and depth")
    assert st.invalid_samples == ref.rejected == int(bad.sum())
    assert (v[..., :3] < 0).any() and (v[..., 3] > 0).any() and np.abs(ref.S[..., :3]).max() > 0


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(phip, box):
    import torch
    gs, desc = box
    INV = A.PHIP_ERR_INVALID
    n = W * H * 2
    mark = 12345.0
    rays = torch.full((n * 8 + 4,), mark, device="cuda"); keys = torch.full((n * 2 + 2,), 77, dtype=torch.int32, device="cuda"); pos = torch.full((n * 2 + 2,), mark, device="cuda")
    film = torch.full((H * W * 5 + 4,), mark, device="cuda"); values = torch.zeros((H * W * 2 * 4 + 4,), device="cuda")
    host = np.zeros(n * 8 + 8, np.float32)
    p = A.default_render_params(spp=2, device=gs.device)

    def cam(**kw):
        d = A.phip_camera_rays_desc(**dict(dict(d_pixels=None, m=0, d_rays=rays.data_ptr(), d_keys=keys.data_ptr(), d_positions=pos.data_ptr()), **kw))
        rc = phip.phip_camera_rays_device(gs._h, C.byref(p), C.byref(d))
        assert rc == 0 or phip.phip_last_error().startswith(b"phip_camera_rays_device: ")
        return rc

    def put(**kw):
        d = A.phip_film_desc(**dict(dict(d_values=values.data_ptr(), d_out=film.data_ptr(), flags=0, reserved=0), **kw))
        rc = phip.phip_film_device(gs._h, C.byref(p), C.byref(d), None)
        assert rc == 0 or phip.phip_last_error().startswith(b"phip_film_device: ")
        return rc

    assert cam(d_rays=host.ctypes.data) == INV and cam(d_keys=host.ctypes.data) == INV and cam(d_positions=host.ctypes.data) == INV      # host pointers
    assert cam(d_rays=rays[1:].data_ptr()) == INV and cam(d_keys=keys[1:].data_ptr()) == INV and cam(d_positions=pos[1:].data_ptr()) == INV      # 4 bytes off
    assert cam(d_rays=rays[2:].data_ptr()) == INV                                                                                             # 8 bytes off: rays want 16
    assert cam(d_rays=None) == INV
    pixels = torch.arange(W * H, dtype=torch.int32, device="cuda")
    pixels[W * H - 3] = W * H                                                                # one past the crop window
    assert cam(d_pixels=pixels.data_ptr(), m=W * H) == INV
    pixels[W * H - 3] = -1
    assert cam(d_pixels=pixels.data_ptr(), m=W * H) == INV
    assert cam(d_pixels=pixels.data_ptr(), m=W * H - 3) == 0                                 # the list ends before the bad entry
    assert (rays[(W * H - 3) * 16:] == mark).all() and (rays[:(W * H - 3) * 16] != mark).any()
    assert (keys[(W * H - 3) * 4:] == 77).all() and (pos[(W * H - 3) * 4:] == mark).all()
    rays.fill_(mark); keys.fill_(77); pos.fill_(mark)
    assert cam(d_pixels=host.ctypes.data, m=4) == INV
    p.sampler = A.PHIP_SAMPLER_SOBOL
    assert cam() == A.PHIP_ERR_UNSUPPORTED and put() == A.PHIP_ERR_UNSUPPORTED
    p.sampler = A.PHIP_SAMPLER_CTR
    assert put(d_values=host.ctypes.data) == INV and put(d_out=host.ctypes.data) == INV
    assert put(d_values=values[1:].data_ptr()) == INV and put(d_out=film[2:].data_ptr()) == INV and put(d_out=None) == INV and put(flags=4) == INV
    p.shard_count = 2
    assert put() == INV
    p.shard_count = 1; p.block_size = 1
    assert put() == INV
    p.block_size = 32
    assert (rays == mark).all() and (keys == 77).all() and (pos == mark).all() and (film == mark).all()      # nothing was written
    assert cam() == 0 and put() == 0
    assert (rays[:n * 8] != mark).any() and (film[:H * W * 5] != mark).all() and (rays[n * 8:] == mark).all() and (film[H * W * 5:] == mark).all()

"""Every film kernel of mitsuba_amd/csrc/k_film.h held PER PIXEL to a float64 sum of its own samples.

The render keeps its per-sample radiance (PHIP_FLAG_SAMPLE_BUFFER); tests/film_reference.py -- a numpy restatement of ImageBlock::put that
tests/test_film_reference.py pins to the oracle -- puts exactly those samples at the counter stream's positions and returns, per pixel and channel,
S = sum of w * v and A = sum of |w * v| in float64 and the number of terms N.  The film kernel is thereby tested in isolation from the path kernels.  At
every pixel and channel, nothing left out:

    |film - S| <= (N + 16) * 2^-24 * A,        film == 0 exactly where A == 0,        stats.invalid_samples == the helper's count.

Derivation of the bound (it is not measured and has no slack beyond it): the film entry is a float32 sum of N products w * v, w = wx * wy being the same
float32 number on both sides.  Each product rounds once (not at all under a fused multiply-add), each of the N - 1 additions once, whatever their order
and grouping: the computed value is sum of t_i (1 + d_i) with |d_i| <= (1 + u)^depth - 1, u = 2^-24, depth <= N.  Grouping the sum -- per source pixel in
registers, per 16 x 16 patch in LDS, at most nine patch images in the merge, the passes of a call, the calls of a frame, the three shards of a film --
adds at most 9 + 3 + 1 + 2 < 16 further additions to a term's chain.  Hence |film - S| <= ((1 + u)^(N + 15) - 1) * A <= (N + 16) u A for N < 2^19.

The sequence samplers (sobol, halton, stratified) have no host twin that hands out their positions: there the reference is the oracle's film of the same
phip_render_params, the samples being bit-identical first.  Both films are float32 sums of the same at most N_max = (2 reach + 1)^2 spp nonnegative terms
(gaussian tables), so A = S for both and |g - o| <= 2 (N_max + 16) 2^-24 max(g, o).

Each case names the kernel it means to reach and asserts it against `film_kernel`, filmPass's selection (host_render.h) restated: a change of the selection
fails here instead of silently moving the coverage.  Kernels reached:
    splat<1> + merge<1>     box, tent, gauss_r1 at block size >= 16                      splat<1, QMC>   the sequence samplers on gauss_r1
    splat<2> + merge<2>     gauss_r2, mitchell, catmullrom, gauss_r2.49 at >= 16        splat<2, QMC>   the sequence samplers on gauss_r2
    tiled<2>                the same filters at block sizes 2, 4, 8
    tiled<4>                gauss_r2.5, lanczos3, gauss_r4, gauss_r4.49
    k_film<false>           gauss_r4.5, gauss_r6
    k_film<true>            the sequence samplers at block size 8, on gauss_r4 and on gauss_r6
"""
import ctypes as C

import numpy as np
import pytest

import film_reference as FR
from mitsuba_amd import _abi as A, scene as S

pytestmark = pytest.mark.gpu

RAGGED = (70, 50)       # two ragged blocks per row and column at every block size from 4 to 64


@pytest.fixture(scope="module")
def gpu(phip):
    if phip.phip_device_count() <= 0:
        pytest.fail("no HIP device visible: " + phip.phip_last_error().decode())
    from mitsuba_amd import integrator
    return integrator


def film_kernel(radius, block_size, sequence_sampler):
    """filmPass's selection (host_render.h), restated"""
    reach = FR.reach_of(radius)
    if reach <= 2 and block_size >= 16:
        return "splat<%d%s>" % (1 if reach <= 1 else 2, ", QMC" if sequence_sampler else "")
    if sequence_sampler:
        return "k_film<true>"
    if reach <= 4:
        return "tiled<2>" if reach <= 2 else "tiled<4>"
    return "k_film<false>"


# one filter and block size per kernel family of the counter stream
FAMILIES = [("splat<2>", "gauss_r2", 32), ("splat<1>", "tent", 32), ("tiled<2>", "mitchell", 8), ("tiled<4>", "lanczos3", 32), ("k_film<false>", "gauss_r6", 32)]
FAMILY_IDS = [f[0] for f in FAMILIES]


def _desc(name, size=RAGGED, crop=None, light_scale=1.0):
    filt = FR.filter_named(name)
    sb = S.cornell_box(size[0], size[1], filt, light_scale=light_scale)
    if crop is not None:
        sb.hdrfilm(size[0], size[1], filt, crop=crop)
    return sb.desc()


class Shot:
    """one scene on the device, rendered at maxDepth 3 (the film has no bearing on the path) with the sample buffer kept"""

    def __init__(self, gpu, name, bs, size=RAGGED, crop=None, light_scale=1.0):
        self.filt = FR.filter_named(name)
        self.desc = _desc(name, size, crop, light_scale)
        self.gs = gpu.Scene(self.desc); self.gs.setBlockSize(bs)
        self.integ = gpu.PathHIP(maxDepth=3)
        self.W, self.H, self.bs, self.gpu = self.gs.width, self.gs.height, bs, gpu
        self.what = "%s r %.2f bs %d %dx%d" % (name, self.filt[0], bs, self.W, self.H)

    def render(self, spp, **kw):
        """(film [H, W, 5], samples [H, W, spp, 4], statistics)"""
        film = self.gpu.HDRFilm(self.W, self.H)
        assert self.integ.render(self.gs, film, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER, **kw)
        return film.storage, self.integ.samples(self.gs, spp), self.integ.stats

    def sums(self, samples, seed=0, sample_offset=0, blocks=None):
        spp = samples.shape[2]
        return FR.film_sums(samples, FR.ctr_jitter(self.W, self.H, spp, seed, sample_offset), self.filt[0], self.filt[1], self.bs, blocks=blocks)

    def check(self, spp, what="", **kw):
        """one render against the float64 sums of its own samples"""
        film, smp, st = self.render(spp, **kw)
        ref = self.sums(smp, kw.get("seed", 0), kw.get("sample_offset", 0))
        assert st.samples == self.W * self.H * spp
        FR.check_film(film, ref, "%s %d spp %s" % (self.what, spp, what))
        assert st.invalid_samples == ref.rejected
        assert np.abs(ref.S[..., :3]).max() > 0 or what == "negative light"
        return film, smp, ref

    def close(self):
        self.gs.close()


def _shot(gpu, kernel, name, bs, **kw):
    assert film_kernel(FR.filter_named(name)[0], bs, False) == kernel, (name, bs, kernel)
    return Shot(gpu, name, bs, **kw)


def _pass_limit(shot, spp_per_pass, shard_count=1):
    """PHIP_MAX_PASS_SAMPLES for passes of spp_per_pass samples per pixel: the sample buffer of a pass holds block_size^2 ids per local block and sample"""
    tiles = -(-shot.W // shot.bs) * -(-shot.H // shot.bs)
    local = max(len(range(r, tiles, shard_count)) for r in range(shard_count))
    return str(spp_per_pass * local * shot.bs * shot.bs)


# ---- filters -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kernel", [
    ("box", "splat<1>"), ("tent", "splat<1>"), ("gauss_r1", "splat<1>"),
    ("gauss_r2", "splat<2>"), ("mitchell", "splat<2>"), ("catmullrom", "splat<2>"), ("gauss_r2.49", "splat<2>"),
    ("gauss_r2.5", "tiled<4>"), ("lanczos3", "tiled<4>"), ("gauss_r4", "tiled<4>"), ("gauss_r4.49", "tiled<4>"),
    ("gauss_r4.5", "k_film<false>"), ("gauss_r6", "k_film<false>")])
def test_every_filter_on_the_ragged_film(gpu, name, kernel):
    """radius and reach of every row of the table, the reach boundaries 2.49 | 2.5 and 4.49 | 4.5 included, negative lobes (mitchell, catmullrom, lanczos)"""
    shot = _shot(gpu, kernel, name, 32)
    shot.check(4)
    shot.close()


@pytest.mark.parametrize("name", ["box", "mitchell", "catmullrom", "gauss_r2.49"])
def test_filters_of_reach_up_to_two_on_small_blocks(gpu, name):
    """the same tables through the LDS-tiled gather of block sizes below 16"""
    shot = _shot(gpu, "tiled<2>", name, 8)
    shot.check(4, seed=5)
    shot.close()


# ---- block sizes ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bs", [2, 4, 8, 16, 32, 64, 128])
@pytest.mark.parametrize("name", ["tent", "gauss_r2", "gauss_r4"])
def test_block_sizes_by_reach(gpu, name, bs):
    """reach 1, 2 and 4 at every block size: 2 and 4 on a 30 x 22 film, 128 on 150 x 140 (two ragged blocks per axis, 8 x 8 patches per block)"""
    size = (30, 22) if bs <= 4 else (150, 140) if bs == 128 else RAGGED
    reach = FR.reach_of(FR.filter_named(name)[0])
    kernel = ("splat<%d>" % reach) if reach <= 2 and bs >= 16 else "tiled<2>" if reach <= 2 else "tiled<4>"
    shot = _shot(gpu, kernel, name, bs, size=size)
    if bs < FR.border_of(shot.filt[0]):
        # reach 4 has a border of 4 pixels: a block of 2 is refused, as the reference refuses it (renderproc.cpp:175-176) -- there is no such film
        with pytest.raises(RuntimeError, match="block size"):
            shot.render(4)
    else:
        shot.check(4)
    shot.close()


# ---- samples per pixel -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spp", [1, 4, 5, 9])
@pytest.mark.parametrize("kernel,name,bs", FAMILIES, ids=FAMILY_IDS)
def test_samples_per_pixel(gpu, kernel, name, bs, spp):
    """5 and 9 leave padding samples behind the pass's last in the splat's prefetch ring of four"""
    shot = _shot(gpu, kernel, name, bs)
    shot.check(spp)
    shot.close()


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,name,bs", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("shape", ["one_block", "smaller_than_a_patch", "crop_window"])
def test_film_shapes(gpu, kernel, name, bs, shape):
    """a film of exactly one block; one smaller than a 16 x 16 patch; the crop window (37, 21, 50, 45) of a 128 x 128 film"""
    kw = dict(one_block=dict(size=(bs, bs)), smaller_than_a_patch=dict(size=(11, 7)), crop_window=dict(size=(128, 128), crop=(37, 21, 50, 45)))[shape]
    shot = _shot(gpu, kernel, name, bs, **kw)
    shot.check(4)
    shot.close()


# ---- passes and calls -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,name,bs", FAMILIES, ids=FAMILY_IDS)
def test_several_passes_accumulate(gpu, monkeypatch, kernel, name, bs):
    """5 spp rendered as 2 + 2 + 1: every pass but the first adds onto the film"""
    shot = _shot(gpu, kernel, name, bs)
    single, smp1, _ = shot.check(5, "one pass")
    monkeypatch.setenv("PHIP_MAX_PASS_SAMPLES", _pass_limit(shot, 2))
    multi, smp3, _ = shot.check(5, "passes of 2")
    assert (smp1.view(np.uint32) == smp3.view(np.uint32)).all()
    assert not (single.view(np.uint32) == multi.view(np.uint32)).all(), "the same bits: the render did not run as several passes"
    shot.close()


@pytest.mark.parametrize("kernel,name,bs", FAMILIES, ids=FAMILY_IDS)
def test_two_calls_accumulate(gpu, phip, kernel, name, bs):
    """8 spp as a call of 3 and a call of 5 (sample_offset / sample_total), the second with PHIP_FLAG_ACCUMULATE onto the first's film.  The sample buffer
    holds one call and excludes that flag, so the second call runs twice: first on its own with its samples kept, then -- behind the first call, whose film
    the library holds -- accumulating"""
    shot = _shot(gpu, kernel, name, bs)
    f2, s2, r2 = shot.check(5, "call 2", sample_offset=3, sample_total=8)
    f1, s1, r1 = shot.check(3, "call 1", sample_offset=0, sample_total=8)
    p = shot.integ.params(shot.gs, 5, flags=A.PHIP_FLAG_ACCUMULATE, sample_offset=3, sample_total=8)
    acc = np.zeros_like(f1); st = A.phip_stats()                           # (the film of the previous call is the library's, not the caller's buffer)
    assert phip.phip_render(shot.gs._h, C.byref(p), acc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)) == 0
    FR.check_film(acc, FR.add_sums(r1, r2), shot.what + " 3 + 5 spp accumulated")
    assert st.invalid_samples == r2.rejected
    # ... and the frame is the one call of 8
    whole, s8, _ = shot.check(8, "one call")
    assert (np.concatenate([s1, s2], axis=2).view(np.uint32) == s8.view(np.uint32)).all()
    shot.close()


# ---- shards ---------------------------------------------------------------------------------------------------------------------------------------------

def _check_shards(shot, spp, n=3, what="", **kw):
    """each shard's film against the sums over that shard's blocks (the spiral of film_reference.shard_blocks, which tests/test_film_reference.py pins to the
    oracle's shard renders -- and the shard's own sample buffer must be the frame's samples on exactly those blocks), the films summed against the frame's"""
    whole, smp, ref = shot.check(spp, what + "unsharded", **kw)
    total = np.zeros_like(whole)
    rejected = 0
    ys, xs = np.arange(shot.H) // shot.bs, np.arange(shot.W) // shot.bs
    for r in range(n):
        film, ssmp, st = shot.render(spp, shard_index=r, shard_count=n, **kw)
        blocks = FR.shard_blocks(shot.W, shot.H, shot.bs, r, n)
        assert blocks.any()
        own = blocks[ys[:, None], xs[None, :]]
        assert (ssmp[own].view(np.uint32) == smp[own].view(np.uint32)).all() and not ssmp[~own].any()
        part = shot.sums(ssmp, kw.get("seed", 0), blocks=blocks)
        FR.check_film(film, part, "%s %sshard %d of %d" % (shot.what, what, r, n))
        assert st.invalid_samples == part.rejected
        rejected += st.invalid_samples
        total += film
    assert rejected == ref.rejected
    return whole, total, ref


@pytest.mark.parametrize("kernel,name,bs", FAMILIES, ids=FAMILY_IDS)
def test_shards(gpu, kernel, name, bs):
    """shard_count = 3 on blocks of 16 (8 for the small-block gather): 20 and 63 blocks dealt round the spiral, seams everywhere"""
    bs = min(bs, 16)
    shot = _shot(gpu, kernel, name, bs)
    whole, total, ref = _check_shards(shot, 4)
    FR.check_film(total, ref, shot.what + " three shards summed")
    shot.close()


# ---- rejected samples ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,name,bs", FAMILIES, ids=FAMILY_IDS)
def test_invalid_samples_are_rejected_and_counted(gpu, oracle, kernel, name, bs):
    """a light of negative radiance: every sample that reaches it is negative and put() refuses it whole.  The film, its weight channel included, is the sum
    over the accepted samples; the count is the helper's and the oracle's, and neither none nor all"""
    shot = _shot(gpu, kernel, name, bs, light_scale=-1.0)
    film, smp, ref = shot.check(5, "negative light")
    assert 0 < ref.rejected < shot.W * shot.H * 5
    assert ((smp < 0).any(axis=-1).sum()) == ref.rejected
    osc = oracle.OracleScene(shot.desc)
    _, _, ost = osc.render(shot.integ.params(shot.gs, 5))
    osc.close()
    assert ost.invalid_samples == ref.rejected == shot.integ.stats.invalid_samples
    assert (film[..., 4] > 0).any() and (ref.N > 0).any()
    shot.close()


# ---- the sequence samplers: against the oracle's film ----------------------------------------------------------------------------------------------------------

def _sampler_kw(sampler, W, H):
    from conftest import sobol_tables, qmc_tables
    return dict(sobol=dict(sobol=sobol_tables(W, H)), halton=dict(sampler=A.PHIP_SAMPLER_HALTON, qmc=qmc_tables(-1)),
                stratified=dict(sampler=A.PHIP_SAMPLER_STRATIFIED, seed=5))[sampler]


def _check_against_oracle(shot, oracle, film, smp, st, spp, what, **kw):
    """film against the oracle's of the same phip_render_params, per pixel: samples bit-identical first, then |g - o| <= 2 (N_max + 16) 2^-24 max(g, o)"""
    assert min(shot.filt[1]) >= 0
    osc = oracle.OracleScene(shot.desc)
    ofilm, osmp, ost = osc.render(shot.integ.params(shot.gs, spp, **kw), want_samples=True)
    osc.close()
    assert (smp.view(np.uint32) == osmp.view(np.uint32)).all(), "%s: the samples are not the oracle's" % what
    n_max = (2 * FR.reach_of(shot.filt[0]) + 1) ** 2 * spp
    g, o = film.astype(np.float64), ofilm.astype(np.float64)
    bound = 2 * (n_max + 16) * 2.0 ** -24 * np.maximum(g, o)
    err = np.abs(g - o)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("%s %s: worst |g - o| / bound = %.3f" % (shot.what, what, float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))))
    over = ~(err <= bound)
    assert not over.any(), "%s %s: %d entries over the bound, first at (y, x, c) = %s: gpu %r oracle %r" % (
        shot.what, what, int(over.sum()), tuple(np.argwhere(over)[0]), film[tuple(np.argwhere(over)[0])], ofilm[tuple(np.argwhere(over)[0])])
    assert (o > 0).any() and st.invalid_samples == ost.invalid_samples


QMC_CASES = [("splat<1, QMC>", "gauss_r1", 32), ("splat<2, QMC>", "gauss_r2", 32), ("k_film<true>", "gauss_r2", 8), ("k_film<true>", "gauss_r4", 32),
             ("k_film<true>", "gauss_r6", 32)]


@pytest.mark.parametrize("sampler", ["sobol", "halton", "stratified"])
@pytest.mark.parametrize("kernel,name,bs", QMC_CASES, ids=["%s-%s-bs%d" % c for c in QMC_CASES])
def test_sequence_samplers_against_the_oracles_film(gpu, oracle, kernel, name, bs, sampler):
    assert film_kernel(FR.filter_named(name)[0], bs, True) == kernel
    shot = Shot(gpu, name, bs)
    kw = _sampler_kw(sampler, shot.W, shot.H)
    film, smp, st = shot.render(4, **kw)
    _check_against_oracle(shot, oracle, film, smp, st, 4, sampler, **kw)
    shot.close()


@pytest.mark.parametrize("sampler", ["sobol", "halton", "stratified"])
def test_sequence_samplers_gather_over_several_passes(gpu, oracle, monkeypatch, sampler):
    """k_film<true>, 9 spp as 4 + 4 + 1"""
    assert film_kernel(FR.filter_named("gauss_r4")[0], 32, True) == "k_film<true>"
    shot = Shot(gpu, "gauss_r4", 32)
    kw = _sampler_kw(sampler, shot.W, shot.H)
    single, _, _ = shot.render(9, **kw)
    monkeypatch.setenv("PHIP_MAX_PASS_SAMPLES", _pass_limit(shot, 4))
    film, smp, st = shot.render(9, **kw)
    assert not (single.view(np.uint32) == film.view(np.uint32)).all(), "the same bits: the render did not run as several passes"
    _check_against_oracle(shot, oracle, film, smp, st, 9, sampler + " passes of 4", **kw)
    shot.close()


@pytest.mark.parametrize("sampler", ["sobol", "halton", "stratified"])
def test_sequence_samplers_gather_on_shards(gpu, oracle, sampler):
    """k_film<true> on the three shards of a film of 8 x 8 blocks: each shard's film against the oracle's render of that shard"""
    assert film_kernel(FR.filter_named("gauss_r2")[0], 8, True) == "k_film<true>"
    shot = Shot(gpu, "gauss_r2", 8)
    kw = _sampler_kw(sampler, shot.W, shot.H)
    whole, wsmp, _ = shot.render(4, **kw)
    total = np.zeros_like(whole)
    for r in range(3):
        film, smp, st = shot.render(4, shard_index=r, shard_count=3, **kw)
        _check_against_oracle(shot, oracle, film, smp, st, 4, "%s shard %d of 3" % (sampler, r), shard_index=r, shard_count=3, **kw)
        total += film
    # three float32 additions of nonnegative numbers on top of the two sums
    n_max = (2 * 2 + 1) ** 2 * 4
    assert (np.abs(total.astype(np.float64) - whole) <= 2 * (n_max + 16) * 2.0 ** -24 * np.maximum(total, whole)).all()
    shot.close()

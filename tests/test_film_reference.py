"""tests/film_reference.py pinned before anything trusts it (no GPU): the oracle -- whose ImageBlock::put is pinned to the reference's -- renders with its
per-sample radiance exported, the helper sums those samples in float64, and the oracle's float32 film must lie within the forward bound
(N + 16) * 2^-24 * A of the helper's sums at EVERY pixel and channel.  The oracle adds a block's terms in float32 one by one and then at most nine
block bitmaps per film pixel: the bound with factor 1, nothing more.  This settles the helper's conventions (pixel index and sample index of the counter
stream's host twin, block-local float32 positions, the clipped footprint, the spiral of the shards, the rejection rule) against the CPU side alone."""
import numpy as np
import pytest

import film_reference as FR
from mitsuba_amd import _abi as A, scene as S


def _cornell(width, height, filt, crop=None, light_scale=1.0):
    sb = S.cornell_box(width, height, filt, light_scale=light_scale)
    if crop is not None:
        sb.hdrfilm(width, height, filt, crop=crop)
    return sb.desc()


def _pin(oracle, phip, desc, filt, bs, spp=4, seed=0, shard=None, what=""):
    """the oracle's film of `desc` against the helper on the oracle's samples; returns (helper sums, oracle statistics)"""
    osc = oracle.OracleScene(desc)
    kw = dict(shard_index=shard[0], shard_count=shard[1]) if shard else {}
    ofilm, osmp, ost = osc.render(A.default_render_params(spp=spp, max_depth=3, block_size=bs, seed=seed, **kw), want_samples=True)
    osc.close()
    W, H = desc.film.crop_width, desc.film.crop_height
    blocks = FR.shard_blocks(W, H, bs, *shard) if shard else None
    ref = FR.film_sums(osmp, FR.ctr_jitter(W, H, spp, seed), filt[0], filt[1], bs, blocks=blocks)
    FR.check_film(ofilm, ref, what)
    assert ref.rejected == ost.invalid_samples
    assert ref.N.max() > 0 and np.abs(ref.S).max() > 0
    return ref, ost


@pytest.mark.parametrize("name,bs", [("gauss_r2", 32), ("gauss_r2", 8), ("gauss_r2", 64), ("gauss_r1", 32), ("gauss_r6", 32), ("gauss_r6", 8),
                                     ("mitchell", 16), ("box", 32)])
def test_oracle_film_on_the_ragged_film_is_the_float64_sum_of_its_samples(oracle, phip, name, bs):
    """70 x 50: ragged right and bottom blocks for every block size; radii 1.0, 2.0 and 6.0 (borders 1, 2 and 6), block sizes 8 and 64; a filter
    with negative lobes; the box, whose border is 0"""
    filt = FR.filter_named(name)
    _pin(oracle, phip, _cornell(70, 50, filt), filt, bs, seed=3 if bs == 8 else 0, what="%s bs %d" % (name, bs))


@pytest.mark.parametrize("name", ["gauss_r2", "gauss_r6"])
def test_oracle_film_on_a_crop_window_off_the_origin(oracle, phip, name):
    """blocks, pixel indices and positions are relative to the crop window"""
    filt = FR.filter_named(name)
    _pin(oracle, phip, _cornell(128, 128, filt, crop=(37, 21, 50, 45)), filt, 32, what="crop " + name)


def test_oracle_shard_films_are_the_sums_over_the_shards_blocks(oracle, phip):
    """the spiral of film_reference.shard_blocks is the oracle's: each shard's film is the sum over that shard's blocks, and the shards partition the blocks"""
    filt = FR.filter_named("gauss_r2")
    desc = _cornell(70, 50, filt)
    whole, _ = _pin(oracle, phip, desc, filt, 16, what="whole")
    parts = [_pin(oracle, phip, desc, filt, 16, shard=(r, 3), what="shard %d of 3" % r)[0] for r in range(3)]
    total = np.sum([FR.shard_blocks(70, 50, 16, r, 3) for r in range(3)], axis=0)
    assert (total == 1).all()
    assert sorted(FR.spiral_blocks(70, 50, 16)) == [(x, y) for x in range(5) for y in range(4)]
    np.testing.assert_allclose(sum(p.S for p in parts), whole.S, rtol=1e-12, atol=1e-300)
    assert (sum(p.N for p in parts) == whole.N).all()


def test_oracle_rejects_what_the_helper_rejects(oracle, phip):
    """a light of negative radiance: every sample that reaches it is negative and put() refuses it -- some samples, not all; the film, its weight
    channel included, is the sum over the accepted ones"""
    filt = FR.filter_named("gauss_r2")
    ref, ost = _pin(oracle, phip, _cornell(70, 50, filt, light_scale=-1.0), filt, 32, what="negative light")
    assert 0 < ref.rejected < 70 * 50 * 4
    assert ref.rejected == ost.invalid_samples


def test_filter_tables_have_the_reach_they_are_meant_to_have():
    for name, (build, reach) in FR.FILTERS.items():
        radius, table = FR.filter_named(name)
        assert FR.reach_of(radius) == reach, (name, radius)
        assert len(table) == 32 and table[31] == 0.0 and np.isfinite(table).all()
        assert abs(sum(table) * 2 * radius / 31 - 1.0) < 1e-5                      # normalised like ReconstructionFilter::configure
    assert sorted({r for _, r in FR.FILTERS.values()}) == [1, 2, 3, 4, 5, 6]
    assert min(FR.filter_named("mitchell")[1]) < 0 and min(FR.filter_named("catmullrom")[1]) < 0 and min(FR.filter_named("lanczos3")[1]) < 0
    assert FR.border_of(0.5) == 0 and FR.border_of(2.49) == 2 and FR.border_of(2.5) == 2 and FR.border_of(4.5) == 4 and FR.border_of(6.0) == 6

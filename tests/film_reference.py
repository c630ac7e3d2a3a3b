"""The film in float64: a numpy restatement of ImageBlock::put (the oracle's ImageBlock::put and render loop, oracle/o_render.h) that
every film kernel of mitsuba_amd/csrc/k_film.h is held to per pixel (tests/test_gpu_film.py), pinned to the oracle first (tests/test_film_reference.py).

A sample taken in crop pixel (sx, sy) belongs to the render block whose origin (offX, offY) is the pixel rounded down to the block size; the block's
bitmap is the block (clipped to the crop window) plus `border` pixels on every side.  Everything that DECIDES something -- the sample's position in
the bitmap, its footprint, the index into the 32-entry table -- is float32, operation by operation as the kernels and the oracle state it (the table
look-up is discontinuous: a position rounded otherwise is another weight):

    px   = float32(sx) + jit                       pos = px - 0.5f - float32(off - border)
    min  = max(ceil(pos - radius), 0)              max = min(floor(pos + radius), bitmap size - 1)
    w(b) = table[min(int(|(float32(b) - pos) * scaleFactor|), 31)],  scaleFactor = 31 / radius,  border = ceil(radius - 0.5)
    w    = float32(wx * wy)

Everything that is SUMMED is float64: per film pixel and channel (R, G, B, alpha, weight) S = sum of w * v, A = sum of |w * v| and N = the number of
terms.  A float32 film of the same terms, added in any order, with or without fused multiply-adds, lies within (N + extra) * 2^-24 * A of S
(`film_bound`).  A sample of which R, G, B or alpha is not finite or negative is rejected as a whole (put returns false) and counted."""
import collections
import functools

import numpy as np

F32 = np.float32
RES = 31                # PHIP_FILTER_RESOLUTION: table[0..30] hold the filter, table[31] = 0

FilmSums = collections.namedtuple("FilmSums", "S A N rejected")


def border_of(radius):
    return int(np.ceil(F32(radius) - F32(0.5)))


def reach_of(radius):
    """pixels a sample can reach beyond its own: what host_render.h's filmPass selects the kernel by"""
    return int(np.floor(F32(radius) + F32(0.5)))


def film_sums(samples, jitter, radius, table, block_size, blocks=None):
    """samples [H, W, spp, 4] float32 (R, G, B, alpha); jitter [H, W, spp, 2] float32: the position of each sample inside its pixel, [0, 1)^2;
    (H, W) is the crop window, which is all the film the blocks know; radius, table[32]: the film's filter; blocks: None, or a boolean
    [tilesY, tilesX] array -- only samples of those render blocks are put (a shard).
    Returns FilmSums(S [H, W, 5] float64, A [H, W, 5] float64, N [H, W] int64, rejected)."""
    samples = np.asarray(samples, F32); jitter = np.asarray(jitter, F32)
    H, W, spp, _ = samples.shape
    assert jitter.shape == (H, W, spp, 2) and len(table) == RES + 1
    radius = F32(radius); table = np.asarray(table, F32); bs = int(block_size)
    scale = F32(RES) / radius
    border = border_of(radius)
    sy, sx, _ = np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij")
    sx, sy = sx.ravel(), sy.ravel()
    v = samples.reshape(-1, 4); jit = jitter.reshape(-1, 2)
    if blocks is not None:
        blocks = np.asarray(blocks, bool)
        assert blocks.shape == (-(-H // bs), -(-W // bs))
        own = blocks[sy // bs, sx // bs]
        sx, sy, v, jit = sx[own], sy[own], v[own], jit[own]
    bad = (~np.isfinite(v)).any(axis=1) | (v < 0).any(axis=1)
    rejected = int(bad.sum())
    sx, sy, v, jit = sx[~bad], sy[~bad], v[~bad], jit[~bad]
    v5 = np.concatenate([v.astype(np.float64), np.ones((len(v), 1))], axis=1)       # (R, G, B, alpha, 1)

    def axis(s, j, size):
        """per sample: the first bitmap column of the unclipped footprint, that column's film coordinate, and the weights of the columns behind it
        (NaN outside the clipped footprint)"""
        off = (s // bs) * bs
        extent = np.minimum(bs, size - off) + 2 * border
        p = s.astype(F32) + j
        pos = p - F32(0.5) - (off - border).astype(F32)
        umin = np.ceil(pos - radius).astype(np.int64)
        lo, hi = np.maximum(umin, 0), np.minimum(np.floor(pos + radius).astype(np.int64), extent - 1)
        n = int(np.ceil(2 * float(radius))) + 1                                     # floor(p + r) - ceil(p - r) + 1 <= 2 r + 1
        assert (hi - umin < n).all()
        w = np.full((n, len(s)), np.nan, F32)
        for i in range(n):
            b = umin + i
            idx = np.minimum(np.abs((b.astype(F32) - pos) * scale).astype(np.int64), RES)
            w[i] = np.where((b >= lo) & (b <= hi), table[idx], F32(np.nan))
        return umin + off - border, w

    x0, wx = axis(sx, jit[:, 0], W)
    y0, wy = axis(sy, jit[:, 1], H)
    S = np.zeros((H * W, 5)); A = np.zeros((H * W, 5)); N = np.zeros(H * W, np.int64)
    for iy in range(len(wy)):
        for ix in range(len(wx)):
            w = wx[ix] * wy[iy]                                                     # one float32 product
            X, Y = x0 + ix, y0 + iy
            m = ~np.isnan(w) & (X >= 0) & (X < W) & (Y >= 0) & (Y < H)              # (the merge of a block into the film clips its border)
            if not m.any():
                continue
            cell = (Y[m] * W + X[m]).astype(np.int64)
            term = w[m].astype(np.float64)[:, None] * v5[m]
            N += np.bincount(cell, minlength=H * W)
            for c in range(5):
                S[:, c] += np.bincount(cell, weights=term[:, c], minlength=H * W)
                A[:, c] += np.bincount(cell, weights=np.abs(term[:, c]), minlength=H * W)
    return FilmSums(S.reshape(H, W, 5), A.reshape(H, W, 5), N.reshape(H, W), rejected)


def add_sums(a, b):
    """the sums of two disjoint sets of samples (two calls, the shards of a frame)"""
    return FilmSums(a.S + b.S, a.A + b.A, a.N + b.N, a.rejected + b.rejected)


def film_bound(ref, extra=16, factor=1.0):
    """The standard forward error bound of a float32 sum of N products, any order: every product rounds once (or not at all under a fused multiply-add)
    and every addition once, so the computed sum is sum of t_i * (1 + d_i) with |d_i| <= (1 + u)^N - 1, u = 2^-24: at most N * u * A to first order, and the
    `extra` additions (the at most nine patch images of the merge, the passes of a call, the calls of a frame, the shards of a film) pay for the second."""
    return factor * (ref.N[..., None] + extra) * 2.0 ** -24 * ref.A


def check_film(film, ref, what="", extra=16, factor=1.0):
    """asserts |film - S| <= (N + extra) * 2^-24 * A at every pixel and channel, and film == 0 exactly where A == 0"""
    film = np.asarray(film)
    assert film.dtype == np.float32 and film.shape == ref.S.shape, (film.dtype, film.shape)
    err = np.abs(film.astype(np.float64) - ref.S)
    bound = film_bound(ref, extra, factor)
    over = ~(err <= bound)                                                          # (a NaN in the film is over the bound)
    empty = ref.A == 0
    dirty = empty & (film != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, 0.0))) if bound.size else 0.0
    print("%s: %d pixels x 5, N up to %d, worst |film - S| / bound = %.3f" % (what, film.shape[0] * film.shape[1], int(ref.N.max()), worst))
    if over.any() or dirty.any():
        lines = []
        for y, x, c in np.argwhere(over | dirty)[:12]:
            lines.append("  pixel (%d, %d) channel %d: film %.9g, S %.17g, |diff| %.3g, bound %.3g (N %d)"
                         % (x, y, c, film[y, x, c], ref.S[y, x, c], err[y, x, c], bound[y, x, c], ref.N[y, x]))
        raise AssertionError("%s: %d entries over the bound, %d not zero where nothing lands; relative to the sum the largest error is %.3g\n%s"
                             % (what, int(over.sum()), int(dirty.sum()),
                                float(np.max(err[over | dirty] / np.maximum(np.abs(ref.S[over | dirty]), 1e-300))), "\n".join(lines)))
    return worst


# ---- positions of the counter stream -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ctr_jitter(width, height, first, count, seed):
    from mitsuba_amd import _ffi
    import ctypes as C
    twin = _ffi.lib().phip_debug_host_ctr_block
    out = np.zeros((height, width, count, 4), F32)
    buf = (C.c_float * 4)()
    for y in range(height):
        for x in range(width):
            pixel = y * width + x                                                   # crop coordinates: the blocks start at the crop window's origin
            for k in range(count):
                twin(pixel, first + k, 0, seed, buf)
                out[y, x, k] = buf[:]
    out = np.ascontiguousarray(out[..., :2])
    out.setflags(write=False)
    return out


def ctr_jitter(width, height, spp, seed=0, sample_offset=0):
    """[height, width, spp, 2]: the camera sample of PHIP_SAMPLER_CTR -- the first two values of block 0 of the stream of (pixel, global sample index), from
    the host twin of the device's generator (phip_debug_host_ctr_block)"""
    return _ctr_jitter(int(width), int(height), int(sample_offset), int(spp), int(seed))


# ---- render blocks of a shard ------------------------------------------------------------------------------------------------------------------

def spiral_blocks(width, height, block_size):
    """(tx, ty) of the render blocks in the order they are handed out: a spiral from the centre block, first to the right, then down (o_render.h's
    spiralBlocks / host_render.h's shardTiles)"""
    nbx, nby = -(-width // block_size), -(-height // block_size)
    out = []
    cx, cy, direction, steps_left, num_steps = nbx // 2, nby // 2, 0, 1, 1
    while True:
        out.append((cx, cy))
        if len(out) == nbx * nby:
            return out
        while True:
            cx, cy = cx + (1, 0, -1, 0)[direction], cy + (0, 1, 0, -1)[direction]
            steps_left -= 1
            if steps_left == 0:
                direction = (direction + 1) % 4
                if direction in (0, 2):
                    num_steps += 1
                steps_left = num_steps
            if 0 <= cx < nbx and 0 <= cy < nby:
                break


def shard_blocks(width, height, block_size, shard_index, shard_count):
    """boolean [tilesY, tilesX]: the blocks whose index in the spiral is congruent to shard_index modulo shard_count"""
    nbx, nby = -(-width // block_size), -(-height // block_size)
    m = np.zeros((nby, nbx), bool)
    for i, (tx, ty) in enumerate(spiral_blocks(width, height, block_size)):
        m[ty, tx] = i % shard_count == shard_index
    return m


# ---- filter tables ---------------------------------------------------------------------------------------------------------------------------------

def filter_table(f, radius):
    """(radius, table[32]) of the filter f(x), x >= 0, discretised and normalised as ReconstructionFilter::configure does it (o_render.h's
    gaussianFilterTable): table[i] = f(radius * i / 31) for i < 31, table[31] = 0, scaled so that the table integrates to one over [-radius, radius]"""
    x = radius * np.arange(RES) / RES
    t = np.array([f(float(xi)) for xi in x], np.float64)
    t /= t.sum() * 2.0 * radius / RES
    return float(F32(radius)), [float(F32(a)) for a in t] + [0.0]


def _cubic(B, C):
    def f(x):                       # Mitchell & Netravali 1988, support [-2, 2]
        if x < 1:
            return ((12 - 9 * B - 6 * C) * x ** 3 + (-18 + 12 * B + 6 * C) * x ** 2 + (6 - 2 * B)) / 6
        if x < 2:
            return ((-B - 6 * C) * x ** 3 + (6 * B + 30 * C) * x ** 2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6
        return 0.0
    return f


def _sinc(x):
    return 1.0 if x == 0 else float(np.sin(np.pi * x) / (np.pi * x))


def box():
    return filter_table(lambda x: 1.0, 0.5)


def tent():
    return filter_table(lambda x: max(0.0, 1.0 - x), 1.0)


def gaussian(radius):
    """the reference's gaussian of standard deviation radius / 4, cut off (and lowered to zero) at `radius`: sigma 0.5 is its default filter; any other
    radius is that table stretched"""
    s = radius / 4.0
    return filter_table(lambda x: max(0.0, float(np.exp(-x * x / (2 * s * s)) - np.exp(-radius * radius / (2 * s * s)))), radius)


def mitchell():
    return filter_table(_cubic(1 / 3, 1 / 3), 2.0)


def catmullrom():
    return filter_table(_cubic(0.0, 0.5), 2.0)


def lanczos(lobes=3):
    return filter_table(lambda x: _sinc(x) * _sinc(x / lobes) if x < lobes else 0.0, float(lobes))


# name -> (builder, the reach the table is meant to have: floor(radius + 0.5)); mitchell, catmullrom and lanczos3 have negative lobes (A > |S|)
FILTERS = {
    "box": (box, 1), "tent": (tent, 1), "gauss_r1": (lambda: gaussian(1.0), 1),
    "gauss_r2": (lambda: gaussian(2.0), 2), "mitchell": (mitchell, 2), "catmullrom": (catmullrom, 2), "gauss_r2.49": (lambda: gaussian(2.49), 2),
    "gauss_r2.5": (lambda: gaussian(2.5), 3), "lanczos3": (lanczos, 3),
    "gauss_r4": (lambda: gaussian(4.0), 4), "gauss_r4.49": (lambda: gaussian(4.49), 4),
    "gauss_r4.5": (lambda: gaussian(4.5), 5), "gauss_r6": (lambda: gaussian(6.0), 6),
}


@functools.lru_cache(maxsize=None)
def filter_named(name):
    return FILTERS[name][0]()

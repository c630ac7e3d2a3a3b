"""The MIP pyramid of the reference's TMIPMap restated in numpy float32, one IEEE operation per line: the arbiter of phip_mip_pyramid between the committed fixtures
(tests/golden/ref_renders.npz, mip/*) and the sizes they do not cover.  mipmap.h:181-270 (sizes, clampNegative, the chain), bitmap.cpp:2230-2329 (X into a
temporary, then Y; equal sizes skip the pass), rfilter.h:123-198 (the weights), 232-330 (resampleAndClamp), 437-458 (the boundary look-up), lanczos.cpp:43-55.
sin is the float32 rounding of float64 sin."""
import numpy as np

F = np.float32
CLAMP, REPEAT, MIRROR, ZERO, ONE = range(5)
WRAP = {"clamp": CLAMP, "repeat": REPEAT, "mirror": MIRROR, "zero": ZERO, "one": ONE}


def sizes(w, h):
    out = [(h, w)]
    while w > 1 or h > 1:
        w, h = max(1, (w + 1) // 2), max(1, (h + 1) // 2)
        out.append((h, w))
    return out


def _sin(x):
    return F(np.sin(np.float64(x)))


def lanczos2(x):
    x = F(abs(x))
    if x < F(1e-4):
        return F(1.0)
    if x > F(2.0):
        return F(0.0)
    x1 = F(F(np.pi) * x)
    x2 = F(x1 / F(2.0))
    num = F(_sin(x1) * _sin(x2))
    den = F(x1 * x2)
    return F(num / den)


def weights(s, t):
    """(start[t], w[t, taps]) of a pass from s to t < s samples"""
    scale = F(F(s) / F(t))
    inv = F(F(1.0) / scale)
    radius = F(F(2.0) * scale)
    taps = int(np.ceil(F(radius * F(2.0))))
    start = np.zeros(t, np.int64)
    w = np.zeros((t, taps), F)
    for i in range(t):
        center = F(F(F(F(i) + F(0.5)) / F(t)) * F(s))
        start[i] = int(np.floor(F(F(center - radius) + F(0.5))))
        total = F(0.0)
        for j in range(taps):
            pos = F(F(F(start[i] + j) + F(0.5)) - center)
            w[i, j] = lanczos2(F(pos * inv))
            total = F(total + w[i, j])
        norm = F(F(1.0) / total)
        for j in range(taps):
            w[i, j] = F(w[i, j] * norm)
    return start, w


def _lookup(line, pos, wrap):
    """line: (n, ...) samples along the axis; the sample at `pos` under the boundary condition"""
    n = line.shape[0]
    if 0 <= pos < n:
        return line[pos]
    if wrap == CLAMP:
        return line[min(max(pos, 0), n - 1)]
    if wrap == REPEAT:
        return line[pos % n]
    if wrap == MIRROR:
        r = pos % (2 * n)
        return line[2 * n - r - 1 if r >= n else r]
    return np.full(line.shape[1:], 0.0 if wrap == ZERO else 1.0, F)


def resample_axis0(a, t, wrap, maxv):
    """a: (s, m, 3) float32, resampled along axis 0 to t samples, clamped to [0, maxv]"""
    s = a.shape[0]
    start, w = weights(s, t)
    out = np.zeros((t,) + a.shape[1:], F)
    for i in range(t):
        r = np.zeros(a.shape[1:], F)
        for j in range(w.shape[1]):
            r = (r + (_lookup(a, int(start[i]) + j, wrap) * w[i, j]).astype(F)).astype(F)
        lo = np.where(F(0.0) < r, r, F(0.0)).astype(F)                  # std::max(min, r)
        out[i] = np.where(lo < F(maxv), lo, F(maxv))                    # std::min(max, .)
    return out


def to_half_and_back(a):
    with np.errstate(over="ignore"):
        return a.astype(np.float16).astype(F)


def pyramid(level0, wrap_u, wrap_v, max_value):
    """every level as delivered (half rounded, widened), level 0 first"""
    wu, wv = WRAP.get(wrap_u, wrap_u), WRAP.get(wrap_v, wrap_v)
    cur = np.ascontiguousarray(level0, F)
    cur = np.where(F(0.0) < cur, cur, F(0.0)).astype(F)                 # clampNegative
    out = [to_half_and_back(cur)]
    h, w = cur.shape[:2]
    while w > 1 or h > 1:
        tw, th = max(1, (w + 1) // 2), max(1, (h + 1) // 2)
        if tw != w:
            cur = np.ascontiguousarray(resample_axis0(np.ascontiguousarray(cur.transpose(1, 0, 2)), tw, wu, max_value).transpose(1, 0, 2))
        if th != h:
            cur = resample_axis0(cur, th, wv, max_value)
        out.append(to_half_and_back(cur))
        w, h = tw, th
    return out

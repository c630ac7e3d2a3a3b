/*
 * pyramid_hd.h -- the MIP pyramid of the reference's TMIPMap (mipmap.h:181-270), stated once as __host__ __device__ functions: the kernels of
 * phip_mip_pyramid_device (k_pyramid.h) and the host call phip_mip_pyramid (host_pyramid.h) both run these and nothing else.  What is restated:
 *   sizes      n -> max(1, (n + 1) / 2) per axis until 1 x 1 (mipmap.h:182-192)
 *   level 0    negative channels are set to 0 (clampNegative, mipmap.h:236-243); the chain starts from that float32 image
 *   one step   Bitmap::resample (bitmap.cpp:2230-2329) with the 2-lobe Lanczos filter (lanczos.cpp:43-55): X into a temporary of target width x source height,
 *              then Y; a pass whose sizes are equal is skipped.  The weights of a pass are Resampler's (rfilter.h:123-198), an output texel is
 *              resampleAndClamp's (rfilter.h:232-330): r = 0; r += lookup * w in tap order, then std::min(max, std::max(0, r)) -- after EACH pass
 *   lookup     outside the source: the axis's boundary condition (rfilter.h:437-458)
 *   delivery   every level is stored in half precision (nearest-even, overflow to infinity, subnormals kept) and handed out widened to float
 * All float32, one IEEE operation per statement, -ffp-contract=off on both sides; sin is pm_sincosf (phip_fmath.h).  The bits are the reference's.
 */
#pragma once
#include <cstdint>
#include "dv_math.h"
#include "../../include/phip.h"

namespace pt {
namespace detail {

#define PHD __host__ __device__ inline

#define PYR_MAX_TAPS 8          /* taps = ceil(2 * 2 * s / t) and s / t <= 2 */

PHD int pyramidNextSize(int n) { return (n + 1) / 2 > 1 ? (n + 1) / 2 : 1; }
PHD int pyramidLevelCount(int w, int h) {
    int n = 1;
    while (w > 1 || h > 1) { w = pyramidNextSize(w); h = pyramidNextSize(h); ++n; }
    return n;
}

/* std::max(0.0f, v) and std::min(maxv, v) as libstdc++ spells them: a NaN becomes 0 */
PHD float pyramidClampLow(float v) { return (0.0f < v) ? v : 0.0f; }
PHD float pyramidClamp(float v, float maxv) { const float lo = (0.0f < v) ? v : 0.0f; return (lo < maxv) ? lo : maxv; }

/* float -> IEEE half (round to nearest even, overflow to infinity, subnormals kept) -> float, in integer and exact float operations */
PHD float pyramidHalfRound(float f) {
    const uint32_t u = pm_to_bits(f), sign = u & 0x80000000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return f;                                           /* infinity (NaN: as it is) */
    if (a >= 0x477ff000u) return pm_from_bits(sign | 0x7f800000u);            /* >= 65520: above half's largest finite value after rounding */
    if (a >= 0x38800000u) {                                                   /* a normal half: 10 mantissa bits */
        const uint32_t r = (a + 0xfffu + ((a >> 13) & 1u)) & ~0x1fffu;
        return pm_from_bits(sign | r);
    }
    const float m = pm_from_bits(a);                                          /* below 2^-14: a multiple of 2^-24 -- the spacing of floats in [0.5, 1) */
    const float t = m + 0.5f;
    const float r = t - 0.5f;
    return pm_from_bits(sign | pm_to_bits(r));
}

/* LanczosSincFilter::eval with two lobes */
PHD float pyramidLanczos2(float x) {
    x = fabsf(x);
    if (x < 1e-4f) return 1.0f;
    if (x > 2.0f) return 0.0f;
    const float x1 = PT_PI * x;
    const float x2 = x1 / 2.0f;
    float s1, s2, c;
    pm_sincosf(x1, &s1, &c);
    pm_sincosf(x2, &s2, &c);
    const float num = s1 * s2;
    const float den = x1 * x2;
    return num / den;
}

/* the weights of output index i of a pass from s to t < s samples: the first source index that contributes, the number of taps, the normalised weights */
struct PassWeights { int start, taps; float w[PYR_MAX_TAPS]; };
PHD PassWeights pyramidPassWeights(int s, int t, int i) {
    PassWeights P;
    const float scale = (float) s / (float) t;
    const float inv = 1.0f / scale;
    const float radius = 2.0f * scale;
    P.taps = (int) ceilf(radius * 2.0f);
    const float center = (i + 0.5f) / t * s;
    P.start = (int) floorf(center - radius + 0.5f);
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < PYR_MAX_TAPS; ++j) {
        P.w[j] = 0.0f;
        if (j < P.taps) {
            const float pos = (P.start + j) + 0.5f - center;
            P.w[j] = pyramidLanczos2(pos * inv);
            sum += P.w[j];
        }
    }
    const float norm = 1.0f / sum;
#pragma unroll
    for (int j = 0; j < PYR_MAX_TAPS; ++j) P.w[j] = P.w[j] * norm;
    return P;
}

/* Resampler::lookup: the sample index that position `pos` of an axis of n samples reads, -1 for a constant 0 and -2 for a constant 1 */
PHD int pyramidLookup(int pos, int n, uint32_t wrap) {
    if (pos >= 0 && pos < n) return pos;
    switch (wrap) {
        case PHIP_WRAP_CLAMP: return pos < 0 ? 0 : n - 1;
        case PHIP_WRAP_REPEAT: { const int r = pos % n; return r < 0 ? r + n : r; }
        case PHIP_WRAP_MIRROR: { int r = pos % (2 * n); if (r < 0) r += 2 * n; return r >= n ? 2 * n - r - 1 : r; }
        case PHIP_WRAP_ZERO: return -1;
        default: return -2;
    }
}

/* one RGB output texel of a pass: `line` is the first sample of the source row (X pass, stride 3) or column (Y pass, stride 3 * width), n the source size of the axis */
PHD void pyramidPassTexel(const float *line, size_t stride, int n, uint32_t wrap, const PassWeights &P, float maxv, float out[3]) {
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
#pragma unroll
    for (int j = 0; j < PYR_MAX_TAPS; ++j) {
        if (j < P.taps) {
            const int p = pyramidLookup(P.start + j, n, wrap);
            const float k = p == -1 ? 0.0f : 1.0f;
            const float *s = line + stride * (size_t) (p < 0 ? 0 : p);
            const float v0 = p < 0 ? k : s[0], v1 = p < 0 ? k : s[1], v2 = p < 0 ? k : s[2];
            r0 += v0 * P.w[j];
            r1 += v1 * P.w[j];
            r2 += v2 * P.w[j];
        }
    }
    out[0] = pyramidClamp(r0, maxv); out[1] = pyramidClamp(r1, maxv); out[2] = pyramidClamp(r2, maxv);
}

/* The tail of a pyramid in one block's LDS: the float32 level, the X-pass temporary and the next level side by side.  64 KiB of the CU's 160 KiB: static LDS
   that needs no attribute call, and a source of at most ~3100 texels -- beyond that one block's 1024 lanes are slower than the grid-wide pass kernels are. */
#define PYR_TAIL_LDS_BYTES 65536
#define PYR_TAIL_FLOATS (PYR_TAIL_LDS_BYTES / 4)
PHD size_t pyramidTailFloats(int w, int h) {
    const size_t tw = (size_t) pyramidNextSize(w), th = (size_t) pyramidNextSize(h);
    return 3 * ((size_t) w * h + tw * h + tw * th);
}
PHD bool pyramidTailFits(int w, int h) { return pyramidTailFloats(w, h) <= (size_t) PYR_TAIL_FLOATS; }

} // namespace detail
} // namespace pt

/* launch shapes of k_pyramid.h, and the caller's level pointers as the tail kernel takes them */
#define PYR_BLOCK 256
#define PYR_TAIL_THREADS 1024
struct PyramidOuts { float *level[PHIP_MIP_MAX_LEVELS]; };

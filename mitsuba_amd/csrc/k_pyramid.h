/*
 * k_pyramid.h -- the kernels of phip_mip_pyramid_device: a MIP pyramid as the reference's TMIPMap builds it, from a level 0 in device memory.  The arithmetic is
 * pyramid_hd.h's, which the host call phip_mip_pyramid runs too; these kernels only say which lane computes which texel.  No float atomics.
 * In launch order (host_pyramid.h):
 *   k_pyramid_level0   one lane per texel of level 0: negative channels to 0 into the float32 chain, its half rounding into the caller's level 0 (where asked for)
 *   k_pyramid_pass     one lane per output texel of one pass (axis 0: X, into the temporary; axis 1: Y): the lane's own <= 8 weights, three channels, the clamp;
 *                      float32 into the chain, and the half rounding into the caller's level when the pass completes one
 *   k_pyramid_tail     ONE block, once the float32 level fits its LDS (pyramidTailFits) with the temporary and the next level beside it: every remaining level
 *                      is made there, X pass, barrier, Y pass, barrier, and only the rounded levels leave the CU
 * Every lane computes its own weights: two pm_sincosf per tap, ~1500 FP64 operations per texel; a per-pass table would add a launch per pass to a call that is
 * launch-bound at its small end.  At 2048 x 1024 the weights are what the wide steps cost (DESIGN.md 3.20 has the measurement and names the table as the remedy).
 */
#pragma once
#include "pyramid_hd.h"

__global__ __launch_bounds__(PYR_BLOCK) void k_pyramid_level0(const float *src, size_t nTexels, float *chain, float *out) {
    const size_t i = (size_t) blockIdx.x * PYR_BLOCK + threadIdx.x;
    if (i >= nTexels) return;
    const float v0 = pt::detail::pyramidClampLow(src[3 * i]), v1 = pt::detail::pyramidClampLow(src[3 * i + 1]), v2 = pt::detail::pyramidClampLow(src[3 * i + 2]);
    chain[3 * i] = v0; chain[3 * i + 1] = v1; chain[3 * i + 2] = v2;
    if (out) { out[3 * i] = pt::detail::pyramidHalfRound(v0); out[3 * i + 1] = pt::detail::pyramidHalfRound(v1); out[3 * i + 2] = pt::detail::pyramidHalfRound(v2); }
}

/* source sw x sh; axis 0: target next(sw) x sh, axis 1: target sw x next(sh) */
__global__ __launch_bounds__(PYR_BLOCK) void k_pyramid_pass(const float *src, int sw, int sh, float *dst, float *rounded, int axis, uint32_t wrap, float maxv) {
    using namespace pt::detail;
    const int tw = axis == 0 ? pyramidNextSize(sw) : sw, th = axis == 0 ? sh : pyramidNextSize(sh);
    const size_t idx = (size_t) blockIdx.x * PYR_BLOCK + threadIdx.x;
    if (idx >= (size_t) tw * th) return;
    const int x = (int) (idx % (size_t) tw), y = (int) (idx / (size_t) tw);
    float out[3];
    if (axis == 0) pyramidPassTexel(src + 3 * (size_t) y * sw, 3, sw, wrap, pyramidPassWeights(sw, tw, x), maxv, out);
    else pyramidPassTexel(src + 3 * (size_t) x, 3 * (size_t) sw, sh, wrap, pyramidPassWeights(sh, th, y), maxv, out);
    dst[3 * idx] = out[0]; dst[3 * idx + 1] = out[1]; dst[3 * idx + 2] = out[2];
    if (rounded) { rounded[3 * idx] = pyramidHalfRound(out[0]); rounded[3 * idx + 1] = pyramidHalfRound(out[1]); rounded[3 * idx + 2] = pyramidHalfRound(out[2]); }
}

/* src: the float32 level `first` of w x h texels (pyramidTailFits(w, h)); levels first + 1 ... are written to outs.level[] */
__global__ __launch_bounds__(PYR_TAIL_THREADS) void k_pyramid_tail(const float *src, int w, int h, int first, PyramidOuts outs, uint32_t wrapU, uint32_t wrapV, float maxv) {
    using namespace pt::detail;
    __shared__ float lds[PYR_TAIL_FLOATS];
    /* three regions, fixed for the whole tail: level / temporary / next level of the first step; later steps are smaller and alternate between the outer two */
    float *cur = lds, *tmp = lds + 3 * (size_t) w * h, *nxt = tmp + 3 * (size_t) pyramidNextSize(w) * h;
    for (int i = threadIdx.x; i < 3 * w * h; i += PYR_TAIL_THREADS) cur[i] = src[i];
    __syncthreads();
    for (int l = first + 1; w > 1 || h > 1; ++l) {
        const int tw = pyramidNextSize(w), th = pyramidNextSize(h);
        float *rounded = outs.level[l];
        const float *from = cur;
        if (tw != w) {
            float *to = th == h ? nxt : tmp;
            for (int idx = threadIdx.x; idx < tw * h; idx += PYR_TAIL_THREADS) {
                const int x = idx % tw, y = idx / tw;
                float out[3];
                pyramidPassTexel(from + 3 * y * w, 3, w, wrapU, pyramidPassWeights(w, tw, x), maxv, out);
                to[3 * idx] = out[0]; to[3 * idx + 1] = out[1]; to[3 * idx + 2] = out[2];
                if (th == h) { rounded[3 * idx] = pyramidHalfRound(out[0]); rounded[3 * idx + 1] = pyramidHalfRound(out[1]); rounded[3 * idx + 2] = pyramidHalfRound(out[2]); }
            }
            __syncthreads();
            from = to;
        }
        if (th != h) {
            for (int idx = threadIdx.x; idx < tw * th; idx += PYR_TAIL_THREADS) {
                const int x = idx % tw, y = idx / tw;
                float out[3];
                pyramidPassTexel(from + 3 * x, 3 * (size_t) tw, h, wrapV, pyramidPassWeights(h, th, y), maxv, out);
                nxt[3 * idx] = out[0]; nxt[3 * idx + 1] = out[1]; nxt[3 * idx + 2] = out[2];
                rounded[3 * idx] = pyramidHalfRound(out[0]); rounded[3 * idx + 1] = pyramidHalfRound(out[1]); rounded[3 * idx + 2] = pyramidHalfRound(out[2]);
            }
            __syncthreads();
        }
        float *t = cur; cur = nxt; nxt = t;
        w = tw; h = th;
    }
}

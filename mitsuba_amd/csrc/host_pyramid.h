/*
 * host_pyramid.h -- host side of phip_mip_pyramid_device and of the host call phip_mip_pyramid: the MIP pyramid of the reference's TMIPMap from a level 0, on
 * the caller's device memory (the kernels: k_pyramid.h in phip_pyramid.hip) and on host memory.  Both run the statements of pyramid_hd.h; this header holds the
 * checks of the arguments (all of them before any write), the order of the passes and, on the device, the scratch: the float32 chain and the X-pass temporary
 * live in one grow-only buffer of the scene (SceneDev::pyramidScratch), allocated under the render lock.
 * PYRAMID_TAIL (a build-time constant, default 1): 1 = the levels after the first float32 level that fits one block's LDS come from k_pyramid_tail in one launch;
 * 0 = every step goes through k_pyramid_pass (the measurement of DESIGN.md 3.20, tools/gpu_pyramid.py).
 * Host code only; included by phip.hip alone, after host_boundary.h.  The caller of mipPyramidDevice holds the scene's render lock.
 */
#pragma once
#include "host_boundary.h"
#include "pyramid_hd.h"

#ifndef PYRAMID_TAIL
#define PYRAMID_TAIL 1
#endif

/* What the arguments say without a device: NULL, or the refusal (PHIP_ERR_INVALID, all of them) */
static const char *pyramidArgsError(bool haveScene, const phip_pyramid_desc *p) {
    if (!haveScene || !p) return "NULL argument";
    if (p->width == 0 || p->height == 0) return "width and height must not be 0";
    if (p->width > 0xFFFFu || p->height > 0xFFFFu) return "width and height must be smaller than 65536";
    if (p->n_levels != (uint32_t) detail::pyramidLevelCount((int) p->width, (int) p->height)) return "n_levels must be the complete pyramid down to 1x1";
    if (p->wrap_u > PHIP_WRAP_ONE || p->wrap_v > PHIP_WRAP_ONE) return "bad wrap mode";
    if (!(p->max_value > 0.0f)) return "max_value must be greater than 0";
    if (!p->d_level0) return "d_level0 must not be NULL";
    for (uint32_t l = 1; l < p->n_levels; ++l)
        if (!p->d_levels[l]) return "d_levels[l] must not be NULL for 1 <= l < n_levels";
    if (misaligned(p->d_level0, 4)) return "every pointer must be 4-byte aligned";
    for (uint32_t l = 0; l < p->n_levels; ++l)
        if (misaligned(p->d_levels[l], 4)) return "every pointer must be 4-byte aligned";
    /* the byte ranges of level 0 and of every output level: pairwise disjoint, but for d_levels[0] == d_level0 */
    struct Range { uintptr_t b, e; };
    Range r[PHIP_MIP_MAX_LEVELS + 1]; int n = 0;
    int w = (int) p->width, h = (int) p->height;
    r[n++] = { (uintptr_t) p->d_level0, (uintptr_t) p->d_level0 + (size_t) w * h * 3 * sizeof(float) };
    for (uint32_t l = 0; l < p->n_levels; ++l) {
        if (p->d_levels[l] && !(l == 0 && p->d_levels[0] == p->d_level0)) r[n++] = { (uintptr_t) p->d_levels[l], (uintptr_t) p->d_levels[l] + (size_t) w * h * 3 * sizeof(float) };
        w = detail::pyramidNextSize(w); h = detail::pyramidNextSize(h);
    }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (r[i].b < r[j].e && r[j].b < r[i].e) return "levels overlap: only d_levels[0] == d_level0 may";
    return nullptr;
}
static int pyramidDeviceRefusal(bool haveScene, const phip_pyramid_desc *p) { return refusal("phip_mip_pyramid_device", PHIP_ERR_INVALID, pyramidArgsError(haveScene, p)); }
static int pyramidHostRefusal(const phip_pyramid_desc *p) { return refusal("phip_mip_pyramid", PHIP_ERR_INVALID, pyramidArgsError(true, p)); }

static int mipPyramidDevice(phip_scene *sc, const phip_pyramid_desc *p) {
    SceneDev &sd = *sc->devs[0];
    if (!allOnSceneDevice(sd, { p->d_level0 }) || !allOnSceneDevice(sd, (const void *const *) p->d_levels, p->n_levels))
        return setErr(PHIP_ERR_INVALID, "phip_mip_pyramid_device: every pointer must be device memory of the scene's device");
    const int w0 = (int) p->width, h0 = (int) p->height, w1 = detail::pyramidNextSize(w0), h1 = detail::pyramidNextSize(h0);
    /* level l / the temporary / level l + 1 of the first step; later steps are smaller and alternate between the outer two */
    const size_t nCur = 3 * (size_t) w0 * h0, nTmp = 3 * (size_t) w1 * h0, nNxt = 3 * (size_t) w1 * h1;
    sd.pyramidScratch.alloc(nCur + nTmp + nNxt);
    float *cur = sd.pyramidScratch.p, *tmp = cur + nCur, *nxt = tmp + nTmp;
    const hipStream_t stream = sceneStream(sd, p->stream);
    const PyramidKernels K = phipPyramidKernels();
    hipLaunchKernelGGL(K.level0, dim3((unsigned) (((size_t) w0 * h0 + PYR_BLOCK - 1) / PYR_BLOCK)), dim3(PYR_BLOCK), 0, stream, p->d_level0, (size_t) w0 * h0, cur, p->d_levels[0]);
    int w = w0, h = h0;
    for (uint32_t l = 0; l + 1 < p->n_levels; ++l) {
        if (PYRAMID_TAIL && detail::pyramidTailFits(w, h)) {
            PyramidOuts outs; memcpy(outs.level, p->d_levels, sizeof(outs.level));
            hipLaunchKernelGGL(K.tail, dim3(1), dim3(PYR_TAIL_THREADS), 0, stream, (const float *) cur, w, h, (int) l, outs, p->wrap_u, p->wrap_v, p->max_value);
            break;
        }
        const int tw = detail::pyramidNextSize(w), th = detail::pyramidNextSize(h);
        const float *from = cur;
        if (tw != w) {
            float *to = th == h ? nxt : tmp;
            hipLaunchKernelGGL(K.pass, dim3((unsigned) (((size_t) tw * h + PYR_BLOCK - 1) / PYR_BLOCK)), dim3(PYR_BLOCK), 0, stream, from, w, h, to, th == h ? p->d_levels[l + 1] : (float *) nullptr,
                               0, p->wrap_u, p->max_value);
            from = to;
        }
        if (th != h)
            hipLaunchKernelGGL(K.pass, dim3((unsigned) (((size_t) tw * th + PYR_BLOCK - 1) / PYR_BLOCK)), dim3(PYR_BLOCK), 0, stream, from, tw, h, nxt, p->d_levels[l + 1], 1, p->wrap_v, p->max_value);
        std::swap(cur, nxt);
        w = tw; h = th;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PHIP_OK;
}

/* the kernels' twin on host memory: the same statements in the same order, the weights of a pass made once per output index */
static void mipPyramidHost(const phip_pyramid_desc *p) {
    int w = (int) p->width, h = (int) p->height;
    std::vector<float> cur(3 * (size_t) w * h), tmp, nxt;
    for (size_t i = 0; i < cur.size(); ++i) cur[i] = detail::pyramidClampLow(p->d_level0[i]);
    if (p->d_levels[0])
        for (size_t i = 0; i < cur.size(); ++i) p->d_levels[0][i] = detail::pyramidHalfRound(cur[i]);
    std::vector<detail::PassWeights> W;
    for (uint32_t l = 0; l + 1 < p->n_levels; ++l) {
        const int tw = detail::pyramidNextSize(w), th = detail::pyramidNextSize(h);
        const std::vector<float> *from = &cur;
        if (tw != w) {
            std::vector<float> &to = th == h ? nxt : tmp;
            to.resize(3 * (size_t) tw * h);
            W.resize(tw);
            for (int x = 0; x < tw; ++x) W[x] = detail::pyramidPassWeights(w, tw, x);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < tw; ++x)
                    detail::pyramidPassTexel(from->data() + 3 * (size_t) y * w, 3, w, p->wrap_u, W[x], p->max_value, to.data() + 3 * ((size_t) y * tw + x));
            from = &to;
        }
        if (th != h) {
            nxt.resize(3 * (size_t) tw * th);
            W.resize(th);
            for (int y = 0; y < th; ++y) W[y] = detail::pyramidPassWeights(h, th, y);
            for (int y = 0; y < th; ++y)
                for (int x = 0; x < tw; ++x)
                    detail::pyramidPassTexel(from->data() + 3 * (size_t) x, 3 * (size_t) tw, h, p->wrap_v, W[y], p->max_value, nxt.data() + 3 * ((size_t) y * tw + x));
        }
        for (size_t i = 0; i < nxt.size(); ++i) p->d_levels[l + 1][i] = detail::pyramidHalfRound(nxt[i]);
        cur.swap(nxt);
        w = tw; h = th;
    }
}

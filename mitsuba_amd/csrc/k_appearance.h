/*
 * k_appearance.h -- the kernels of phip_scene_update_appearance: what a material, a texture or the environment map says in the scene's device arrays, rewritten where
 * it is.  Plain one-lane-per-item passes around the __host__ __device__ bodies of appearance_hd.h; no LDS, no float atomics.  In launch order (host_appearance.h):
 *   k_appearance_texmax     the level-0 maximum of a caller's RGB texture: packTextures' comparison per texel, a wave reduction, one atomicMax per wave on the bit
 *                           pattern (every candidate is >= +0, so the unsigned order is the float order); the host reads it BEFORE anything is written
 *   k_appearance_texels     RGB float3 -> float4 (w = 0) into the scene's texel array; bitmap textures and the environment map's levels
 *   k_envmap_cdf_rows       one lane per row of the environment map: the conditional CDF, the row weight, the row's term of the marginal -- sequential along the row,
 *                           because the sum has to be the creation's (lanes read texels a row apart: an uncoalesced walk of a few milliseconds at 4096 x 2048, which
 *                           is what it replaces a scene creation with)
 *   k_envmap_cdf_marginal   one lane: the h + 1 marginal entries and their sum
 *   k_appearance_records    one lane per triangle: front / back leaf and the material's flag bits of its shading record from a per-shape table, its shade class into
 *                           a byte array (the one phip_scene_rebuild tags its next tree from)
 *   k_appearance_classes    one lane per Wald record: word 11 from the class of the record's primitive (a placeholder record, 0xFFFFFFFF: class 0 -- tagShadeClasses)
 */
#pragma once
#include "appearance_hd.h"

__global__ __launch_bounds__(APP_BLOCK) void k_appearance_texmax(const float *rgb, uint32_t n, uint32_t *out) {
    float m = 0.0f;
    for (uint32_t i = blockIdx.x * APP_BLOCK + threadIdx.x; i < n; i += gridDim.x * APP_BLOCK)
        m = pt::detail::texelMaxStep(m, rgb[3 * (size_t) i], rgb[3 * (size_t) i + 1], rgb[3 * (size_t) i + 2]);
    for (int off = 32; off > 0; off >>= 1) m = pt::detail::texelMaxMerge(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63u) == 0u) atomicMax(out, __float_as_uint(m));
}

__global__ __launch_bounds__(APP_BLOCK) void k_appearance_texels(const float *rgb, float4 *dst, uint32_t n) {
    const uint32_t i = blockIdx.x * APP_BLOCK + threadIdx.x;
    if (i >= n) return;
    dst[i] = make_float4(rgb[3 * (size_t) i], rgb[3 * (size_t) i + 1], rgb[3 * (size_t) i + 2], 0.0f);
}

__global__ __launch_bounds__(64) void k_envmap_cdf_rows(const float4 *texels, int w, int h, float *cdfCols, float *rowWeights, float *rowTerms) {
    const int y = (int) (blockIdx.x * 64u + threadIdx.x);
    if (y >= h) return;
    rowTerms[y] = pt::detail::envmapRowCdf(texels + (size_t) y * w, w, h, y, cdfCols + (size_t) y * (w + 1), rowWeights + y);
}

__global__ __launch_bounds__(64) void k_envmap_cdf_marginal(const float *rowTerms, int h, float *cdfRows, float *rowSum) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *rowSum = pt::detail::envmapMarginalCdf(rowTerms, h, cdfRows);
}

__global__ __launch_bounds__(APP_BLOCK) void k_appearance_records(float4 *triShade, uint32_t stride, uint32_t nTriangles, const uint32_t *triShape,
                                                                  const pt::detail::ShapeWords *shapeWords, uint8_t *triClass) {
    const uint32_t i = blockIdx.x * APP_BLOCK + threadIdx.x;
    if (i >= nTriangles) return;
    const pt::detail::ShapeWords s = shapeWords[triShape[i]];
    float *r = (float *) (triShade + (size_t) stride * i);
    r[3] = __uint_as_float(s.front);
    r[7] = __uint_as_float(s.back);
    r[15] = __uint_as_float((__float_as_uint(r[15]) & ~TS_MATERIAL_BITS) | s.flags);
    triClass[i] = (uint8_t) s.cls;
}

__global__ __launch_bounds__(APP_BLOCK) void k_appearance_classes(float4 *recs, const uint32_t *recPrim, uint32_t nRecs, const uint8_t *triClass, uint32_t nTriangles) {
    const uint32_t i = blockIdx.x * APP_BLOCK + threadIdx.x;
    if (i >= nRecs) return;
    const uint32_t prim = recPrim[i];
    ((float *) recs)[12 * (size_t) i + 11] = __uint_as_float(prim < nTriangles ? (uint32_t) triClass[prim] : 0u);
}

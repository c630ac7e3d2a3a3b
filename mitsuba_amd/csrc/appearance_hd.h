/*
 * appearance_hd.h -- the arithmetic the creation's host stages (host_scene.h: packTextures, buildEnvmap) and the kernels of phip_scene_update_appearance
 * (k_appearance.h) share, stated once as __host__ __device__ functions, as refit_hd.h does for the refit: the maximum of a texel, one row of the environment map's
 * conditional CDF with its weight, the marginal CDF.  Float addition is not associative and the call's contract is bit identity with a fresh creation, so the sums
 * run in EnvironmentMap::configure's order (envmap.cpp:262-328) on both sides: sequentially along a row, sequentially over the rows.  Everything is compiled with
 * -ffp-contract=off.
 */
#pragma once
#include <cstdint>
#include "dv_scene.h"

namespace pt {
namespace detail {

#define AHD __host__ __device__ inline

/* packTextures' running maximum of level 0: m = std::max(m, std::max(c0, std::max(c1, c2))) with std::max spelled out ((a < b) ? b : a) -- a NaN channel is
   ignored exactly as it is there.  m starts at 0, so the result is never below +0 and never NaN: the maximum of the per-texel candidates in any order */
AHD float texelMaxStep(float m, float c0, float c1, float c2) {
    const float i = (c1 < c2) ? c2 : c1;
    const float t = (c0 < i) ? i : c0;
    return (m < t) ? t : m;
}
AHD float texelMaxMerge(float m, float o) { return (m < o) ? o : m; }

/* row y of an environment map of w x h float4 texels: the w + 1 entries of its conditional CDF over luminance, its weight sin(theta), and the row's term of the
   marginal (returned): envmap.cpp:279-304 */
AHD float envmapRowCdf(const float4 *row, int w, int h, int y, float *cdfRow, float *rowWeight) {
    float colSum = 0;
    cdfRow[0] = 0;
    for (int x = 0; x < w; ++x) {
        const float4 t = row[x];
        colSum += rgbLuminance(V3(t.x, t.y, t.z));
        cdfRow[x + 1] = colSum;
    }
    const float norm = 1.0f / colSum;
    for (int x = 1; x < w; ++x) cdfRow[w - x] *= norm;
    cdfRow[w] = 1.0f;
    float sn, cs; pm_sincosf((y + 0.5f) * PT_PI / h, &sn, &cs);
    *rowWeight = sn;
    return colSum * sn;
}

/* the h + 1 entries of the marginal CDF from the rows' terms; returns their sum, which the caller checks (a black or non-finite map) and normalises by: envmap.cpp:305-317 */
AHD float envmapMarginalCdf(const float *rowTerms, int h, float *cdfRows) {
    float rowSum = 0.0f;
    cdfRows[0] = 0;
    for (int y = 0; y < h; ++y) { rowSum += rowTerms[y]; cdfRows[y + 1] = rowSum; }
    const float norm = 1.0f / rowSum;
    for (int y = 1; y < h; ++y) cdfRows[h - y] *= norm;
    cdfRows[h] = 1.0f;
    return rowSum;
}

#define APP_BLOCK 256
/* what a shape's material says in the shading records of its triangles, and their shade class */
struct ShapeWords { uint32_t front, back, flags, cls; };
#define TS_MATERIAL_BITS ((uint32_t) (TS_TWOSIDED | TS_MF_SMOOTH | TS_TRANS_OR_BACK))

} // namespace detail
} // namespace pt

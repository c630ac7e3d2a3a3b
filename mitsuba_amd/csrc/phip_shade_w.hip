/*
 * phip_shade_w.hip -- k_shade_trace_w<materials, strictNormals, features> (k_shade_trace_w.h): the one-kernel iterations of the scenes on the 8-wide tree in memory
 * that k_mega does not serve.  Compiled once per feature set (-DSHADE_FEAT=0..3, 8 and 11, as phip_shade.hip): six objects of four kernels each.  phip.hip asks for the
 * kernel's LDS plan and residency (phipShadeTraceWidePlan) and launches it (phipLaunchShadeTraceWide) through the entry points of the render's feature set.
 */
#include "phip_common.h"
#include "k_traverse.h"
#include "k_wide_node.h"
#include "k_wide_wave.h"
#include "k_shade.h"
#include "k_shade_trace.h"
#include "k_shade_trace_w.h"

#ifndef SHADE_FEAT
#error "compile with -DSHADE_FEAT=0..3, 8 or 11"
#endif
#define SHADE_CAT2(a, b) a##b
#define SHADE_CAT(a, b) SHADE_CAT2(a, b)

typedef void (*ShadeTraceWideKernel)(DevScene, PathPool, RenderConst, float4 *, uint32_t);

/* leaf BSDF models = diffuse only / all, as k_shade_trace (a scene with glass but no copper runs the kernel that also knows copper) */
static ShadeTraceWideKernel kernelOf(bool strictNormals, int materialMask) {
    static const ShadeTraceWideKernel table[2][2] = { { k_shade_trace_w<0, false, SHADE_FEAT>, k_shade_trace_w<MM_ALL, false, SHADE_FEAT> },
                                                      { k_shade_trace_w<0, true, SHADE_FEAT>, k_shade_trace_w<MM_ALL, true, SHADE_FEAT> } };
    return table[strictNormals ? 1 : 0][(materialMask & MM_ALL) ? 1 : 0];
}

/* the kernel's dynamic LDS with `nodeCache` staged nodes, and the blocks of it that the runtime finds resident on a compute unit (0: none) */
int SHADE_CAT(phipShadeTraceWidePlanF, SHADE_FEAT)(bool strictNormals, int materialMask, uint32_t nodeCache, size_t *ldsBytes) {
    const ShadeTraceWideKernel k = kernelOf(strictNormals, materialMask);
    *ldsBytes = shadeTraceWideLdsBytes(nodeCache, (materialMask & MM_ALL) != 0);
    int n = 0;
    if (*ldsBytes > 48 * 1024 && hipFuncSetAttribute((const void *) k, hipFuncAttributeMaxDynamicSharedMemorySize, (int) *ldsBytes) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *) k, BLOCK, *ldsBytes) != hipSuccess) return 0;
    return n;
}

void SHADE_CAT(phipLaunchShadeTraceWideF, SHADE_FEAT)(bool strictNormals, int materialMask, dim3 grid, size_t ldsBytes, hipStream_t stream,
                                                      const DevScene &S, const PathPool &P, const RenderConst &rc, float4 *L, uint32_t nodeCache) {
    hipLaunchKernelGGL(kernelOf(strictNormals, materialMask), grid, dim3(BLOCK), ldsBytes, stream, S, P, rc, L, nodeCache);
}

/*
 * phip_shade_w.hip -- k_shade_trace_w<materials, strictNormals, features> (k_shade_trace_w.h): the one-kernel iterations of the scenes on the 8-wide tree in memory
 * that k_mega does not serve.  Compiled once per feature set (-DSHADE_FEAT=0..3, 8 and 11, as phip_shade.hip): six objects of four kernels each, behind one look-up that
 * returns them (phip_common.h).  phip.hip prices the kernel's LDS (shadeTraceWideLdsBytes), asks the runtime for its residency and launches it.
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

/* leaf BSDF models = diffuse only / all, as k_shade_trace (a scene with glass but no copper runs the kernel that also knows copper) */
ShadeTraceWideKernel SHADE_CAT(phipShadeTraceWideKernelF, SHADE_FEAT)(bool strictNormals, int materialMask) {
    static const ShadeTraceWideKernel table[2][2] = { { k_shade_trace_w<0, false, SHADE_FEAT>, k_shade_trace_w<MM_ALL, false, SHADE_FEAT> },
                                                      { k_shade_trace_w<0, true, SHADE_FEAT>, k_shade_trace_w<MM_ALL, true, SHADE_FEAT> } };
    return table[strictNormals ? 1 : 0][(materialMask & MM_ALL) ? 1 : 0];
}

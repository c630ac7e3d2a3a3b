/*
 * phip_shade_r.hip -- the kernels of phip_radiance_device (k_shade_r.h): k_shade_r<materials, strictNormals, features>, the wavefront vertex kernel fed from a
 * caller's ray array, and k_radiance_out.  Compiled per feature set (-DSHADE_FEAT=0..3: bit 0 = environment emitter, bit 1 = bitmap textures; the entry point
 * serves the counter stream only, so there is no build with the QMC samplers) and per part (-DSHADE_PART=0 / 1: without / with strictNormals), eight objects, for
 * the reason phip_shade.hip is: the texture code is inlined into every kernel that can meet a textured leaf.  Every object exports one look-up that returns its
 * kernels (declared in phip_common.h); the object of feature set 0, part 0 also holds k_radiance_out.
 */
#include "phip_common.h"
#include "k_traverse.h"
#include "k_shade.h"
#if SHADE_FEAT == 0 && SHADE_PART == 0
#define SHADE_R_OUT_KERNEL
#endif
#include "k_shade_r.h"

#if !defined(SHADE_FEAT) || !defined(SHADE_PART) || SHADE_FEAT < 0 || SHADE_FEAT > 3 || SHADE_PART < 0 || SHADE_PART > 1
#error "compile with -DSHADE_FEAT=0..3 and -DSHADE_PART=0..1"
#endif
#define SHADE_CAT2(a, b) a##b
#define SHADE_CAT(a, b) SHADE_CAT2(a, b)
#define SHADE_STRICT (SHADE_PART == 1)

ShadeRaysKernel SHADE_CAT(SHADE_CAT(SHADE_CAT(phipShadeRaysKernelS, SHADE_PART), F), SHADE_FEAT)(int materialMask, int tables) {
#define SHADE_ROW(F_) { k_shade_r<0, SHADE_STRICT, F_>, k_shade_r<MM_ROUGH, SHADE_STRICT, F_>, k_shade_r<MM_DIELECTRIC, SHADE_STRICT, F_>, k_shade_r<MM_ALL, SHADE_STRICT, F_> }
    static const ShadeRaysKernel table[4] = SHADE_ROW(SHADE_FEAT);
#if SHADE_FEAT == 0
    /* the table sets of k_shade (phip_shade.hip): emitter table and materials addressed as LDS (1), the emitter table only (2) */
    static const ShadeRaysKernel tableLds[4] = SHADE_ROW(4), tableEmLds[4] = SHADE_ROW(16);
    if (tables == 1) return tableLds[materialMask & MM_ALL];
    if (tables == 2) return tableEmLds[materialMask & MM_ALL];
#endif
#undef SHADE_ROW
    (void) tables;
    return table[materialMask & MM_ALL];
}

#if SHADE_FEAT == 0 && SHADE_PART == 0
RadianceOutKernel phipRadianceOutKernel() { return k_radiance_out; }
#endif

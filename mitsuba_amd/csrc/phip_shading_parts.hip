/*
 * phip_shading_parts.hip -- the kernels of phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device (k_shading_parts.h: k_bsdf_parts per output
 * set, k_emitter_sample and k_emitter_eval without / with an environment emitter) behind the one look-up that returns them (phip_common.h).  One object; phip.hip
 * validates the arguments and launches them (host_shading_parts.h).
 */
#include "phip_common.h"
#include "k_shade.h"             /* (stageShadeTables: the emitter table in LDS; shadeVertex and k_shade are templates this unit does not instantiate) */
#define PHIP_SHADING_PARTS_KERNELS
#include "k_shading_parts.h"

ShadingPartsKernels phipShadingPartsKernels() {
    ShadingPartsKernels k;
    k.bsdf[0] = k_bsdf_parts<false, false>; k.bsdf[1] = k_bsdf_parts<true, false>; k.bsdf[2] = k_bsdf_parts<false, true>; k.bsdf[3] = k_bsdf_parts<true, true>;
    k.emitterSample[0] = k_emitter_sample<false>; k.emitterSample[1] = k_emitter_sample<true>;
    k.emitterEval[0] = k_emitter_eval<false>; k.emitterEval[1] = k_emitter_eval<true>;
    return k;
}

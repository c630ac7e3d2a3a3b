/*
 * host_shading_parts.h -- host side of phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device: what an integrator does between two ray casts, on
 * the caller's arrays in device memory (the kernels: k_shading_parts.h in phip_shading_parts.hip).  With phip_camera_rays_device, phip_trace_device and
 * phip_film_device these are the parts of a render the caller's own integrator is written over.
 * The calls take no render parameters: there is no sampler, no pass and no pool -- one launch of one lane per item, ordered after the caller's stream and complete on
 * return.  They allocate nothing.  Everything is validated before the launch, so a refused call has written nothing.
 * Host code only; included by phip.hip alone, after host_boundary.h.  The caller holds the scene's render lock.
 */
#pragma once
#include "host_boundary.h"

/* What the arguments say without a device (the debug library tests it on a machine without one): NULL, or the refusal.  Every refusal is PHIP_ERR_INVALID.
   n == 0 is served before any pointer is looked at. */

static const char *bsdfArgsError(bool haveScene, const phip_bsdf_desc *b) {
    if (!haveScene || !b) return "NULL argument";
    if (b->flags & ~PHIP_BSDF_LOCAL) return "unknown flag";
    if (b->n == 0) return nullptr;
    if (b->n > CALL_MAX_ITEMS) return "more than 2^32 - 256 items in one call";
    if (!b->d_rays || !b->d_hits) return "d_rays and d_hits must not be NULL";
    if (!b->d_eval && !b->d_sampled && !b->d_wi_local) return "no output: one of d_eval, d_sampled and d_wi_local must be set";
    if (b->d_eval && !b->d_wo) return "d_eval needs d_wo";
    if (b->d_sampled && !b->d_samples) return "d_sampled needs d_samples";
    if (misaligned(b->d_rays, 16) || misaligned(b->d_hits, 16) || misaligned(b->d_wo, 16) || misaligned(b->d_eval, 16) || misaligned(b->d_sampled, 16) ||
        misaligned(b->d_wi_local, 16)) return "d_rays, d_hits, d_wo, d_eval, d_sampled and d_wi_local must be 16-byte aligned";
    if (misaligned(b->d_samples, 8)) return "d_samples must be 8-byte aligned";
    return nullptr;
}

static const char *emitterSampleArgsError(bool haveScene, const phip_emitter_sample_desc *e) {
    if (!haveScene || !e) return "NULL argument";
    if (e->n == 0) return nullptr;
    if (e->n > CALL_MAX_ITEMS) return "more than 2^32 - 256 items in one call";
    if (!e->d_ref || !e->d_samples || !e->d_sampled) return "d_ref, d_samples and d_sampled must not be NULL";
    if (misaligned(e->d_ref, 16) || misaligned(e->d_ref_n, 16) || misaligned(e->d_sampled, 16) || misaligned(e->d_shadow_rays, 16))
        return "d_ref, d_ref_n, d_sampled and d_shadow_rays must be 16-byte aligned";
    if (misaligned(e->d_samples, 8)) return "d_samples must be 8-byte aligned";
    return nullptr;
}

static const char *emitterEvalArgsError(bool haveScene, const phip_emitter_eval_desc *e) {
    if (!haveScene || !e) return "NULL argument";
    if (e->n == 0) return nullptr;
    if (e->n > CALL_MAX_ITEMS) return "more than 2^32 - 256 items in one call";
    if (!e->d_rays || !e->d_hits || !e->d_eval) return "d_rays, d_hits and d_eval must not be NULL";
    if (misaligned(e->d_rays, 16) || misaligned(e->d_hits, 16) || misaligned(e->d_ref_n, 16) || misaligned(e->d_eval, 16) || misaligned(e->d_emitter, 16))
        return "d_rays, d_hits, d_ref_n, d_eval and d_emitter must be 16-byte aligned";
    return nullptr;
}

/* ... as the entry points and their test hooks return them */
static int bsdfRefusal(bool haveScene, const phip_bsdf_desc *b) { return refusal("phip_bsdf_device", PHIP_ERR_INVALID, bsdfArgsError(haveScene, b)); }
static int emitterSampleRefusal(bool haveScene, const phip_emitter_sample_desc *e) { return refusal("phip_emitter_sample_device", PHIP_ERR_INVALID, emitterSampleArgsError(haveScene, e)); }
static int emitterEvalRefusal(bool haveScene, const phip_emitter_eval_desc *e) { return refusal("phip_emitter_eval_device", PHIP_ERR_INVALID, emitterEvalArgsError(haveScene, e)); }

static int bsdfDevice(phip_scene *sc, const phip_bsdf_desc *b) {
    SceneDev &sd = *sc->devs[0];
    if (!allOnSceneDevice(sd, { b->d_rays, b->d_hits, b->d_wo, b->d_samples, b->d_eval, b->d_sampled, b->d_wi_local }))
        return setErr(PHIP_ERR_INVALID, "phip_bsdf_device: every pointer must be device memory of the scene's device");
    const hipStream_t stream = sceneStream(sd, b->stream);
    const ShadingPartsKernels K = phipShadingPartsKernels();
    hipLaunchKernelGGL(K.bsdf[(b->d_eval ? 1 : 0) | (b->d_sampled ? 2 : 0)], dim3(blocksFor(b->n)), dim3(BLOCK), 0, stream, sd.dev, (const float4 *) b->d_rays, (const float4 *) b->d_hits,
                       (const float4 *) b->d_wo, (const float2 *) b->d_samples, (uint32_t) b->n, (uint32_t) (b->flags & PHIP_BSDF_LOCAL), (float4 *) b->d_eval, (float4 *) b->d_sampled, (float4 *) b->d_wi_local);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PHIP_OK;
}

static int emitterSampleDevice(phip_scene *sc, const phip_emitter_sample_desc *e) {
    SceneDev &sd = *sc->devs[0];
    if (!allOnSceneDevice(sd, { e->d_ref, e->d_ref_n, e->d_samples, e->d_sampled, e->d_shadow_rays }))
        return setErr(PHIP_ERR_INVALID, "phip_emitter_sample_device: every pointer must be device memory of the scene's device");
    const hipStream_t stream = sceneStream(sd, e->stream);
    const ShadingPartsKernels K = phipShadingPartsKernels();
    hipLaunchKernelGGL(K.emitterSample[sd.dev.envEmitter >= 0 ? 1 : 0], dim3(blocksFor(e->n)), dim3(BLOCK), 0, stream, sd.dev, (const float4 *) e->d_ref, (const float4 *) e->d_ref_n,
                       (const float2 *) e->d_samples, (uint32_t) e->n, (float4 *) e->d_sampled, (float4 *) e->d_shadow_rays);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PHIP_OK;
}

static int emitterEvalDevice(phip_scene *sc, const phip_emitter_eval_desc *e) {
    SceneDev &sd = *sc->devs[0];
    if (!allOnSceneDevice(sd, { e->d_rays, e->d_hits, e->d_ref_n, e->d_eval, e->d_emitter }))
        return setErr(PHIP_ERR_INVALID, "phip_emitter_eval_device: every pointer must be device memory of the scene's device");
    const hipStream_t stream = sceneStream(sd, e->stream);
    const ShadingPartsKernels K = phipShadingPartsKernels();
    hipLaunchKernelGGL(K.emitterEval[sd.dev.envEmitter >= 0 ? 1 : 0], dim3(blocksFor(e->n)), dim3(BLOCK), 0, stream, sd.dev, (const float4 *) e->d_rays, (const float4 *) e->d_hits,
                       (const float4 *) e->d_ref_n, (uint32_t) e->n, (float4 *) e->d_eval, e->d_emitter);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PHIP_OK;
}

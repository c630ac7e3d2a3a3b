/*
 * host_radiance.h -- host side of phip_radiance_device: path-traced radiance along a caller's rays in device memory.  The call is a render job without a film: the
 * passes, the pool and the pass loop are host_render.h's (planPasses, setupWavefront, wavefrontPass, passResults) over n x sppPass sample ids, the vertex kernel is
 * k_shade_r (k_shade_r.h in phip_shade_r.hip: k_shade's block step fed from the ray array), the ray kernel is k_rays_w unchanged, and k_radiance_out stands where
 * the film pass stands.  There is no fused path: the call always runs what PHIP_FLAG_NO_FUSED runs.
 * Buffers: the pool, the per-sample buffer L and the statistics are the SceneDev's, shared with the renders (the render lock serialises the two).  A call whose spp
 * does not fit one pass (PHIP_MAX_PASS_SAMPLES, the 24 GiB budget of L, 32-bit sample ids) keeps its running float64 sums in SceneDev::radianceAcc, 32 bytes per
 * ray: the one buffer of this call that grows with n.
 * Host code only; included by phip.hip alone, after host_render.h.  The caller holds the scene's render lock.
 */
#pragma once
#include "host_render.h"

/* What the arguments say without a device (the debug library tests it on a machine without one): NULL, or the refusal and its code */
static const char *radianceArgsError(const phip_render_params *p, const phip_radiance_desc *r, int &code) {
    code = PHIP_ERR_INVALID;
    if (!p || !r) return "NULL argument";
    if (p->integrator > PHIP_INTEGRATOR_VOLPATH_SIMPLE) return "unknown integrator kind";
    if (p->sampler > PHIP_SAMPLER_HAMMERSLEY) return "unknown sampler kind";
    if (p->n_devices < 0 || p->n_devices > 1) return "one device: the rays and the result are device memory of the scene's device (n_devices must be 0 or 1)";
    if (p->flags & (PHIP_FLAG_SAMPLE_BUFFER | PHIP_FLAG_ACCUMULATE)) return "PHIP_FLAG_SAMPLE_BUFFER and PHIP_FLAG_ACCUMULATE concern the film: the call has none";
    if (r->n > CALL_MAX_ITEMS) return "more than 2^32 - 256 rays in one call";
    if (r->n) {
        if (!r->d_rays || !r->d_out) return "d_rays and d_out must not be NULL";
        if (misaligned(r->d_rays, 16) || misaligned(r->d_out, 16)) return "d_rays and d_out must be 16-byte aligned";
        if (misaligned(r->d_stream, 4)) return "d_stream must be 4-byte aligned";
    }
    if (r->stream_layout > PHIP_RADIANCE_STREAM_PAIRS) return "unknown stream_layout";
    if (r->stream_layout == PHIP_RADIANCE_STREAM_PAIRS) {
        if (p->sample_offset != 0) return "PHIP_RADIANCE_STREAM_PAIRS: the sample index is the pair's, sample_offset must be 0";
        if (r->n && !r->d_stream) return "PHIP_RADIANCE_STREAM_PAIRS: d_stream must not be NULL";
        if (r->n && misaligned(r->d_stream, 8)) return "PHIP_RADIANCE_STREAM_PAIRS: d_stream must be 8-byte aligned";
    }
    code = PHIP_ERR_UNSUPPORTED;
    if (p->integrator == PHIP_INTEGRATOR_DIRECT) return "PHIP_INTEGRATOR_DIRECT is not served: its sample arrays are addressed by film coordinates";
    if (p->sampler != PHIP_SAMPLER_CTR) return "PHIP_SAMPLER_CTR only: the other samplers' streams are addressed by film coordinates";
    code = PHIP_OK;
    return nullptr;
}
/* ... as the entry point and its test hook return it */
static int radianceRefusal(const phip_render_params *p, const phip_radiance_desc *r) {
    int code = PHIP_OK;
    const char *bad = radianceArgsError(p, r, code);
    return refusal("phip_radiance_device", code, bad);
}

/* k_shade_r for this scene's feature set, leaf BSDF models and table set, and k_radiance_out: resolved once per scene and strictNormals through shadeUnit */
static ShadeRaysKernel radianceVertexKernel(RenderJob &J) {
    SceneDev::RadiancePlan &R = J.sd.radiance;
    const int strict = J.p->strict_normals != 0 ? 1 : 0;
    if (!R.out) R.out = phipRadianceOutKernel();
    if (!R.vertex[strict]) R.vertex[strict] = shadeUnit(J.wf.feat).rays[strict](J.sc->materialMask, shadeTableSet(J.wf.feat, J.D));
    return R.vertex[strict];
}

static int radianceDevice(phip_scene *sc, const phip_render_params *p, const phip_radiance_desc *r, phip_stats *stats) {
    SceneDev &sd = *sc->devs[0];
    const std::string who = "phip_radiance_device: ";
    const size_t n = r->n;
    if (!allOnSceneDevice(sd, { r->d_rays, r->d_out, r->d_stream })) return setErr(PHIP_ERR_INVALID, who + "d_rays, d_out and d_stream must be device memory of the scene's device");
    /* the render parameters of a job without a film: one device, no shards, no callback (its totals are the film's), the flags of the film off */
    phip_render_params q = *p;
    requireSceneDevice(sd, p, who);
    q.device = sd.device; q.n_devices = 0;
    q.flags = (p->flags & PHIP_FLAG_KERNEL_TIMING) | PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND;      /* (a caller's ray has no differentials: nothing is filtered) */
    q.shard_index = 0; q.shard_count = 1; q.block_size = 0; q.progress = nullptr; q.progress_user = nullptr;
    validateParams(sc, &q);

    RenderJob J(sc, sd, &q, nullptr);
    J.nCU = cuCount(sd.device, J.nCU);
    J.stream = sceneStream(sd, q.stream);
    planPasses(J, (unsigned long long) n);
    HIP_TRY(hipMemsetAsync(sd.invalid.p, 0, sizeof(unsigned long long), J.stream));
    setupWavefront(J, J.idsPerSpp * J.sppPerPass);
    J.wf.vertexRays = radianceVertexKernel(J);
    J.wf.rays.rays = (const float4 *) r->d_rays; J.wf.rays.stream = r->d_stream; J.wf.rays.firstStream = r->first_stream; J.wf.rays.n = (uint32_t) n;
    J.wf.rays.pairs = r->stream_layout == PHIP_RADIANCE_STREAM_PAIRS ? 1u : 0u;
    callConstants(J);
    J.rc.envFiltered = 0;
    const bool onePass = J.sppPerPass >= (uint32_t) q.spp;
    if (!onePass && sd.radianceAcc.n < 2 * n) sd.radianceAcc.alloc(2 * n);

    for (uint32_t sppDone = 0; sppDone < (uint32_t) q.spp; sppDone += J.sppPerPass) {
        passConstants(J, sppDone);
        wavefrontPass(J);
        if (J.cancelled) break;                                 /* L is incomplete: d_out is not written */
        if (J.timing) J.evFilm.record(J.stream);
        hipLaunchKernelGGL(sd.radiance.out, dim3(blocksFor(n)), dim3(BLOCK), 0, J.stream, (const float4 *) sd.L.p, onePass ? nullptr : sd.radianceAcc.p,
                           (uint32_t) n, J.rc.sppPass, (uint32_t) q.spp, sppDone == 0 ? 1u : 0u, sppDone + J.rc.sppPass >= (uint32_t) q.spp ? 1u : 0u, (float4 *) r->d_out, sd.invalid.p);
        if (J.timing) J.evFilm.record(J.stream);
        passResults(J);
    }

    phip_stats &st = J.st;
    unsigned long long inv = 0;
    HIP_TRY(hipMemcpy(&inv, sd.invalid.p, sizeof(inv), hipMemcpyDeviceToHost));
    st.invalid_samples = inv;
    st.trace_kernel_ms = J.evTrace.sumPairs(); st.shade_kernel_ms = J.evShade.sumPairs(); st.film_kernel_ms = J.evFilm.sumPairs();     /* (film_kernel_ms: k_radiance_out) */
    st.n_devices = 1;
    st.render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - J.t0).count();
    algorithmicBytes(true, st, 0.0);
    if (stats) *stats = st;
    if (J.cancelled) {
        __atomic_store_n(sc->cancelFlag, 0, __ATOMIC_RELAXED);
        return setErr(PHIP_ERR_CANCELLED, who + "the call was cancelled");
    }
    return PHIP_OK;
}

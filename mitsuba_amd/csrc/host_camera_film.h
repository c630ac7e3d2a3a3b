/*
 * host_camera_film.h -- host side of phip_camera_rays_device and phip_film_device: the two ends of phip_render_device as entry points of their own.  The camera
 * samples of the counter stream go out to the caller's device memory (k_camera_rays), per-sample values of the caller's come in and are filtered onto a film with
 * ImageBlock::put's arithmetic (k_film_values); the kernels: k_camera_film.h in phip_camera_film.hip.  Neither touches the path pool, the sample buffer or a render
 * kernel: what they share with a render is the stream (streamJitter), the camera (cameraRay) and the film's constants in the DevScene.
 * Both validate everything before the first launch -- after a refusal no output buffer has been written -- and use one word of the scene's (SceneDev::invalid) for
 * the pixel list's check and the count of rejected samples; the render lock serialises them with the renders.
 * Host code only; included by phip.hip alone, after host_radiance.h.  The caller holds the scene's render lock.
 */
#pragma once
#include "host_render.h"

/* what both calls read of the parameters, without a device: NULL, or the refusal and its code (`who` has no sampler but the counter stream) */
static const char *cameraFilmParamsError(const phip_render_params *p, int &code) {
    code = PHIP_ERR_INVALID;
    if (p->sampler > PHIP_SAMPLER_HAMMERSLEY) return "unknown sampler kind";
    if (p->n_devices < 0 || p->n_devices > 1) return "one device: the buffers are device memory of the scene's device (n_devices must be 0 or 1)";
    if (p->spp <= 0) return "spp must be > 0";
    if (p->sample_offset < 0) return "sample_offset must not be negative";
    if ((long long) p->sample_offset + p->spp > 0x7FFFFFFFll) return "sample_offset + spp exceeds the 31 bits of a sample index";
    return nullptr;
}

/* What the arguments of phip_camera_rays_device say without a device (the debug library tests it on a machine without one) */
static const char *cameraRaysArgsError(const phip_render_params *p, const phip_camera_rays_desc *r, int &code) {
    code = PHIP_ERR_INVALID;
    if (!p || !r) return "NULL argument";
    if (const char *bad = cameraFilmParamsError(p, code)) return bad;
    if (!r->d_pixels || r->m) {                                 /* (an empty list: no pointer is looked at) */
        if (!r->d_rays) return "d_rays must not be NULL";
        if (misaligned(r->d_rays, 16)) return "d_rays must be 16-byte aligned";
        if (misaligned(r->d_keys, 8) || misaligned(r->d_positions, 8)) return "d_keys and d_positions must be 8-byte aligned";
        if (misaligned(r->d_pixels, 4)) return "d_pixels must be 4-byte aligned";
        if (r->d_pixels && (r->m > CALL_MAX_ITEMS || r->m * (unsigned long long) p->spp > CALL_MAX_ITEMS)) return "more than 2^32 - 256 samples in one call";
    }
    code = PHIP_ERR_UNSUPPORTED;
    if (p->sampler != PHIP_SAMPLER_CTR) return "PHIP_SAMPLER_CTR only: the other samplers' streams are addressed by film coordinates";
    code = PHIP_OK;
    return nullptr;
}

/* ... and those of phip_film_device */
static const char *filmArgsError(const phip_render_params *p, const phip_film_desc *f, int &code) {
    code = PHIP_ERR_INVALID;
    if (!p || !f) return "NULL argument";
    if (const char *bad = cameraFilmParamsError(p, code)) return bad;
    if (p->shard_count > 1) return "shard_count > 1: the call puts every sample of the crop window";
    const int bs = p->block_size > 0 ? p->block_size : 32;
    if (bs < 2 || bs > 128 || (bs & (bs - 1))) return "block_size must be a power of two in [2,128]";
    if (!f->d_values || !f->d_out) return "d_values and d_out must not be NULL";
    if (misaligned(f->d_values, 16) || misaligned(f->d_out, 16)) return "d_values and d_out must be 16-byte aligned";
    if (f->flags & ~PHIP_FILM_SIGNED) return "unknown flag";
    code = PHIP_ERR_UNSUPPORTED;
    if (p->sampler != PHIP_SAMPLER_CTR) return "PHIP_SAMPLER_CTR only: the other samplers' streams are addressed by film coordinates";
    code = PHIP_OK;
    return nullptr;
}

/* ... as the entry points and their test hooks return them */
static int cameraRaysRefusal(const phip_render_params *p, const phip_camera_rays_desc *r) {
    int code = PHIP_OK;
    const char *bad = cameraRaysArgsError(p, r, code);
    return refusal("phip_camera_rays_device", code, bad);
}
static int filmRefusal(const phip_render_params *p, const phip_film_desc *f) {
    int code = PHIP_OK;
    const char *bad = filmArgsError(p, f, code);
    return refusal("phip_film_device", code, bad);
}

/* the constants k_camera_rays and k_film_values read: the stream's, and the samples of the call as one pass */
static RenderConst cameraFilmConstants(const phip_render_params *p, int tileShift) {
    RenderConst rc; memset(&rc, 0, sizeof(rc));
    rc.seed = p->seed; rc.sampler = (uint32_t) p->sampler;
    rc.sppPass = (uint32_t) p->spp; rc.sppFirst = (uint32_t) p->sample_offset;
    rc.sppMagic = (uint32_t) std::min<unsigned long long>((1ull << 32) / rc.sppPass, 0xFFFFFFFFull);
    rc.tileShift = (uint32_t) tileShift; rc.tilePixels = 1u << (2 * tileShift);
    return rc;
}

static int cameraRaysDevice(phip_scene *sc, const phip_render_params *p, const phip_camera_rays_desc *r) {
    SceneDev &sd = *sc->devs[0];
    const std::string who = "phip_camera_rays_device: ";
    const unsigned long long nPixels = (unsigned long long) sd.dev.film.width * (unsigned long long) sd.dev.film.height;
    const unsigned long long m = r->d_pixels ? (unsigned long long) r->m : nPixels;
    if (m == 0) return PHIP_OK;
    if (m * (unsigned long long) p->spp > CALL_MAX_ITEMS) return setErr(PHIP_ERR_INVALID, who + "more than 2^32 - 256 samples in one call");
    if (!allOnSceneDevice(sd, { r->d_rays, r->d_keys, r->d_positions, r->d_pixels })) return setErr(PHIP_ERR_INVALID, who + "d_pixels, d_rays, d_keys and d_positions must be device memory of the scene's device");
    requireSceneDevice(sd, p, who);
    const hipStream_t stream = sceneStream(sd, p->stream);
    const CameraFilmKernels K = phipCameraFilmKernels();
    if (r->d_pixels) {          /* the list, before anything is written */
        unsigned long long bad = 0;
        HIP_TRY(hipMemsetAsync(sd.invalid.p, 0, sizeof(unsigned long long), stream));
        hipLaunchKernelGGL(K.pixelsCheck, dim3(blocksFor(m)), dim3(BLOCK), 0, stream, r->d_pixels, (uint32_t) m, (uint32_t) nPixels, sd.invalid.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(&bad, sd.invalid.p, sizeof(bad), hipMemcpyDeviceToHost));
        if (bad) return setErr(PHIP_ERR_INVALID, who + "d_pixels holds an index that is not below crop_w * crop_h");
    }
    const uint32_t n = (uint32_t) (m * (unsigned long long) p->spp);
    const RenderConst rc = cameraFilmConstants(p, 0);
    hipLaunchKernelGGL(K.rays, dim3(blocksFor(n)), dim3(BLOCK), 0, stream, sd.dev, rc, r->d_pixels, n, (float4 *) r->d_rays, (uint2 *) r->d_keys, (float2 *) r->d_positions);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PHIP_OK;
}

static int filmDevice(phip_scene *sc, const phip_render_params *p, const phip_film_desc *f, phip_stats *stats) {
    SceneDev &sd = *sc->devs[0];
    const std::string who = "phip_film_device: ";
    const auto t0 = std::chrono::steady_clock::now();
    DevScene D = sd.dev;                                        /* ... with this call's block size, as a render's (RenderJob) */
    const int bs = p->block_size > 0 ? p->block_size : 32;
    if (bs < D.film.border) return setErr(PHIP_ERR_INVALID, who + "The block size must be larger than the image reconstruction filter radius!");      /* renderproc.cpp:175-176 */
    D.film.blockSize = bs;
    int tileShift = 0; while ((1 << tileShift) < bs) ++tileShift;
    if (!allOnSceneDevice(sd, { f->d_values, f->d_out })) return setErr(PHIP_ERR_INVALID, who + "d_values and d_out must be device memory of the scene's device");
    requireSceneDevice(sd, p, who);
    const hipStream_t stream = sceneStream(sd, p->stream);
    const CameraFilmKernels K = phipCameraFilmKernels();
    const RenderConst rc = cameraFilmConstants(p, tileShift);
    const bool timing = (p->flags & PHIP_FLAG_KERNEL_TIMING) != 0;
    EventList ev;
    HIP_TRY(hipMemsetAsync(sd.invalid.p, 0, sizeof(unsigned long long), stream));
    if (timing) ev.record(stream);
    hipLaunchKernelGGL(K.film[(f->flags & PHIP_FILM_SIGNED) ? 1 : 0], dim3((D.film.width + 15) / 16, (D.film.height + 15) / 16), dim3(BLOCK), 0, stream, D, rc,
                       (const float4 *) f->d_values, f->d_out, (p->flags & PHIP_FLAG_ACCUMULATE) ? 1 : 0, sd.invalid.p);
    if (timing) ev.record(stream);
    HIP_TRY(hipGetLastError());
    unsigned long long inv = 0;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(&inv, sd.invalid.p, sizeof(inv), hipMemcpyDeviceToHost));
    if (stats) {
        stats->samples = (unsigned long long) D.film.width * (unsigned long long) D.film.height * (unsigned long long) p->spp;
        stats->invalid_samples = inv;
        stats->film_kernel_ms = ev.sumPairs();
        stats->n_devices = 1;
        stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return PHIP_OK;
}

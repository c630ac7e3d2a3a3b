/*
 * host_raycast.h -- host side of phip_trace_device: the caller's rays, in device memory, through the persistent ray server (k_raycast_p) and, where asked for,
 * the surface records behind it (k_surfaces); the kernels: k_raycast.h in phip_raycast.hip.
 * The server's grid is its resident set (asked of the runtime, as for k_rays_w: setupWavefrontGrids), so the region its group stacks spill to covers the grid
 * and not the rays: no chunking, and nothing is allocated after a scene's first call -- the spill region, the draw counters and the per-wave statistics are the
 * buffers the wavefront render keeps in the SceneDev (the render lock serialises the two).  The plan is resolved once per scene and again when the node cache
 * changed (phip_scene_rebuild: another tree, another LDS plan).
 * Host code only; included by phip.hip alone, after host_render.h.  The caller holds the scene's render lock.
 */
#pragma once
#include "host_render.h"

/* the server's kernels, LDS plan and resident grid for this scene's tree */
static void planRaycast(SceneDev &sd) {
    SceneDev::RaycastPlan &R = sd.raycast;
    const DevScene &D = sd.dev;
    if (R.k.cast && R.nodeCache == D.wideNodeCache) return;
    R.k = phipRaycastKernels();
    R.lds = wideLdsBytes(D.wideNodeCache, WIDE_BLOCK) + wideDealBytes(WIDE_BLOCK);
    const Residency res = residentBlocksPerCU((const void *) R.k.cast, WIDE_BLOCK, R.lds);
    if (res.limit != hipSuccess) throw std::runtime_error(std::string("k_raycast_p: hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize): ") + hipGetErrorString(res.limit));
    const int nCU = cuCount(sd.device, 256);
    const int perCU = std::max(1, std::min(res.blocks > 0 ? res.blocks : 1, WIDE_WAVES * 256 / WIDE_BLOCK));
    R.blocks = (unsigned) (nCU * perCU);
    R.nodeCache = D.wideNodeCache;
}

static int traceDevice(phip_scene *sc, const phip_ray *dRays, size_t n, phip_hit *dHits, uint8_t *dOccluded, phip_surface *dSurfaces, void *callerStream, phip_stats *stats) {
    SceneDev &sd = *sc->devs[0];
    const std::string who = "phip_trace_device: ";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (dSurfaces && !dHits) return setErr(PHIP_ERR_INVALID, who + "d_surfaces needs d_hits");
    if (n == 0) return PHIP_OK;
    if (n > CALL_MAX_ITEMS) return setErr(PHIP_ERR_INVALID, who + "more than 2^32 - 256 rays in one call");
    const auto t0 = std::chrono::steady_clock::now();
    const void *ptrs[4] = { dRays, dHits, dSurfaces, dOccluded };
    for (int i = 0; i < 4; ++i) {
        if (!ptrs[i]) continue;
        if (!onSceneDevice(ptrs[i], sd.device)) return setErr(PHIP_ERR_INVALID, who + "rays, hits, occlusion and surfaces must be device memory of the scene's device");
        if (i < 3 && misaligned(ptrs[i], 16)) return setErr(PHIP_ERR_INVALID, who + "rays, hits and surfaces must be 16-byte aligned");
    }
    planRaycast(sd);
    const SceneDev::RaycastPlan &R = sd.raycast;
    const hipStream_t stream = sceneStream(sd, callerStream);
    const unsigned blocks = (unsigned) std::min<size_t>(R.blocks, (n + WIDE_BLOCK - 1) / WIDE_BLOCK);
    /* the buffers cover the resident grid, whatever this call's: a later call of any size finds them */
    const size_t spillWords = (size_t) R.blocks * WIDE_BLOCK * SPILL_DEPTH, nWavesMax = (size_t) R.blocks * (WIDE_BLOCK / 64);
    if (sd.spill.n < spillWords) sd.spill.alloc(spillWords);
    if (sd.stat.n < (size_t) ST_COUNT * nWavesMax) sd.stat.alloc((size_t) ST_COUNT * nWavesMax);
    if (sd.drawCounters.n < 2 * RAY_SHARDS * RAY_SHARD_STRIDE) sd.drawCounters.alloc(2 * RAY_SHARDS * RAY_SHARD_STRIDE);
    PathPool P; memset(&P, 0, sizeof(P));
    P.stat = sd.stat.p; P.nWaves = blocks * (WIDE_BLOCK / 64); P.spill = sd.spill.p; P.spillLanes = (uint32_t) std::min<size_t>(sd.spill.n / SPILL_DEPTH, 0xFFFFFFFFu);
    const int rows = ST_SH_TRI + 1;                        /* the six rows the server writes */
    HIP_TRY(hipMemsetAsync(sd.stat.p, 0, (size_t) rows * P.nWaves * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(sd.drawCounters.p, 0, 2 * RAY_SHARDS * RAY_SHARD_STRIDE * sizeof(unsigned int), stream));
    EventList ev;
    ev.record(stream);
    hipLaunchKernelGGL(R.k.cast, dim3(blocks), dim3(WIDE_BLOCK), R.lds, stream, sd.dev, (const float4 *) dRays, (uint32_t) n, (float4 *) dHits, dOccluded, P, sd.drawCounters.p);
    ev.record(stream);
    if (dSurfaces) hipLaunchKernelGGL(R.k.surfaces, dim3(blocksFor(n)), dim3(BLOCK), 0, stream, sd.dev, (const float4 *) dRays, (const float4 *) dHits, (uint32_t) n, (float4 *) dSurfaces);
    ev.record(stream);
    if (stats) {
        HIP_TRY(hipMemsetAsync(sd.counters.p, 0, sizeof(Counters), stream));
        hipLaunchKernelGGL(k_reduce_stats, dim3(rows, REDUCE_SPLIT), dim3(256), 0, stream, P, sd.counters.p, 0);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    if (stats) {
        Counters hc; HIP_TRY(hipMemcpy(&hc, sd.counters.p, sizeof(hc), hipMemcpyDeviceToHost));
        stats->closest_rays = hc.total[ST_CLOSEST_RAYS]; stats->shadow_rays = hc.total[ST_SHADOW_RAYS];
        stats->closest_node_visits = hc.total[ST_NODE]; stats->closest_triangle_tests = hc.total[ST_TRI];
        stats->shadow_node_visits = hc.total[ST_SH_NODE]; stats->shadow_triangle_tests = hc.total[ST_SH_TRI];
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, ev.ev[0], ev.ev[1])); HIP_TRY(hipEventElapsedTime(&b, ev.ev[1], ev.ev[2]));
        stats->trace_kernel_ms = a; stats->shade_kernel_ms = dSurfaces ? b : 0.0;      /* (k_surfaces: the one shading-side kernel of this call) */
        stats->iterations = 1; stats->n_devices = 1;
        algorithmicBytes(true, *stats, 0.0);
        stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return PHIP_OK;
}

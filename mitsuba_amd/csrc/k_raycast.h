/*
 * k_raycast.h -- the kernels of phip_trace_device (phip_raycast.hip): k_raycast_p, the persistent ray server of k_wide.h fed from a caller's ray array in device
 * memory, and k_surfaces, the surface record at every hit (phip_surface, include/phip.h).
 *
 * k_raycast_w (phip_trace) gives every lane one ray and no second one: a wave stays in its loop until its slowest ray is done.  The wavefront's ray kernel does
 * not -- its waves are persistent, refill the lanes that went idle and deal the Wald tests of a round over the whole wave (persistentTraverseWide) -- but it
 * could be fed from nothing but the path pool.  Here its two sources are stated over the ray array: work units are chunks of 64 rays, dealt statically and then
 * drawn from the sharded counters (DrawCounter: one returning atomic per 64 rays), the any-hit pass and the closest-hit pass of a call run in one launch.
 * A caller's rays are not pre-clipped as the pool's are, so the sources clip in `load` (clipToScene, the arithmetic phip_trace clips with); a ray that misses the
 * scene box comes out with an empty interval and the loop commits its miss without traversing, as it does for the pool's.
 * The hit is decided by the same Wald test on the same records with the same tie rule (winsTie as an LDS min), so hits and occlusion are k_raycast_w's bits.
 * The surface fill is a kernel of its own: in the server it would take the registers its seven waves per SIMD live on (tests/test_kernel_resources_raycast.py).
 */
#pragma once

/* the source state both passes share: chunk `chunk` of 64 rays, `pos` rays of it handed out (wave-uniform: SGPRs) */
struct RayArrayChunks {
    uint32_t n; DrawCounter q; uint32_t chunk, pos;
    __device__ __forceinline__ void start() { chunk = q.total ? WIDE_UNIFORM(q.draw()) : 0xFFFFFFFFu; pos = 0; }       /* (a pass the caller did not ask for has no units: no draw) */
    __device__ __forceinline__ bool more() const { return chunk != 0xFFFFFFFFu; }
    __device__ __forceinline__ uint32_t assign(bool want, unsigned long long wantMask) {
        const uint32_t idx = pos + (uint32_t) __popcll(wantMask & ((1ull << __lane_id()) - 1ull));
        const uint32_t h = (want && idx < 64u && chunk * 64u + idx < n) ? chunk * 64u + idx : INVALID_RAY;
        pos = WIDE_UNIFORM(pos + (uint32_t) __popcll(wantMask));
        if (pos >= 64u) start();
        return h;
    }
};
/* ray i of the array, clipped to the scene box: an empty interval (maxt < mint) where the clip says that the ray misses it */
template <bool SHADOW>
__device__ __forceinline__ void loadArrayRay(const DevScene &S, const float4 *rays, uint32_t i, V3 &o, V3 &d, float &mint, float &maxt) {
    const float4 ro = rays[2 * (size_t) i], rd = rays[2 * (size_t) i + 1];
    o = V3(ro.x, ro.y, ro.z); d = V3(rd.x, rd.y, rd.z);
    V3 slab;              /* (the loop takes its slab reciprocal from v_rcp_f32: slabRcpFast) */
    if (!clipToScene<SHADOW>(S, o, d, ro.w, rd.w, mint, maxt, slab)) { mint = 0.0f; maxt = -1.0f; }
}
struct RayArrayClosest : RayArrayChunks {
    const DevScene &S; const float4 *rays; float4 *hits;
    __device__ __forceinline__ RayArrayClosest(const DevScene &S, const float4 *rays, float4 *hits, uint32_t n) : RayArrayChunks{ n, {}, 0u, 0u }, S(S), rays(rays), hits(hits) {}
    __device__ __forceinline__ bool load(uint32_t i, V3 &o, V3 &d, float &mint, float &maxt) const { loadArrayRay<false>(S, rays, i, o, d, mint, maxt); return true; }
    __device__ __forceinline__ void commit(uint32_t i, bool, const TravResult &r) const {
        hits[i] = make_float4(r.t, r.u, r.v, pm_from_bits(hitPrim(r.prim)));      /* (r.prim carries the shade class of the record: k_pool.h; phip_hit does not) */
    }
};
struct RayArrayAny : RayArrayChunks {
    const DevScene &S; const float4 *rays; uint8_t *occluded;
    __device__ __forceinline__ RayArrayAny(const DevScene &S, const float4 *rays, uint8_t *occluded, uint32_t n) : RayArrayChunks{ n, {}, 0u, 0u }, S(S), rays(rays), occluded(occluded) {}
    __device__ __forceinline__ bool load(uint32_t i, V3 &o, V3 &d, float &mint, float &maxt) const { loadArrayRay<true>(S, rays, i, o, d, mint, maxt); return true; }
    __device__ __forceinline__ void commit(uint32_t i, bool occ, const TravResult &) const { occluded[i] = occ ? 1 : 0; }
};

/* P: the statistics rows (stat, nWaves: the grid's waves) and the spill region (SPILL_DEPTH words per lane of the grid) only; hits / occluded may be NULL: that pass has no work */
__global__ __launch_bounds__(WIDE_BLOCK, WIDE_WAVES) void k_raycast_p(DevScene S, const float4 *rays, uint32_t n, float4 *hits, uint8_t *occluded, PathPool P,
                                                                      unsigned int *drawCounters /* 2 * RAY_SHARDS lines, zeroed */) {
    __shared__ unsigned long long wcnt[WIDE_BLOCK / 64][WW_COUNT];
    const uint32_t wave = WIDE_UNIFORM(threadIdx.x >> 6), waveId = blockIdx.x * (WIDE_BLOCK / 64) + wave;
    if (threadIdx.x < (WIDE_BLOCK / 64) * WW_COUNT) (&wcnt[0][0])[threadIdx.x] = 0;
    WideStackT<WIDE_BLOCK> stk; setupWide<WIDE_BLOCK>(S, S.wideNodeCache, g_smem, P.spill + (size_t) blockIdx.x * WIDE_BLOCK * SPILL_DEPTH, stk);   /* (barrier inside) */
    const uint32_t nChunk = (n + 63u) / 64u, nWavesGrid = gridDim.x * (WIDE_BLOCK / 64);
    RayArrayAny ss(S, rays, occluded, n);
    RayArrayClosest ts(S, rays, hits, n);
    ss.q.init(drawCounters, blockIdx.x % RAY_SHARDS, occluded ? nChunk : 0u, waveId, nWavesGrid);
    ts.q.init(drawCounters + RAY_SHARDS * RAY_SHARD_STRIDE, blockIdx.x % RAY_SHARDS, hits ? nChunk : 0u, waveId, nWavesGrid);
    ss.start(); ts.start();
    persistentTraverseWide(S, stk, ss, ts, wcnt[wave], g_smem + wideLdsBytes(S.wideNodeCache, WIDE_BLOCK) + wave * WD_WAVE_BYTES);
    if (__lane_id() == 0) {
        const unsigned long long v[6] = { wcnt[wave][WW_RAYS], wcnt[wave][WW_STEPS] & 0xFFFFFFFFull, wcnt[wave][WW_STEPS] >> 32,
                                          wcnt[wave][WW_SH_RAYS], wcnt[wave][WW_SH_STEPS] & 0xFFFFFFFFull, wcnt[wave][WW_SH_STEPS] >> 32 };
        const int rows[6] = { ST_CLOSEST_RAYS, ST_NODE, ST_TRI, ST_SHADOW_RAYS, ST_SH_NODE, ST_SH_TRI };
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (v[i]) P.stat[(size_t) rows[i] * P.nWaves + waveId] += v[i];
    }
}

/* one lane per ray, behind the traversal on the same stream: hit + ray direction -> the 64-byte record (fillSurface, dv_scene.h), four 16-byte stores */
__global__ __launch_bounds__(BLOCK) void k_surfaces(DevScene S, const float4 *rays, const float4 *hits, uint32_t n, float4 *out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 h = hits[i], rd = rays[2 * (size_t) i + 1];
    phip_surface s;
    fillSurface(S, V3(rd.x, rd.y, rd.z), h.x, h.y, h.z, pm_to_bits(h.w), s);
    float4 *o = out + 4 * (size_t) i;
    o[0] = make_float4(s.p[0], s.p[1], s.p[2], s.t);
    o[1] = make_float4(s.ng[0], s.ng[1], s.ng[2], pm_from_bits(s.prim));
    o[2] = make_float4(s.ns[0], s.ns[1], s.ns[2], pm_from_bits(s.flags));
    o[3] = make_float4(s.uv[0], s.uv[1], pm_from_bits(s.material), pm_from_bits((uint32_t) s.emitter));
}

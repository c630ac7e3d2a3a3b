/*
 * k_shade_trace_w.h -- k_shade_trace_w: k_shade_trace (k_shade_trace.h: one path vertex AND its two rays in one kernel) on the compressed 8-wide tree in memory, for
 * the scenes between the packed leaf table (at most 64 Wald records) and the big trees whose feature set keeps them off k_mega: bitmap textures, texture coordinates,
 * a `constant` / `envmap` emitter.  Such a scene -- a Cornell box with two 500-triangle spheres, one of them with a bitmap albedo -- ran the wavefront's three launches
 * per iteration (k_shade -> k_rays_w, ~350 B of path state per vertex through HBM) around a tree that lives in L2.
 *
 * Same head as k_shade_trace: slot load, the lane deal by BSDF model, shadeVertex with the LPending policy, shadeEpilogue.  The traversal is traceWidePool
 * (k_wide_wave.h): ONE call per block of slots that carries the vertex's shadow ray and the slot's next ray together -- 64 closest-hit rays and the ~34 shadow rays of
 * a wave's vertices fill its node visits where the shadow rays alone left every iteration half empty.  The vertex's additions (`pend`) and the sample id
 * they belong to stay in registers across the epilogue and join L[id] after the call in the order k_shade_trace adds them: the vertex's own terms, then the shadow
 * ray's contribution -- same bits.
 *
 * The grid is PERSISTENT: the kernel's resident set, every block walking the blocks of BLOCK slots blk = blockIdx.x, blockIdx.x + gridDim.x, ...  A wave's task stack
 * spills into its lanes' share of the spill buffer (WP_SPILL_CAP), which therefore has to cover the GRID and not the pool -- the buffer k_rays_w's persistent grid has
 * already (phip.hip: setupWavefront), not 1.6 GB for a pool of 4 M slots; and the top of the tree and the scene tables are staged once per resident block, not once per
 * 256 slots.
 *
 * Dynamic LDS: [the four waves' task stacks][nodeCache nodes][the four waves' slots / ray tables / pair lists, under the class deal's exchange buffer][emitter table]
 * [materials] (shadeTraceWideLdsBytes).  The tables are staged when they fit, as in k_shade (stageShadeTables: generic pointers) -- no limit on their size.
 * A task stack that outgrows LDS + spill stops its wave's traversals (traceWidePool: `overflow`); the wave says so in the ST_GAVE_UP row, the host discards the pass and
 * renders it, and the rest of the job, on k_shade + k_rays_w (phip.hip) -- k_mega's contract.
 */
#pragma once

#ifndef SHADE_TRACE_W_WAVES
#define SHADE_TRACE_W_WAVES 4            /* a block's ~40 KB of LDS admit four blocks per CU, whatever the registers say: <= 128 VGPRs */
#endif

/* the exchange buffer of the class deal (builds with more than one BSDF model) lies over the traversal's per-wave buffers: it is used at the head of a block of slots,
   they after the epilogue's barriers */
__host__ __device__ __forceinline__ size_t shadeTraceWideTablesOffset(uint32_t nodeCache, bool deal) {
    const size_t waves = (size_t) (BLOCK / 64u) * WP_WAVE_BYTES;
    return widePoolDealOffset(nodeCache) + ((deal && SHADE_DEAL_BYTES > waves) ? (size_t) SHADE_DEAL_BYTES : waves);
}
__host__ __device__ __forceinline__ size_t shadeTraceWideLdsBytes(uint32_t nodeCache, bool deal) {
    return shadeTraceWideTablesOffset(nodeCache, deal) + EMITTER_LDS_FLOATS * sizeof(float) + MATERIAL_LDS_MAX * sizeof(DevMaterial);
}
static_assert(SHADE_DEAL_BYTES % 16 == 0 && WP_WAVE_BYTES % 16 == 0 && sizeof(DevMaterial) % 16 == 0, "the tables behind the deal buffer are staged with 16-byte stores");

template <int MM, bool STRICT, int FEAT> __global__ __launch_bounds__(BLOCK, SHADE_TRACE_W_WAVES) void k_shade_trace_w(DevScene S, PathPool P, RenderConst rc, float4 *L, uint32_t nodeCache) {
    __shared__ uint32_t waveCnt[BLOCK / 64];
    __shared__ uint32_t clsCnt[4][BLOCK / 64];
    __shared__ unsigned long long wcnt[BLOCK / 64][2];           /* node visits | triangle tests << 32 of the wave's any-hit / closest-hit rays (traceWidePool) */
    const uint32_t lane = __lane_id(), wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    unsigned char *const xbuf = g_smem + widePoolDealOffset(nodeCache);
    float *const ldsEm = (float *) (g_smem + shadeTraceWideTablesOffset(nodeCache, MM != 0));
    DevMaterial *const ldsMat = (DevMaterial *) (ldsEm + EMITTER_LDS_FLOATS);
    const ShadeTables tab = stageShadeTables(S, ldsEm, ldsMat);
    unsigned long long *const wc = wcnt[wave];
    if (lane < 2u) wc[lane] = 0ull;                              /* (every wave its own row) */
    WidePool wp;
    setupWidePool(S, nodeCache, g_smem, P.spill + (size_t) blockIdx.x * BLOCK * SPILL_DEPTH, wave, wp);     /* (barrier inside: the LDS tables are complete) */
    bool overflow = false;
    unsigned long long nClosest = 0, nShadow = 0;
    const uint32_t nBlk = P.capacity / BLOCK;                    /* (the pool's capacity is a multiple of BLOCK: every lane has a slot) */

    for (uint32_t blk = blockIdx.x; blk < nBlk; blk += gridDim.x) {
        if (rc.draining && P.blockDead[blk]) continue;          /* (block-uniform) */
        uint32_t slot = blk * BLOCK + threadIdx.x;
        bool inRange = slot < P.capacity;
        const uint32_t lslot = inRange ? slot : 0u;
        uint4 info = P.info[lslot];
        info.w = P.state[lslot];
        PathVertex v;
        v.hit = P.hit[lslot];
        v.rayD = P.rayD[lslot];
        v.thr = P.thr[lslot];
        v.mis = P.mis[lslot];
        v.rayO = make_float4(0, 0, 0, 0);
        /* the lane deal by BSDF model (k_shade.h: dealSlotsByClass): the class is what THIS kernel left in the hit word when it traced the ray.  Its first barrier is
           behind every wave's traversal of the previous block of slots, whose buffers the exchange buffer lies over */
        if (MM != 0 && SHADE_SORT && S.shadeSort) dealSlotsByClass(xbuf, clsCnt, P, info, v, slot, inRange);
        v.hit.w = pm_from_bits(hitPrim(pm_to_bits(v.hit.w)));
        if (!inRange) info = make_uint4(0, 0, 0, 0);
        const bool alive = inRange && (info.w & F_ALIVE);
        bool needNew = inRange && !alive && !(info.w & F_DEAD);
        unsigned long long vertices = 0, done = 0;
        bool pushShadow = false, newRay = false;
        ShadowEntry sh; sh.e0 = make_float4(0, 0, 0, 0); sh.e1 = sh.e0; sh.e2 = sh.e0;
        float4 pend = make_float4(0, 0, 0, 0); bool havePend = false;
        const uint32_t oldId = info.x;                           /* the sample the vertex's additions belong to: the epilogue may start the slot's next one */

        if (alive) {
            v.id = info.x; v.pixel = info.y; v.k = info.z; v.state = info.w;
            uint32_t nv = 0;
            const LPending acc{ L, P, slot, pend, havePend };
            if (shadeVertex<MM, STRICT, FEAT>(S, tab.T, tab.materials, rc, v, acc, newRay, pushShadow, sh, nv)) {
                vertices = nv; done = 1;
                needNew = true;
            } else {
                info.w = v.state;
                P.state[slot] = info.w;
            }
            if (newRay) { P.rayO[slot] = v.rayO; P.rayD[slot] = v.rayD; P.thr[slot] = v.thr; P.mis[slot] = v.mis; }
        }

        /* ---- regeneration (shadeEpilogue: static schedule + dynamic tail; its barriers separate the deal's exchange from the traversal's buffers) ---- */
        NextRay next{ v.rayO, v.rayD, false };
        shadeEpilogue<(FEAT & 8) != 0>(S, P, rc, waveCnt, slot, inRange, info, alive, needNew, false, sh.e0, sh.e1, sh.e2, vertices, done, blk, &next);

        /* ---- the vertex's shadow ray (path.cpp:187-199) and the next ray of every live slot: one traversal of the wave ---- */
        {
            const V3 so(sh.e0.x, sh.e0.y, sh.e0.z), sd(sh.e1.x, sh.e1.y, sh.e1.z);
            float smint, smaxt; V3 srcp;
            const bool goS = pushShadow & clipToSceneSel<true>(S, so, sd, PT_EPSILON, sh.e0.w, smint, smaxt, srcp);
            const V3 o(next.ro.x, next.ro.y, next.ro.z), d(next.rd.x, next.rd.y, next.rd.z);
            float mint, maxt; V3 rcp;
            const bool goC = next.alive & clipToSceneSel<false>(S, o, d, next.ro.w, next.rd.w, mint, maxt, rcp);
            bool occluded = false; TravResult r;
            traceWidePool<true, true>(S, wp, lane, goS, so, sd, smint, smaxt, goC, o, d, mint, maxt, occluded, r, wc, wc + 1, overflow);
            joinShadow(L, sh, pushShadow && !occluded, pend, havePend);
            if (havePend) L[oldId] = pend;
            if (next.alive) P.hit[slot] = packHitWord(r);
        }
        nClosest += next.alive ? 1ull : 0ull;
        nShadow += pushShadow ? 1ull : 0ull;
    }

    /* the work counters of this wave's blocks of slots, in the rows of the wave's place in the GRID (fewer waves than the pool has: the rows are sums) */
    const uint32_t waveId = blockIdx.x * (BLOCK / 64) + wave;
    const unsigned long long stS = lane == 0u ? wc[0] : 0ull, stC = lane == 0u ? wc[1] : 0ull;
    tracedStats(P, waveId, nClosest, nShadow, stC & 0xFFFFFFFFull, stC >> 32, stS & 0xFFFFFFFFull, stS >> 32);
    /* a wave whose task stack overflowed says so in a row of its own (one owner per entry, zeroed by the host before the pass): the host discards the pass */
    if (__any(overflow) && lane == 0u) P.stat[(size_t) ST_GAVE_UP * P.nWaves + waveId] = 1ull;
}

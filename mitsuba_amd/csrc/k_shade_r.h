/*
 * k_shade_r.h -- the kernels of phip_radiance_device (phip_shade_r.hip): k_shade_r, the wavefront vertex kernel whose slots take the samples they start from a
 * caller's ray array instead of the film, and k_radiance_out, the mean of every ray's samples.
 *
 * k_shade_r is k_shade with another sample source behind its epilogue (shadeEpilogueRays below).  Sample id -> (ray = id / sppPass, k = id mod sppPass + sppFirst); the
 * ray is two 16-byte loads, clipped like a camera ray (preclipRay in the epilogue); the sample's counter stream is that of "pixel" = the ray's stream key, so
 * a ray with key p and sample k draws what phip_render draws for sample k of pixel p.  Every id of a pass names a ray (the film's ids of edge blocks outside the
 * crop window have no counterpart), the static schedule, the dynamic tail, the shadow queue, the class deal and the pass protocol are k_shade's as they are.
 * The caller's ray has no differentials: FEAT bit 5 compiles the first vertex's texture partials and the filtered environment look-up of a camera ray out, so the
 * first vertex reads bitmap textures and the environment map the way every later vertex does (level 0, bilinear).
 */
#pragma once

/* the sample source of k_shade_r: n rays of (o, mint | d, maxt), their stream keys (NULL: firstStream + ray index) -- or, with `pairs` (phip_radiance_desc::stream_layout
   = PHIP_RADIANCE_STREAM_PAIRS), n pairs (key, sample): the ray's own sample index, on top of which the call's k counts (one 8-byte load in place of the 4-byte one) */
struct RaySamples {
    static constexpr bool RAYS = true;
    const float4 *rays; const uint32_t *stream; uint32_t firstStream, n, pairs;
    /* the sample of id `id` (< rc.totalIds = n * rc.sppPass, so ray < n): its stream key, sample index and ray */
    __device__ __forceinline__ void sample(const RenderConst &rc, unsigned long long id, uint32_t &key, uint32_t &k, V3 &o, V3 &d, float &mint, float &maxt) const {
        const uint32_t r = (uint32_t) id;                           /* ids of a pass are < 2^32 */
        uint32_t ray = __umulhi(r, rc.sppMagic);                    /* floor(r / sppPass) or one less (decodeId, k_pool.h) */
        k = r - ray * rc.sppPass;
        if (k >= rc.sppPass) { k -= rc.sppPass; ++ray; }
        k += rc.sppFirst;
        const float4 ro = rays[2 * (size_t) ray], rd = rays[2 * (size_t) ray + 1];
        o = V3(ro.x, ro.y, ro.z); d = V3(rd.x, rd.y, rd.z); mint = ro.w; maxt = rd.w;
        if (pairs) { const uint2 ks = ((const uint2 *) stream)[ray]; key = ks.x; k += ks.y; }       /* (block-uniform: a kernel argument) */
        else key = stream ? stream[ray] : firstStream + ray;
    }
};

#define SHADE_FEAT_NO_DIFFERENTIALS 32      /* FEAT bit 5 (shadeVertex): the sample's first ray carries no differentials */

/* shadeEpilogue (k_shade.h) with the ray array as the source of samples: the shadow-queue compaction, the static schedule, the dynamic tail, retirement and the
   statistics are its text, statement by statement; what differs is marked "rays".  (A copy, not a template over the source: shadeEpilogue declares LDS words, their
   names and the inlining order of its callers decide the code of every kernel that calls it, and those code objects are held to what they were.) */
__device__ __forceinline__ void shadeEpilogueRays(const RaySamples &src, const DevScene &S, const PathPool &P, const RenderConst &rc, uint32_t *waveCnt,
                                              const uint32_t slot, const bool inRange, uint4 info, const bool alive, bool needNew,
                                              const bool pushShadow, const float4 sh0, const float4 sh1, const float4 sh2,
                                              const unsigned long long vertices, const unsigned long long done,
                                              const uint32_t blk /* the block of BLOCK slots this thread block works on: blockIdx.x, but for k_shade_trace_w, whose persistent grid walks them */,
                                              NextRay *next = nullptr) {
    /* ---- shadow queue: compact this block's entries to the front of its own region (no global atomics) ---- */
    uint32_t shadowTotal = 0;
    {
        const unsigned long long m = __ballot(pushShadow);
        const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
        if (lane == 0) waveCnt[wave] = (uint32_t) __popcll(m);
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < BLOCK / 64; ++w) { const uint32_t c = waveCnt[w]; if (w < wave) base += c; total += c; }
        if (pushShadow) {
            const size_t sidx = (size_t) blk * BLOCK + base + (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
            float4 e0 = sh0, e1 = sh1;
            if (S.preclip) preclipShadow(S, e0, e1);
            P.shadow[3 * sidx] = e0; P.shadow[3 * sidx + 1] = e1; P.shadow[3 * sidx + 2] = sh2;
        }
        if (threadIdx.x == 0) P.shadowCount[blk] = total;
        shadowTotal = total;
    }

    /* ---- regeneration: the lane starts a new camera path right away (integrator.cpp:157-183).
       Sample ids [0, staticIds) follow a static schedule (slot s renders s, s + capacity, ... -- no global
       counter in steady state).  The last part of the frame is handed out dynamically so that slots whose
       paths happened to be short keep working until the frame is really finished: one atomicAdd per BLOCK
       on one of DYN_SHARDS counters (block-aggregated through LDS; each shard owns a contiguous id range). ---- */
    bool nowAlive = alive && !needNew;
    unsigned long long newId = ~0ull;
    bool wantDyn = false;
    if (needNew) {
        unsigned long long id = (info.w & F_FRESH) ? (unsigned long long) slot      /* first sample of this slot */
                              : ((info.w & F_DYNAMIC) ? ~0ull : (unsigned long long) info.x + P.capacity);
        if (id >= rc.staticIds) wantDyn = true;
        else newId = id;            /* rays: every id of the pass names a ray, none is skipped */
    }
    bool dynamicId = false;
    {
        const unsigned long long m = __ballot(wantDyn);
        const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
        __syncthreads();                                   /* waveCnt is reused from the shadow compaction */
        if (lane == 0) waveCnt[wave] = (uint32_t) __popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < BLOCK / 64; ++w) { const uint32_t c = waveCnt[w]; if (w < wave) before += c; total += c; }
        if (total) {                                       /* block-uniform */
            __shared__ unsigned long long dynBase;
            __shared__ uint32_t dynShard;
            if (threadIdx.x == 0) {
                uint32_t sh = (blk + rc.blockShard[blk]) % DYN_SHARDS;    /* blockShard = shards this block has seen run dry */
                uint32_t dry = 0;
                unsigned long long base = ~0ull;
                for (int tries = 0; tries < DYN_SHARDS; ++tries) {
                    const unsigned long long old = atomicAdd(rc.dynCounter + (size_t) sh * DYN_STRIDE, (unsigned long long) total);
                    if (old < rc.shardIds) { base = old; break; }
                    sh = (sh + 1) % DYN_SHARDS; ++dry;     /* this shard is used up: move on for good */
                }
                if (dry) rc.blockShard[blk] += dry;
                dynBase = base; dynShard = sh;
            }
            __syncthreads();
            if (wantDyn) {
                bool got = false;
                if (dynBase != ~0ull) {
                    const unsigned long long off = dynBase + before + (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
                    const unsigned long long id = rc.staticIds + (unsigned long long) dynShard * rc.shardIds + off;
                    if (off < rc.shardIds && id < rc.totalIds) { got = true; newId = id; dynamicId = true; }      /* rays */
                }
                if (!got && dynBase == ~0ull) { info.w = F_DEAD; P.state[slot] = F_DEAD; }   /* all shards empty: slot dies */
                else if (newId == ~0ull) { info.w = F_DYNAMIC; P.state[slot] = F_DYNAMIC; }                        /* try again next iteration */
            }
        }
    }
    if (newId != ~0ull) {
        uint32_t k, pixel;          /* rays: `pixel` is the ray's stream key */
        V3 o, d; float mint, maxt;
        src.sample(rc, newId, pixel, k, o, d, mint, maxt);
        float4 ro = make_float4(o.x, o.y, o.z, mint), rd = make_float4(d.x, d.y, d.z, maxt);
        if (S.preclip) preclipRay(S, ro, rd);
        P.rayO[slot] = ro;
        P.rayD[slot] = rd;
        if (next) { next->ro = ro; next->rd = rd; }
        P.thr[slot] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        P.mis[slot] = make_float2(0.0f, 0.0f);
        info = make_uint4((uint32_t) newId, pixel, k, 1u | F_ALIVE | F_EMITTED | F_FIRST | (dynamicId ? F_DYNAMIC : 0u));
        P.info[slot] = info;
        P.state[slot] = info.w;
        nowAlive = true;
    }
    if (next) next->alive = nowAlive;
    const uint32_t waveId = (blk * BLOCK + threadIdx.x) >> 6;      /* the wave's position in the grid (NOT slot >> 6: k_shade may have permuted the block's slots) */
    /* a slot still waiting for a dynamic sample id counts as live for the termination test */
    const bool live = nowAlive || (inRange && info.w == F_DYNAMIC);
    /* the block retires once none of its slots will ever work again and its last shadow entries have been consumed
       (this launch queued nothing, so shadowCount is 0): later launches of the pass return at the first line */
    const bool retire = !__syncthreads_or(live ? 1 : 0) && shadowTotal == 0;
    if (retire && threadIdx.x == 0) P.blockDead[blk] = 1u;
    if (inRange || (slot & ~63u) < P.capacity) {
        waveStat(P, ST_VERTICES, waveId, vertices);
        waveStat(P, ST_SAMPLES, waveId, done);
        if (rc.countAlive || retire) waveStat(P, ST_ALIVE, waveId, live ? 1ull : 0ull, true);
    }
}


/* k_shade (k_shade.h) line by line -- the head of the block in one round trip, the tables in LDS, the deal by BSDF class, one vertex per live slot -- with the
   ray array behind its epilogue.  The wave budgets are k_shade's, instantiation by instantiation. */
template <int MM, bool STRICT, int FEAT> __global__ __launch_bounds__(BLOCK, MM == 0 ? SHADE_WAVES_LEAN : ((FEAT & 3) == 0 ? SHADE_WAVES_PLAIN : SHADE_WAVES)) void k_shade_r(DevScene S, PathPool P, RenderConst rc, float4 *L, RaySamples src) {
    __shared__ uint32_t waveCnt[BLOCK / 64];
    __shared__ __align__(16) float ldsEm[EMITTER_LDS_FLOATS];
    __shared__ DevMaterial ldsMat[MATERIAL_LDS_MAX];
    if (rc.draining && P.blockDead[blockIdx.x]) return;         /* (block-uniform) */
    uint32_t slot = blockIdx.x * BLOCK + threadIdx.x;
    bool inRange = slot < P.capacity;
    uint32_t lslot = inRange ? slot : 0u;
    uint4 info = P.info[lslot];
    info.w = P.state[lslot];
    PathVertex v;
    v.hit = P.hit[lslot];
    v.rayD = P.rayD[lslot];
    v.thr = P.thr[lslot];
    v.mis = P.mis[lslot];
    ShadeTables tab = stageShadeTables<(FEAT & 16) == 0>(S, ldsEm, ldsMat);
    if (FEAT & 4) { tab.T.t = ldsEm; tab.materials = ldsMat; }
    else if (FEAT & 16) { tab.T.t = ldsEm; tab.materials = S.materials; }
    if (MM != 0 && SHADE_SORT && S.shadeSort) {                 /* (block-uniform) */
        __shared__ __align__(16) unsigned char xbuf[SHADE_DEAL_BYTES];
        __shared__ uint32_t clsCnt[4][BLOCK / 64];
        dealSlotsByClass(xbuf, clsCnt, P, info, v, slot, inRange);
    }
    v.hit.w = pm_from_bits(hitPrim(pm_to_bits(v.hit.w)));
    if (!inRange) info = make_uint4(0, 0, 0, 0);
    __syncthreads();                                            /* LDS tables are complete */
    bool alive = inRange && (info.w & F_ALIVE);
    bool needNew = inRange && !alive && !(info.w & F_DEAD);
    unsigned long long vertices = 0, done = 0;
    bool pushShadow = false;
    ShadowEntry sh; sh.e0 = make_float4(0, 0, 0, 0); sh.e1 = sh.e0; sh.e2 = sh.e0;

    if (alive) {
        v.id = info.x; v.pixel = info.y; v.k = info.z; v.state = info.w;
        bool newRay; uint32_t nv = 0;
        const LGlobal acc{ L, P, slot };
        if (shadeVertex<MM, STRICT, FEAT | SHADE_FEAT_NO_DIFFERENTIALS>(S, tab.T, tab.materials, rc, v, acc, newRay, pushShadow, sh, nv)) {
            vertices = nv; done = 1;
            needNew = true;
        } else {
            info.w = v.state;
            P.state[slot] = info.w;
        }
        if (newRay) {
            if (S.preclip) preclipRay(S, v.rayO, v.rayD);
            P.rayO[slot] = v.rayO; P.rayD[slot] = v.rayD; P.thr[slot] = v.thr; P.mis[slot] = v.mis;
        }
    }

    shadeEpilogueRays(src, S, P, rc, waveCnt, slot, inRange, info, alive, needNew, pushShadow, sh.e0, sh.e1, sh.e2, vertices, done, blockIdx.x, nullptr);
}

#ifdef SHADE_R_OUT_KERNEL        /* (a plain kernel, not a template: defined in the one object that asks for it -- phip_shade_r.hip, feature set 0, part 0) */
/* One lane per ray: the float64 sum of the ray's sppPass entries of L in ascending k, on top of what the earlier passes of the call left in acc (first = 0), and
   -- in the last pass -- the mean over the call's spp samples, rounded once to float32: one 16-byte store.  A sample the film would reject (non-finite or negative,
   imageblock.h:124-138) is counted and adds nothing.  acc: two double2 per ray, the scene's; NULL for a call of one pass. */
__global__ __launch_bounds__(BLOCK) void k_radiance_out(const float4 *L, double2 *acc, uint32_t n, uint32_t sppPass, uint32_t spp, uint32_t first, uint32_t last, float4 *out,
                                                        unsigned long long *invalidCount) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long invalid = 0;
    if (i < n) {
        double2 a = make_double2(0.0, 0.0), b = a;
        if (!first) { a = acc[2 * (size_t) i]; b = acc[2 * (size_t) i + 1]; }
        const float4 *l = L + (size_t) i * sppPass;
        for (uint32_t k = 0; k < sppPass; ++k) {
            const float4 v = l[k];
            if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w)) || v.x < 0 || v.y < 0 || v.z < 0 || v.w < 0) { ++invalid; continue; }
            a.x += (double) v.x; a.y += (double) v.y; b.x += (double) v.z; b.y += (double) v.w;
        }
        if (last) {
            const double s = (double) spp;
            out[i] = make_float4((float) (a.x / s), (float) (a.y / s), (float) (b.x / s), (float) (b.y / s));
        } else {
            acc[2 * (size_t) i] = a; acc[2 * (size_t) i + 1] = b;
        }
    }
    for (int off = 32; off > 0; off >>= 1) invalid += __shfl_down(invalid, off);
    if (__lane_id() == 0 && invalid) atomicAdd(invalidCount, invalid);
}
#endif

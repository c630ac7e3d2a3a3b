/*
 * k_traverse.h -- the LDS-resident scenes: the block's staged Wald records (stageRecords), the packed leaf table with the Wald tests dealt
 * over the wave (traverseFlat2W).  Included by phip.hip, phip_mega.hip and phip_shade.hip; see the header of phip.hip.
 */

/* ======================================================================================
 *  BVH traversal (closest / any hit)
 * ====================================================================================== */
struct TravResult { float t, u, v; uint32_t prim; uint32_t cls = 0; /* shade class of the record hit (k_rays_w only: k_pool.h) */ };

/* LDS pointers carry their address space in the type: through a generic pointer the compiler emits flat_load for the cached
   records, which goes through the texture addresser (16 clk per 16-byte wave instruction, shared by the CU's four SIMDs)
   instead of the LDS pipe (ds_read_b128) -- on the Cornell box, where everything is cached, that was the bottleneck. */
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef float f4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) f4v lds_cf4;
__device__ __forceinline__ float4 ldsLoad4(lds_cf4 *p) { const f4v v = *p; return make_float4(v.x, v.y, v.z, v.w); }

/* k_mega<MM_ALL>: the region [0, 12 KB) of the dynamic LDS (DevScene::dealDwords; phip.hip sizes it) --
   the four waves' work lists (6 KB), then the S-box of the mailboxes */
#define MEGA_DEAL_DWORDS 12u
/* bytes of dynamic LDS up to the end of the records stageRecords() stages; k_mega appends its shading tables (megaLdsBytesOf) */
__host__ __device__ __forceinline__ size_t recordsLdsEndOf(const DevScene &S) {
    return (size_t) S.dealDwords * BLOCK * sizeof(uint32_t) + (size_t) S.triCache * 3 * sizeof(float4);
}
__host__ __device__ __forceinline__ size_t megaLdsBytesOf(const DevScene &S) {
    return recordsLdsEndOf(S) + (size_t) S.nTriangles * TRISHADE_FLOAT4S * sizeof(float4) + (size_t) ((S.emitterTabSize + 3u) & ~3u) * sizeof(float)
         + (size_t) S.nMaterials * sizeof(DevMaterial) + 16 /* alignment of the next array */ + (size_t) S.nFlatLeaves * 2 * sizeof(float4);
}

/* k_shade_trace (k_shade_trace.h), dynamic LDS of a block: the packed leaf table, the Wald records, the emitter table and the materials -- sized for THIS scene (the static 8.5 KB of k_shade's
   two tables would cost a block of occupancy; the work lists of the dealt traversals live in the static exchange buffer) */
__host__ __device__ __forceinline__ size_t shadeTraceLdsBytes(const DevScene &S) {
    return (size_t) S.nFlatLeaves * 2 * sizeof(float4) + (size_t) S.triCache * 3 * sizeof(float4) + (size_t) ((S.emitterTabSize + 3u) & ~3u) * sizeof(float)
         + (size_t) S.nMaterials * sizeof(DevMaterial);
}

/* k_mega on the packed table: stage the scene's Wald records behind the deal / mailbox region at the front of the block's dynamic LDS and return the copy
   (all threads of the block must call: barrier inside).  k_mega takes the same address BEFORE the call instead of the result: a pointer that is live out of the
   staging costs k_mega<MM_ALL, strict, .., QMC> two more dwords of scratch (120 B against the 112 of tests/test_kernel_resources.py) */
__device__ __forceinline__ lds_cf4 *stageRecords(const DevScene &S, unsigned char *smem) {
    float4 *lt = (float4 *) (smem + (size_t) S.dealDwords * BLOCK * sizeof(uint32_t));
    for (uint32_t i = threadIdx.x; i < S.triCache * 3u; i += BLOCK)
        lt[i] = S.tris[i];
    __syncthreads();
    return (lds_cf4 *) lt;
}

#define SPILL_DEPTH 96


/* The packed leaf table of trees of at most 64 Wald records (the Cornell box: 32 triangles in 17 leaves): no walk at all.
 *   pass 1, uniform: every lane tests the SAME leaf box per step (the table entry is one LDS broadcast) and collects a bit mask of the RECORDS of the
 *           leaves its ray enters; the entries four at a time (eight LDS broadcasts in flight instead of a wait per leaf), the rest one by one;
 *   pass 2: the Wald tests of the records in the masks (traverseFlat2W below) -- no leaf reference to fetch and decode between records, a record
 *           referenced by two leaves is tested once.  The Wald test is branch-free here (waldIntersectSel: the axis permutation as twelve selects
 *           instead of three divergent branches).
 * Same arithmetic on the same operands as the walk of the tree, so (t, u, v, prim) are the same bits; records in index order instead of leaf order: winsTie. */
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bool waldIntersectSel(const float4 &a, const float4 &b, const float4 &c, const V3 &o, const V3 &d,
                                                 float mint, float maxt, float &u, float &v, float &t) {
    const uint32_t k = pm_to_bits(a.x);
    const bool k0 = k == 0, k2 = k == 2;                       /* k == 1: the default of the selects; k == 3 (degenerate record) fails below */
    const float o_u = k0 ? o.y : (k2 ? o.x : o.z), o_v = k0 ? o.z : (k2 ? o.y : o.x), o_k = k0 ? o.x : (k2 ? o.z : o.y);
    const float d_u = k0 ? d.y : (k2 ? d.x : d.z), d_v = k0 ? d.z : (k2 ? d.y : d.x), d_k = k0 ? d.x : (k2 ? d.z : d.y);
    const float n_u = a.y, n_v = a.z, n_d = a.w;
    t = (n_d - o_u * n_u - o_v * n_v - o_k) / (d_u * n_u + d_v * n_v + d_k);
    const float hu = o_u + t * d_u - b.x;
    const float hv = o_v + t * d_v - b.y;
    u = hv * b.z + hu * b.w;
    v = hu * c.x + hv * c.y;
    /* waldIntersect: `if (t < mint || t > maxt) return false; ... return u >= 0 && v >= 0 && u + v <= 1` (a NaN t fails through u) */
    return (k < 3u) & !(t < mint) & !(t > maxt) & (u >= 0) & (v >= 0) & (u + v <= 1.0f);
}


/* Pass 1 of the packed flat table (DevScene::flatMode 2 / 3): the bit mask of the Wald records whose leaf box the ray enters.  The table's form is shared
 * with the host code that packs it (phip.hip): entry = (c.x, c.y, c.z, 0) (h.x, h.y, h.z, bits(records)), centre and half extent: with
 * c' = c * rcp - o * rcp the slab distances of an axis are c' -+ h * |rcp| -- ALREADY ordered, one v_pk_fma_f32 whose source modifiers negate h for the
 * low half and replicate h, |rcp| and c' into both halves (inline assembly: the compiler does not form them) -- 11.3 VALU per box, against 15.3 for a
 * table of planes whose pairs are ordered with a min and a max (HISTORY.md).  The test only has to be conservative, and the host pads h for it (phip.hip). */
/* R64 (DevScene::flatMode 3, trees of 33..64 Wald records): the record mask has a second word, kept in the centre's spare word (A.w) */
template <bool R64 = false>
__device__ __forceinline__ uint32_t flat2Pass1(lds_cf4 *flat, uint32_t nFlat, const V3 &o, const V3 &rcp, float mint, float maxt, uint32_t *maskHi = nullptr) {
    uint32_t mask = 0, hi = 0;
    const f2v rxy = { rcp.x, rcp.y }, oxy = { -(o.x * rcp.x), -(o.y * rcp.y) };
    const f2v rz2 = { rcp.z, 0.0f }, oz2 = { -(o.z * rcp.z), 0.0f };
    f2v axy = { fabsf(rcp.x), fabsf(rcp.y) }, az2 = { fabsf(rcp.z), 0.0f };
    asm("" : "+v"(axy), "+v"(az2));                   /* (opaque: otherwise the two v_and are rematerialised inside the loop) */
    /* the orderings in assembly as well: on values that come out of inline assembly fmaxf / fminf first canonicalise every operand (v_max_f32 x, x, x) */
#define FLAT2_BOX(c_)                                                                                                                  \
        {                                                                                                                              \
            const f4v A = flat[2 * (c_)], B = flat[2 * (c_) + 1];                                                                      \
            const f2v cxy = __builtin_elementwise_fma(A.xy, rxy, oxy), cz = __builtin_elementwise_fma(A.zw, rz2, oz2);                 \
            f2v tx, ty, tz;                           /* (near, far) = (c' - h |r|, c' + h |r|) */                                      \
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,0,0] neg_lo:[1,0,0]" : "=v"(tx) : "v"(B.xy), "v"(axy), "v"(cxy));            \
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,1] op_sel_hi:[1,1,1] neg_lo:[1,0,0]" : "=v"(ty) : "v"(B.xy), "v"(axy), "v"(cxy)); \
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,0,0] neg_lo:[1,0,0]" : "=v"(tz) : "v"(B.zw), "v"(az2), "v"(cz));             \
            float tn, tf;                                                                                                              \
            asm("v_max3_f32 %0, %1, %2, %3" : "=v"(tn) : "v"(tx.x), "v"(ty.x), "v"(mint));                                              \
            asm("v_max_f32 %0, %1, %2" : "=v"(tn) : "v"(tn), "v"(tz.x));                                                               \
            asm("v_min3_f32 %0, %1, %2, %3" : "=v"(tf) : "v"(tx.y), "v"(ty.y), "v"(maxt));                                              \
            asm("v_min_f32 %0, %1, %2" : "=v"(tf) : "v"(tf), "v"(tz.y));                                                               \
            mask |= (tn <= tf) ? pm_to_bits(B.w) : 0u;                                                                                 \
            if (R64) hi |= (tn <= tf) ? pm_to_bits(A.w) : 0u;                                                                          \
        }
    /* groups of four entries (eight LDS broadcasts in flight), then the rest one by one: the Cornell box has 17 leaves -- padded to 20 it paid for three
       boxes no ray can enter, 15 % of a pass that is a third of the traversal */
    const uint32_t nFlat4 = nFlat & ~3u;
    for (uint32_t c4 = 0; c4 < nFlat4; c4 += 4) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) FLAT2_BOX(c4 + j)
    }
    for (uint32_t c = nFlat4; c < nFlat; ++c) FLAT2_BOX(c)
#undef FLAT2_BOX
    if (R64) *maskHi = hi;
    return mask;
}


/* Pass 2 DEALT OVER THE WAVE.  A per-lane loop `while (mask) test record ffs(mask)` runs for the wave's slowest lane -- about
 * eight Wald tests where the average ray needs 3.1, and in the shadow phase 30 of 64 lanes have no ray at all.  Here the (ray, record) pairs
 * of the whole wave are written to a work list in LDS and every lane tests one pair per step, whoever the ray belongs to:
 *   1. a prefix sum of popcount(mask) over the wave (six DPP steps) gives every lane its segment of the list; it writes (lane << 5 | record)
 *      per set bit -- a loop of the slowest lane's length, but of seven instructions, not seventy;
 *   2. ceil(pairs / 64) steps: entry -> the owner's ray through ds_bpermute (eight dwords), the record from LDS, the same Wald test on the
 *      same operands, against the owner's ORIGINAL interval (the sequential loop's shrinking maxt only rejects candidates that lose anyway);
 *      closest hit: LDS min of (bits(t) << 32 | (0x7FFFFFF - prim) << 5 | record) on the owner's slot -- the smallest t, at equal t the
 *      highest triangle index: winsTie, independent of the order; shadow ray: LDS min of the record index (the sequential loop stops at the
 *      first hit in index order: the work counter stays what it was);
 *   3. the owner reads its slot and repeats the winning test with its own registers for (t, u, v): same operands, same bits.
 * A work list of BAL_CAP pairs; a wave with more (never seen on the Cornell box: 64 x 3.1) goes round again with the lanes that did not fit.
 * Every lane of the wave must call, converged; `go` = this lane has a ray.  The buffers lie at the front of the dynamic LDS (DevScene::dealDwords). */
#define BAL_CAP 512u
#ifndef BAL_ILP
#define BAL_ILP 1                        /* pairs per lane and step of the test loop (BAL_CAP is a multiple of 64 * BAL_ILP).  Measured: 1 / 2 / 4 = 53.0 / 56.0 / 59.8 ms
                                            per C2 frame (profiles/r04_gpu_call_m_*): the list's tail is rounded up to whole steps, and wider steps waste more tests than their
                                            interleaving hides */
#endif
#define BAL_WAVE_BYTES (64u * 8u + BAL_CAP * 2u)                          /* slots, work list */
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
struct WaveBalance { lds_u64 *slot; lds_u16 *list; };
__device__ __forceinline__ WaveBalance waveBalanceAt(unsigned char *smem, uint32_t waveInBlock) {
    unsigned char *p = smem + waveInBlock * BAL_WAVE_BYTES;
    WaveBalance wb; wb.slot = (lds_u64 *) p; wb.list = (lds_u16 *) (p + 64u * 8u);
    return wb;
}
#define BAL_SYNC() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }    /* DS operations of a wave execute in order: this only pins the compiler's order */

/* R64: up to 64 records (a two-word mask; list entry = lane << 6 | record, key = ... (0x3FFFFFF - prim) << 6 | record) -- round 5: a scene of 33..64 records
   (a Cornell box with a third block) used to leave the dealt traversal for the per-lane leaf table */
template <bool R64> struct RecMask;
template <> struct RecMask<false> { typedef uint32_t T; static __device__ __forceinline__ uint32_t popc(T m) { return (uint32_t) __popc(m); }
                                    static __device__ __forceinline__ uint32_t ctz(T m) { return (uint32_t) __builtin_ctz(m); }
                                    static __device__ __forceinline__ T upTo(uint32_t i) { return (2u << i) - 1u; } };
template <> struct RecMask<true>  { typedef unsigned long long T; static __device__ __forceinline__ uint32_t popc(T m) { return (uint32_t) __popcll(m); }
                                    static __device__ __forceinline__ uint32_t ctz(T m) { return (uint32_t) __builtin_ctzll(m); }
                                    static __device__ __forceinline__ T upTo(uint32_t i) { return i >= 63u ? ~0ull : (2ull << i) - 1ull; } };
template <bool SHADOW, bool R64 = false>
__device__ __forceinline__ bool traverseFlat2W(lds_cf4 *flat, uint32_t nFlat, lds_cf4 *tris, const WaveBalance &wb, uint32_t lane, bool go,
                                               const V3 &o, const V3 &d, const V3 &rcp, float mint, float maxt, TravResult &res, uint32_t &nodeVisits, uint32_t &triTests) {
    typedef RecMask<R64> RM; typedef typename RM::T Mask;
    constexpr uint32_t RB = R64 ? 6u : 5u, RMSK = (1u << RB) - 1u;     /* bits of a record index */
    uint32_t maskHi = 0;
    const uint32_t maskLo = flat2Pass1<R64>(flat, nFlat, o, rcp, mint, maxt, &maskHi);
    Mask mask = R64 ? (Mask) (((unsigned long long) maskHi << 32) | maskLo) : (Mask) maskLo;
    mask = go ? mask : (Mask) 0;                                 /* (a lane without a ray ran pass 1 on whatever its registers held) */
    nodeVisits += go ? 1u : 0u;
    const Mask mask0 = mask;

    if (SHADOW) *(lds_u32 *) (wb.slot + lane) = 0xFFFFFFFFu; else wb.slot[lane] = ~0ull;
    while (__ballot(mask != 0)) {
        /* list segments in lane order: an inclusive scan of the pair counts over the wave (every lane is active here: plain DPP, the
           sequence the compiler itself emits for wave-aggregated atomics -- four shifts inside the rows of 16, then two row broadcasts) */
        const uint32_t pc = RM::popc(mask);
        uint32_t incl = pc;
        incl += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) incl, 0x111 /* row_shr:1 */, 0xf, 0xf, true);
        incl += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) incl, 0x112 /* row_shr:2 */, 0xf, 0xf, true);
        incl += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) incl, 0x114 /* row_shr:4 */, 0xf, 0xf, true);
        incl += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) incl, 0x118 /* row_shr:8 */, 0xf, 0xf, true);
        incl += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) incl, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
        incl += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) incl, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
        /* the lanes whose segment ends inside the list (a prefix of the wave, never empty: a lane has at most 64 pairs) write it and are done */
        const bool fits = incl <= BAL_CAP;
        const uint32_t nFit = (uint32_t) __popcll(__ballot(fits));
        const uint32_t total = (uint32_t) __builtin_amdgcn_readlane((int) incl, (int) (nFit - 1u));
        if (pc && fits) {
            const uint32_t tag = lane << RB;
            lds_u16 *w = wb.list + (incl - pc);
            do {
                *w++ = (uint16_t) (tag | RM::ctz(mask));
                mask &= mask - 1u;
            } while (mask);
        }
        BAL_SYNC()
        /* one pair per lane and step (BAL_ILP of them interleaved measured slower, see above) */
        for (uint32_t base = 0; base < total; base += 64u * BAL_ILP) {
            bool hit[BAL_ILP]; uint32_t own[BAL_ILP], lo[BAL_ILP], hi[BAL_ILP];
#pragma unroll
            for (uint32_t j = 0; j < BAL_ILP; ++j) {             /* the tests, free of control flow so that the compiler interleaves them ... */
                const uint32_t i = base + 64u * j + lane;
                const uint32_t item = wb.list[i];                /* (entries behind `total` hold stale pairs: tested, not committed) */
                const uint32_t owner = (item >> RB) & 63u, rec = item & RMSK;
                const int src = (int) (owner << 2);
                const V3 po(pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(o.x))), pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(o.y))),
                            pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(o.z))));
                const V3 pd(pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(d.x))), pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(d.y))),
                            pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(d.z))));
                const float pmint = pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(mint)));
                const float pmaxt = pm_from_bits((uint32_t) __builtin_amdgcn_ds_bpermute(src, (int) pm_to_bits(maxt)));
                lds_cf4 *t_ = tris + 3 * rec;
                const float4 a = ldsLoad4(t_), b = ldsLoad4(t_ + 1), c = ldsLoad4(t_ + 2);
                float tu, tv, tt;
                hit[j] = (i < total) & waldIntersectSel(a, b, c, po, pd, pmint, pmaxt, tu, tv, tt);
                own[j] = owner; hi[j] = pm_to_bits(tt);
                lo[j] = SHADOW ? rec : ((((0xFFFFFFFFu >> RB) - pm_to_bits(c.z)) << RB) | rec);
            }
#pragma unroll
            for (uint32_t j = 0; j < BAL_ILP; ++j)               /* ... then the commits */
                if (hit[j]) {
                    if (SHADOW) __hip_atomic_fetch_min((lds_u32 *) (wb.slot + own[j]), lo[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else __hip_atomic_fetch_min(wb.slot + own[j], ((unsigned long long) hi[j] << 32) | (unsigned long long) lo[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
        }
        BAL_SYNC()
    }
    res.prim = PHIP_NO_HIT; res.t = INFINITY; res.u = res.v = 0;
    if (SHADOW) {
        const uint32_t first = *(lds_u32 *) (wb.slot + lane);
        const bool found = first != 0xFFFFFFFFu;
        triTests += RM::popc(found ? (Mask) (mask0 & RM::upTo(first & RMSK)) : mask0);
        return found;
    } else {
        const unsigned long long best = wb.slot[lane];
        const bool found = best != ~0ull;
        triTests += RM::popc(mask0);
        lds_cf4 *t_ = tris + 3 * ((uint32_t) best & RMSK);
        const float4 a = ldsLoad4(t_), b = ldsLoad4(t_ + 1), c = ldsLoad4(t_ + 2);
        /* t is the key's high word (the tester's quotient, bit for bit); (u, v) follow from it as in the Wald test -- no division, no o_k / d_k selects */
        const float tt = pm_from_bits((uint32_t) (best >> 32));
        const uint32_t k = pm_to_bits(a.x);
        const bool k0 = k == 0, k2 = k == 2;
        const float o_u = k0 ? o.y : (k2 ? o.x : o.z), o_v = k0 ? o.z : (k2 ? o.y : o.x);
        const float d_u = k0 ? d.y : (k2 ? d.x : d.z), d_v = k0 ? d.z : (k2 ? d.y : d.x);
        const float hu = o_u + tt * d_u - b.x, hv = o_v + tt * d_v - b.y;
        const float tu = hv * b.z + hu * b.w, tv = hu * c.x + hv * c.y;
        res.t = found ? tt : res.t; res.u = found ? tu : res.u; res.v = found ? tv : res.v; res.prim = found ? pm_to_bits(c.z) : res.prim;
        res.cls = found ? (pm_to_bits(c.w) & 3u) : 0u;           /* the record's shade class (k_shade_trace passes it on in the hit word: k_pool.h) */
        return found;
    }
}

/* the block's dynamic LDS (k_mega.h has the map) */
extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];

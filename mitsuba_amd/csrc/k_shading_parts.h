/*
 * k_shading_parts.h -- phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device (phip_shading_parts.hip): what an integrator does between two ray
 * casts, as kernels over a caller's arrays in device memory.  Each kernel gives one lane one item and evaluates ONE statement per item -- bsdfPartsItem,
 * emitterSampleItem, emitterEvalItem below, __host__ __device__ like the functions of dv_scene.h they call -- which the debug library's host twins evaluate on the
 * host-side DevScene (phip_debug.inl).  Nothing of shadeVertex is restated: the items call fillIntersection, bsdfResolve, bsdfTextures, bsdfEvalPdf<MM_ALL>,
 * bsdfSample<MM_ALL>, sampleEmitterDirect<ENV>, pdfEmitterDirectDot<ENV>, envFillDirectRecord and envmapEval in the order the vertex calls them, and the unit is built
 * with the product's flags, so a value equals the one the vertex computes from the same inputs, bit for bit.
 * Inputs are read and outputs written as whole 16-byte words (2-float arrays as 8-byte words), as k_surfaces does.
 * Included by phip_shading_parts.hip (the kernels) and by phip.hip (the items, for the host twins: the kernels are templates that unit does not instantiate).
 */
#pragma once

/* ---- phip_bsdf_device ---- */
struct BsdfPartsOut { float4 eval; float4 s0, s1, s2; float4 wi; };

/* The BSDF at a hit (t, u, v, prim) of a ray of direction rayD: eval + pdf of `wo`, a sample from `smp`, wi in the shading frame.  A miss -- and a primitive index
   the scene does not have -- is all zero.  Textured parameters are read as a later path vertex reads them (no UV partials: level 0); on a mesh without texture
   coordinates the texture coordinates are the hit's (u, v) (skdtree.h:404), as in phip_surface.  `local`: wo is given, and the sampled direction returned, in the
   shading frame. */
template <bool EVAL, bool SAMPLE>
DV void bsdfPartsItem(const DevScene &S, const DevMaterial *materials, const V3 &rayD, const float4 &h, const V3 &woIn, const V2 &smp, bool local, BsdfPartsOut &o) {
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o.eval = zero; o.s0 = zero; o.s1 = zero; o.s2 = zero; o.wi = zero;
    const uint32_t prim = pm_to_bits(h.w);
    if (prim >= S.nTriangles) return;                            /* PHIP_NO_HIT included */
    Isect its;
    its.uv = V2(h.y, h.z);
    fillIntersection(S, rayD, prim, h.y, h.z, h.x, its);
    o.wi = make_float4(its.wi.x, its.wi.y, its.wi.z, 0.0f);
    if (!EVAL && !SAMPLE) return;
    BsdfCtx bctx = bsdfResolve(materials, its);
    if (bctx.textured) bsdfTextures(S, bctx, its.uv, false, 0.0f, 0.0f, 0.0f, 0.0f);
    if (EVAL) {
        const V3 wo = local ? woIn : its.sh.toLocal(woIn);
        float pdf;
        const V3 value = bsdfEvalPdf<MM_ALL>(bctx, wo, pdf);
        o.eval = make_float4(value.x, value.y, value.z, pdf);
    }
    if (SAMPLE) {
        BSDFSample bs;
        const V3 weight = bsdfSample<MM_ALL>(bctx, smp, bs);
        if (!weight.isZero()) {
            const V3 wo = local ? bs.wo : its.sh.toWorld(bs.wo);
            o.s0 = make_float4(wo.x, wo.y, wo.z, bs.pdf);
            o.s1 = make_float4(weight.x, weight.y, weight.z, bs.eta);
            o.s2 = make_float4(pm_from_bits(PHIP_BSDF_SAMPLED_VALID | (bs.delta ? PHIP_BSDF_SAMPLED_DELTA : 0u)), 0.0f, 0.0f, 0.0f);
        }
    }
}

/* ---- phip_emitter_sample_device ---- */
struct EmitterSampleOut { float4 s0, s1, s2; float4 ro, rd; };

/* Scene::sampleEmitterDirect(dRec, sample, testVisibility = false) from the reference point `ref` with normal `refN` (zero: a point on no surface), and the shadow
   ray the `path` integrator traces for the sample (k_shade.h: the entry it queues, k_clip.h: the mint it is traced with).  No sample: emitter -1, everything else
   zero, and the empty interval as shadow ray. */
template <bool ENV>
DV void emitterSampleItem(const DevScene &S, const EmitterTab &T, const V3 &ref, const V3 &refN, const V2 &smp, EmitterSampleOut &o) {
    DirectRec dRec;
    dRec.ref = ref; dRec.refN = refN;
    dRec.pdf = 0; dRec.emitter = -1;
    const V3 value = sampleEmitterDirect<ENV>(S, T, dRec, smp);
    if (dRec.pdf == 0) {
        o.s0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); o.s1 = o.s0;
        o.s2 = make_float4(pm_from_bits(0xFFFFFFFFu), 0.0f, 0.0f, 0.0f);
        o.ro = make_float4(ref.x, ref.y, ref.z, 0.0f); o.rd = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        return;
    }
    o.s0 = make_float4(dRec.d.x, dRec.d.y, dRec.d.z, dRec.dist);
    o.s1 = make_float4(value.x, value.y, value.z, dRec.pdf);
    o.s2 = make_float4(pm_from_bits((uint32_t) dRec.emitter), 0.0f, 0.0f, 0.0f);
    o.ro = make_float4(ref.x, ref.y, ref.z, PT_EPSILON);
    o.rd = make_float4(dRec.d.x, dRec.d.y, dRec.d.z, dRec.dist * (1 - PT_SHADOW_EPSILON));
}

/* ---- phip_emitter_eval_device ---- */
/* The emitted radiance a ray (rayO, rayD) meets at its hit `h` and the density with which emitter sampling from the ray's origin -- normal refN -- would have
   produced that direction: the block of path.cpp behind bsdf->sample (shadeVertex: "tail of the previous loop iteration" and the environment branch of a miss).
   On an area emitter Intersection::Le(-d) and pdfEmitterDirect of DirectSamplingRecord::setQuery; at a miss under an environment emitter evalEnvironment of a
   ray without differentials, with the density where the emitter's fillDirectSamplingRecord accepts the ray (the origin lies inside its sphere) and 0 where not;
   otherwise zero and emitter -1. */
template <bool ENV>
DV void emitterEvalItem(const DevScene &S, const EmitterTab &T, const V3 &rayO, const V3 &rayD, const float4 &h, const V3 &refN, float4 &eval, int32_t &emitter) {
    eval = make_float4(0.0f, 0.0f, 0.0f, 0.0f); emitter = -1;
    const uint32_t prim = pm_to_bits(h.w);
    const float dDotRefN = dot(rayD, refN);
    const bool refNZero = refN.isZero();
    if (prim == PHIP_NO_HIT) {
        if (ENV && S.envEmitter >= 0) {
            const float *em = emitterRecord(T, (uint32_t) S.envEmitter);
            const V3 value = (pm_to_bits(em[EM_TYPE]) == PHIP_EMITTER_ENVMAP) ? envmapEval(S.env, rayD) : rgb(em + EM_RADIANCE);
            float pdf = 0.0f;
            if (envFillDirectRecord(S, rayO, rayD))
                pdf = pdfEmitterDirectDot<ENV>(S, T, (uint32_t) S.envEmitter, rayD, dDotRefN, refNZero, 0.0f, 0.0f);
            eval = make_float4(value.x, value.y, value.z, pdf); emitter = S.envEmitter;
        }
        return;
    }
    if (prim >= S.nTriangles) return;
    Isect its;
    fillIntersection(S, rayD, prim, h.y, h.z, h.x, its);
    if (its.emitter < 0 || (uint32_t) its.emitter >= T.n) return;
    const float *em = emitterRecord(T, (uint32_t) its.emitter);
    const V3 value = (dot(its.sh.n, -rayD) <= 0) ? V3(0.0f) : rgb(em + EM_RADIANCE);
    const float pdf = pdfEmitterDirectDot<ENV>(S, T, (uint32_t) its.emitter, rayD, dDotRefN, refNZero, dot(rayD, its.sh.n), its.t);
    eval = make_float4(value.x, value.y, value.z, pdf); emitter = its.emitter;
}

#if defined(__HIPCC__) && defined(PHIP_SHADING_PARTS_KERNELS)
/* one lane per hit.  Whether the BSDF is evaluated and / or sampled are template arguments: an eval-only call carries no sampling code (the Beckmann visible-normal
   sampler is the longest branch of the vertex) and a call for wi alone no BSDF at all; outWi may be NULL in every build.  The one material record of the lane comes from memory, as in k_shade where the materials do not fit
   LDS: a block has no second item per lane to amortise a staging round trip over. */
template <bool EVAL, bool SAMPLE>
__global__ __launch_bounds__(BLOCK) void k_bsdf_parts(DevScene S, const float4 *rays, const float4 *hits, const float4 *wo, const float2 *samples, uint32_t n, uint32_t local,
                                                      float4 *outEval, float4 *outSampled, float4 *outWi) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 h = hits[i], rd = rays[2 * (size_t) i + 1];
    V3 woIn(0.0f); V2 smp(0.0f, 0.0f);
    if (EVAL) { const float4 w = wo[i]; woIn = V3(w.x, w.y, w.z); }
    if (SAMPLE) { const float2 s = samples[i]; smp = V2(s.x, s.y); }
    BsdfPartsOut o;
    bsdfPartsItem<EVAL, SAMPLE>(S, S.materials, V3(rd.x, rd.y, rd.z), h, woIn, smp, local != 0u, o);
    if (EVAL) outEval[i] = o.eval;
    if (SAMPLE) { float4 *s = outSampled + 3 * (size_t) i; s[0] = o.s0; s[1] = o.s1; s[2] = o.s2; }
    if (outWi) outWi[i] = o.wi;
}

/* The emitter table of a block: staged in LDS where k_shade stages it (at most EMITTER_LDS_FLOATS floats; stageShadeTables, k_shade.h) -- the sample walks selection
   CDF -> emitter record -> area CDF -> triangle record, four dependent look-ups per lane that one coalesced round trip at the head of the block turns into LDS reads --
   and read from memory beyond.  All threads of the block call; the caller places the barrier. */
__device__ __forceinline__ EmitterTab stageEmitterTable(const DevScene &S, float *ldsEm) { return stageShadeTables<false>(S, ldsEm, nullptr).T; }

/* one lane per reference point */
template <bool ENV>
__global__ __launch_bounds__(BLOCK) void k_emitter_sample(DevScene S, const float4 *ref, const float4 *refN, const float2 *samples, uint32_t n, float4 *outSampled, float4 *outShadowRays) {
    __shared__ __align__(16) float ldsEm[EMITTER_LDS_FLOATS];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t li = i < n ? i : 0u;                          /* (n > 0: the host launches nothing for an empty call) */
    const float4 p = ref[li];
    const float2 s = samples[li];
    float4 rn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (refN) rn = refN[li];
    const EmitterTab T = stageEmitterTable(S, ldsEm);
    __syncthreads();
    if (i >= n) return;
    EmitterSampleOut o;
    emitterSampleItem<ENV>(S, T, V3(p.x, p.y, p.z), V3(rn.x, rn.y, rn.z), V2(s.x, s.y), o);
    float4 *d = outSampled + 3 * (size_t) i;
    d[0] = o.s0; d[1] = o.s1; d[2] = o.s2;
    if (outShadowRays) { outShadowRays[2 * (size_t) i] = o.ro; outShadowRays[2 * (size_t) i + 1] = o.rd; }
}

/* one lane per ray */
template <bool ENV>
__global__ __launch_bounds__(BLOCK) void k_emitter_eval(DevScene S, const float4 *rays, const float4 *hits, const float4 *refN, uint32_t n, float4 *outEval, int32_t *outEmitter) {
    __shared__ __align__(16) float ldsEm[EMITTER_LDS_FLOATS];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t li = i < n ? i : 0u;
    const float4 ro = rays[2 * (size_t) li], rd = rays[2 * (size_t) li + 1], h = hits[li];
    float4 rn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (refN) rn = refN[li];
    const EmitterTab T = stageEmitterTable(S, ldsEm);
    __syncthreads();
    if (i >= n) return;
    float4 e; int32_t emitter;
    emitterEvalItem<ENV>(S, T, V3(ro.x, ro.y, ro.z), V3(rd.x, rd.y, rd.z), h, V3(rn.x, rn.y, rn.z), e, emitter);
    outEval[i] = e;
    if (outEmitter) outEmitter[i] = emitter;
}
#endif

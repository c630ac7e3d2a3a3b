/*
 * phip_debug.inl -- unit-test entry points, compiled into libphip_debug.so only (-DPHIP_DEBUG_HOOKS=1; the product library does not carry them).
 *
 * The phip_debug_host_* functions execute the
 * __host__ __device__ shading functions of dv_math.h / dv_scene.h ON THE HOST so that
 * `-m "not gpu"` tests can compare the product's arithmetic with the oracle bit for bit
 * without a GPU.  They are never reachable from phip_render*: rendering has no CPU fallback.
 * The others need a device: the fmath probe, the HBM calibration kernels, and phip_debug_rccl_selftest (the RCCL calls of host_multi.h's merge).
 */
extern "C" {

int phip_debug_host_bsdf_sample(const phip_material *materials, uint32_t n_materials, uint32_t material, size_t n,
                                const float *wi3, const float *sample2, float *wo3, float *weight3, float *pdf, uint8_t *delta) {
    try {
        std::vector<DevMaterial> mats = convertMaterials(materials, n_materials);
        if (material >= n_materials) return setErr(PHIP_ERR_INVALID, "material id out of range");
        DevScene S; memset(&S, 0, sizeof(S)); S.materials = mats.data();
        for (size_t i = 0; i < n; ++i) {
            BSDFSample bs;
            V3 w = bsdfSample(S, mats[material], V3(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), V2(sample2[2 * i], sample2[2 * i + 1]), bs);
            if (w.isZero()) { bs.pdf = 0; bs.wo = V3(0.0f); }
            wo3[3 * i] = bs.wo.x; wo3[3 * i + 1] = bs.wo.y; wo3[3 * i + 2] = bs.wo.z;
            weight3[3 * i] = w.x; weight3[3 * i + 1] = w.y; weight3[3 * i + 2] = w.z;
            pdf[i] = bs.pdf; if (delta) delta[i] = bs.delta ? 1 : 0;
        }
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

int phip_debug_host_bsdf_eval_pdf(const phip_material *materials, uint32_t n_materials, uint32_t material, size_t n,
                                  const float *wi3, const float *wo3, float *value3, float *pdf) {
    try {
        std::vector<DevMaterial> mats = convertMaterials(materials, n_materials);
        if (material >= n_materials) return setErr(PHIP_ERR_INVALID, "material id out of range");
        DevScene S; memset(&S, 0, sizeof(S)); S.materials = mats.data();
        for (size_t i = 0; i < n; ++i) {
            V3 wi(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), wo(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);
            V3 v = bsdfEval(S, mats[material], wi, wo);
            value3[3 * i] = v.x; value3[3 * i + 1] = v.y; value3[3 * i + 2] = v.z;
            pdf[i] = bsdfPdf(S, mats[material], wi, wo);
        }
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

void phip_debug_host_camera_ray(const phip_camera *cam, const phip_film *film, float sx, float sy, phip_ray *out) {
    DevCamera dc; setupCamera(*cam, *film, dc);
    V3 o, d; float mint, maxt;
    cameraRay(dc, sx, sy, o, d, mint, maxt);
    out->o[0] = o.x; out->o[1] = o.y; out->o[2] = o.z; out->mint = mint;
    out->d[0] = d.x; out->d[1] = d.y; out->d[2] = d.z; out->maxt = maxt;
}

void phip_debug_host_ctr_block(uint32_t pixel, uint32_t sample, uint32_t block, uint32_t seed, float *out4) {
    const U4 h = pcg4d(pixel, sample, block, seed);
    out4[0] = u32ToFloat(h.x); out4[1] = u32ToFloat(h.y); out4[2] = u32ToFloat(h.z); out4[3] = u32ToFloat(h.w);
}

/* DiscreteDistribution::sample (pmf.h:124-136) as the kernels compile it (cdfSample, dv_scene.h: tables of one to three entries are counted, larger
   ones searched): index of each value; `cdf` holds n_entries + 1 values followed by at least three readable floats */
void phip_debug_host_cdf_sample(const float *cdf, uint32_t n_entries, const float *values, size_t n_values, uint32_t *out_index) {
    for (size_t i = 0; i < n_values; ++i) out_index[i] = cdfSample(cdf, n_entries, values[i]);
}

/* PHIP_SAMPLER_LD: the point of request `dim` (2D request q: 2 q; 1D request j: 2 j + 1) of sample `sample` of `pixel` -- the code the kernels compile */
void phip_debug_host_ld_point(uint32_t pixel, uint32_t sample, uint32_t dim, uint32_t seed, uint32_t mask, float *out2) {
    ldPoint(pixel, sample, dim, seed, mask, out2[0], out2[1]);
}

/* PHIP_SAMPLER_SOBOL on the host: index of sample `sample[i]` of pixel (px[i], py[i]) (SobolSampler::setSampleIndex) and its number in dimension dim[i], with the
   row loops of sobolseq.h (byte_tables = 0) or through the byte tables phip_render builds from the same direction numbers (byte_tables = 1: the device's path) --
   the code the kernels compile (dv_math.h) */
int phip_debug_host_sobol(const uint32_t *matrices, uint32_t dims, const unsigned long long *vdc, const unsigned long long *vdc_inv, uint32_t log_res, uint32_t scramble,
                          int byte_tables, size_t n, const uint32_t *sample, const uint32_t *px, const uint32_t *py, const uint32_t *dim,
                          unsigned long long *out_index, float *out_value, float *out_pair2x2 /* 4 n: dimensions dim, dim + 1, dim + 2, dim + 3 in one pass */) {
    std::vector<unsigned long long> rows(2 * PHIP_SOBOL_MATRIX_SIZE, 0ull);
    if (log_res > 1u) for (int i = 0; i < PHIP_SOBOL_MATRIX_SIZE; ++i) { rows[i] = vdc[i]; rows[PHIP_SOBOL_MATRIX_SIZE + i] = vdc_inv[i]; }
    std::vector<uint32_t> bt; std::vector<unsigned long long> vb;
    SobolTab T; memset(&T, 0, sizeof(T));
    T.matrices = matrices; T.vdc = (const uint64_t *) rows.data(); T.vdcInv = (const uint64_t *) rows.data() + PHIP_SOBOL_MATRIX_SIZE;
    T.dims = dims; T.logRes = log_res; T.scramble = scramble; T.resolution = (float) (1u << log_res);
    if (byte_tables) {
        buildSobolByteTables(matrices, dims, rows.data(), bt, vb);
        T.matBt = bt.data(); T.vdcBt = (const uint64_t *) vb.data(); T.vdcInvBt = (const uint64_t *) vb.data() + 4u * 256u;
    }
    for (size_t i = 0; i < n; ++i) {
        if (dim[i] + 5u >= dims) return setErr(PHIP_ERR_INVALID, "dimension out of range");      /* (an index above 2^52 reads on into the next dimension, as sobolseq.h does) */
        const uint64_t idx = sobolSampleIndex(T, sample[i], px[i], py[i]);
        out_index[i] = idx; out_value[i] = sobolSample(T, idx, dim[i]);
        if (out_pair2x2) sobolSample2x2(T, idx, dim[i], dim[i] + 2u, out_pair2x2 + 4 * i);
    }
    return PHIP_OK;
}

/* the radical inverses of PHIP_SAMPLER_HALTON / _HAMMERSLEY (dv_math.h: rinvRadicalInverse) on the host: digit by digit (tables = 0: the loops of qmc.cpp) or
   through the multi-digit tables the render uploads (buildRinvTables) -- tests/test_host_parity.py holds the two against each other and against numpy */
int phip_debug_host_rinv(const uint32_t *primes, const uint16_t *perm, uint32_t dims, int tables, size_t n, const unsigned long long *index, const uint32_t *dim, float *out) {
    std::vector<uint32_t> off(dims); size_t total = 0;
    for (uint32_t d = 0; d < dims; ++d) { off[d] = (uint32_t) total; total += primes[d]; }
    RinvTab T; memset(&T, 0, sizeof(T));
    T.primes = primes; T.perm = perm; T.permOffset = off.data(); T.dims = dims;
    std::vector<uint32_t> di, ch, pw; std::vector<float> fc;
    if (tables) { T.tabDims = buildRinvTables(primes, perm, off.data(), dims, di, ch, fc, pw); T.dimInfo = di.data(); T.chunk = ch.data(); T.fac = fc.data(); T.pw = pw.data(); }
    for (size_t i = 0; i < n; ++i) {
        if (dim[i] >= dims) return setErr(PHIP_ERR_INVALID, "dimension out of range");
        out[i] = rinvRadicalInverse(T, dim[i], index[i]);
    }
    return PHIP_OK;
}

/* ... and the interleaved form of a 2D request (rinvSample2: dimensions dim, dim + 1 in one pass; hammersley = 1: dimension d is the radical inverse in prime d - 1) */
int phip_debug_host_rinv2(const uint32_t *primes, const uint16_t *perm, uint32_t dims, int hammersley, size_t n, const unsigned long long *index, const uint32_t *dim, float *out2) {
    std::vector<uint32_t> off(dims); size_t total = 0;
    for (uint32_t d = 0; d < dims; ++d) { off[d] = (uint32_t) total; total += primes[d]; }
    RinvTab T; memset(&T, 0, sizeof(T));
    T.primes = primes; T.perm = perm; T.permOffset = off.data(); T.dims = dims; T.hammersley = hammersley ? 1u : 0u; T.factor = 1.0f;
    std::vector<uint32_t> di, ch, pw; std::vector<float> fc;
    T.tabDims = buildRinvTables(primes, perm, off.data(), dims, di, ch, fc, pw); T.dimInfo = di.data(); T.chunk = ch.data(); T.fac = fc.data(); T.pw = pw.data();
    for (size_t i = 0; i < n; ++i) {
        if (dim[i] < 1u || dim[i] + 1u >= dims) return setErr(PHIP_ERR_INVALID, "dimension out of range");
        rinvSample2(T, index[i], dim[i], out2[2 * i], out2[2 * i + 1]);
    }
    return PHIP_OK;
}

/* The kernel the product's selection resolves for a key -- the functions planFused and selectVertexKernel call (phip.hip: shadeKernelOf, shadeTraceWideKernelOf,
   megaKernelOf), not a copy of them -- by the name the dynamic symbol table has for its host pointer: the mangled name with the template arguments.  No HIP call, no GPU.
   family 0: k_shade / k_shade_direct (form = k_shade's table set), 1: k_shade_trace, 2: k_shade_trace_w, 3: k_mega (form = its traversal form).  NULL: nothing
   resolves for the key (a traversal form no build of k_mega holds), or the pointer has no dynamic symbol */
const char *phip_debug_selected_kernel(int family, int feat, int material_mask, int strict_normals, int form, int qmc, int direct) {
    const bool strict = strict_normals != 0;
    const void *k = family == 3 ? (const void *) megaKernelOf(direct != 0, form, material_mask, strict, qmc != 0)
                  : family == 2 ? (const void *) shadeTraceWideKernelOf(feat, strict, material_mask)
                                : (const void *) shadeKernelOf(feat, direct != 0, family == 1, strict, material_mask, form);
    Dl_info info;
    return k && dladdr(k, &info) && info.dli_saddr == k ? info.dli_sname : nullptr;
}

/* Wald records + BVH statistics of a triangle soup, built exactly like phip_scene_create does (no GPU needed) */
int phip_debug_host_build_bvh(const float *positions, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles,
                              phip_accel_info *info, float *scene_box6) {
    try {
        for (uint32_t i = 0; i < 3 * n_triangles; ++i) if (indices[i] >= n_vertices) return setErr(PHIP_ERR_INVALID, "index out of range");
        HostBVH bvh; buildBVH(positions, indices, n_triangles, bvh);
        if (info) {
            info->n_nodes = bvh.nWNodes; info->n_leaves = bvh.nLeaves; info->n_triangle_refs = bvh.nTriRefs; info->max_depth = bvh.wMaxDepth;
            info->node_bytes = 80; info->triangle_bytes = 48; info->sah_cost = bvh.wSahCost; info->build_ms = bvh.buildMs;
        }
        if (scene_box6) for (int a = 0; a < 3; ++a) { scene_box6[a] = bvh.sceneMin[a]; scene_box6[3 + a] = bvh.sceneMax[a]; }
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

} // extern "C"

/* the rays of the two hooks below through a wide tree on the host: scene-box clip, then the walk (use_wide) or every record in turn */
static void hostTraceRays(const float *sceneMin, const float *sceneMax, const float4 *recs, size_t nRecs, const uint4 *wn, uint32_t nWNodes, int use_wide,
                          const phip_ray *rays, size_t n_rays, phip_hit *hits, uint8_t *seq, uint32_t seq_stride) {
    for (size_t i = 0; i < n_rays; ++i) {
        const V3 o(rays[i].o[0], rays[i].o[1], rays[i].o[2]), d(rays[i].d[0], rays[i].d[1], rays[i].d[2]);
        phip_hit h; h.t = INFINITY; h.u = h.v = 0; h.prim = PHIP_NO_HIT;
        /* scene-box clip + adaptive epsilon, skdtree.cpp:112-142 (the host twin of clipToScene<false>) */
        float nearT = -INFINITY, farT = INFINITY; bool ok = true;
        const float oo[3] = { o.x, o.y, o.z }, dd[3] = { d.x, d.y, d.z };
        for (int a = 0; a < 3 && ok; ++a) {
            if (dd[a] == 0) { if (oo[a] < sceneMin[a] || oo[a] > sceneMax[a]) ok = false; }
            else {
                const float rcp = 1.0f / dd[a];
                float t1 = (sceneMin[a] - oo[a]) * rcp, t2 = (sceneMax[a] - oo[a]) * rcp;
                if (t1 > t2) std::swap(t1, t2);
                nearT = smax(t1, nearT); farT = smin(t2, farT);
                if (!(nearT <= farT)) ok = false;
            }
        }
        float mint = nearT, maxt = farT;
        if (ok) {
            float rayMinT = rays[i].mint;
            if (rayMinT == PT_EPSILON) rayMinT *= smax(smax(smax(fabsf(o.x), fabsf(o.y)), fabsf(o.z)), PT_EPSILON);
            if (rayMinT > mint) mint = rayMinT;
            if (rays[i].maxt < maxt) maxt = rays[i].maxt;
            ok = maxt > mint;
        }
        if (ok && !use_wide) {
            for (size_t k = 0; k < nRecs; ++k) {
                float tu, tv, tt;
                if (waldIntersect(recs[3 * k], recs[3 * k + 1], recs[3 * k + 2], o, d, mint, maxt, tu, tv, tt) && winsTie(tt, pm_to_bits(recs[3 * k + 2].z), h.t, h.prim)) { maxt = tt; h.t = tt; h.u = tu; h.v = tv; h.prim = pm_to_bits(recs[3 * k + 2].z); }
            }
        } else if (ok) {
            WideRay ray; wideRaySetup(ray, o, d, V3(slabRcp(d.x), slabRcp(d.y), slabRcp(d.z)), mint, maxt);
            std::vector<uint2> stack;
            uint32_t nSeq = 0;
            auto note = [&](uint8_t what) { if (seq && nSeq + 1 < seq_stride) seq[i * seq_stride + nSeq++] = what; };
            uint2 ng = make_uint2(0u, 0x80000000u), tg = make_uint2(0u, 0u);
            for (;;) {
                if (tg.y == 0u && (ng.y & 0xff000000u)) {
                    const uint32_t bit = 31u - (uint32_t) __builtin_clz(ng.y);
                    ng.y &= ~(1u << bit);
                    if (ng.y & 0xff000000u) stack.push_back(ng);
                    const uint32_t slot = (bit - 24u) ^ (ray.octinv4 & 7u);
                    const uint32_t idx = ng.x + (uint32_t) __builtin_popcount(ng.y & ((1u << slot) - 1u) & 0xffu);
                    if (idx >= nWNodes) throw std::runtime_error("wide BVH: child index out of range");
                    const uint4 *g = wn + 5 * (size_t) idx;
                    note(1);
                    const uint32_t hitsMask = wideNodeHits(g[0], g[1], g[2], g[3], g[4], ray);
                    ng = make_uint2(g[1].x, (hitsMask & 0xff000000u) | (g[0].w >> 24));
                    tg = make_uint2(g[1].y, hitsMask & 0x00ffffffu);
                }
                if (tg.y) {
                    const uint32_t bit = (uint32_t) __builtin_ctz(tg.y);
                    tg.y &= tg.y - 1u;
                    const size_t k = (size_t) tg.x + bit;
                    if (k >= nRecs) throw std::runtime_error("wide BVH: triangle index out of range");
                    note(2);
                    float tu, tv, tt;
                    if (waldIntersect(recs[3 * k], recs[3 * k + 1], recs[3 * k + 2], o, d, ray.mint, ray.maxt, tu, tv, tt) && winsTie(tt, pm_to_bits(recs[3 * k + 2].z), h.t, h.prim)) { ray.maxt = tt; h.t = tt; h.u = tu; h.v = tv; h.prim = pm_to_bits(recs[3 * k + 2].z); }
                }
                if (tg.y == 0u && !(ng.y & 0xff000000u)) {
                    if (stack.empty()) break;
                    ng = stack.back(); stack.pop_back();
                }
            }
        }
        hits[i] = h;
    }
}

extern "C" {

/* Closest-hit ray casts through the compressed wide BVH ON THE HOST: the tree of buildWide() walked with the node-step
   arithmetic of k_wide.h (wideNodeHits is __host__ __device__) and the Wald test of dv_scene.h.  Lets the CPU test-suite pin
   the builder's encoding (quantisation, slots, child / triangle indexing) and the group stack logic against the oracle
   without a GPU; the device kernels run the same functions.  use_wide = 0 walks nothing and tests every record (brute force). */
int phip_debug_host_trace_wide(const float *positions, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles,
                               const phip_ray *rays, size_t n_rays, phip_hit *hits, int use_wide, phip_accel_info *info,
                               uint8_t *seq, uint32_t seq_stride /* optional: the ray's steps in order, 1 = node step, 2 = triangle test, 0 = end */) {
    try {
        for (uint32_t i = 0; i < 3 * n_triangles; ++i) if (indices[i] >= n_vertices) return setErr(PHIP_ERR_INVALID, "index out of range");
        HostBVH bvh; buildBVH(positions, indices, n_triangles, bvh);
        if (info) {
            memset(info, 0, sizeof(*info));
            info->n_nodes = bvh.nWNodes; info->max_depth = bvh.wMaxDepth; info->n_triangle_refs = bvh.nWTris; info->node_bytes = 80; info->triangle_bytes = 48;
            info->sah_cost = bvh.wSahCost; info->build_ms = bvh.buildMs;
        }
        if (use_wide && bvh.nWNodes == 0) return setErr(PHIP_ERR_INVALID, "the scene has no wide tree (a single leaf)");
        hostTraceRays(bvh.sceneMin, bvh.sceneMax, (const float4 *) (use_wide ? bvh.wtris.data() : bvh.tris.data()), (use_wide ? bvh.wtris.size() : bvh.tris.size()) / 12,
                      (const uint4 *) bvh.wnodes.data(), bvh.nWNodes, use_wide, rays, n_rays, hits, seq, seq_stride);
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

/* The refit of phip_scene_update ON THE HOST, sibling of phip_debug_host_trace_wide: the tree is built on positions_a (no camera), then refitted to positions_b and the
   camera position camera3 (NULL: none) -- and, if positions_c is given, once more to positions_c -- by the __host__ __device__ functions the kernels of k_update.h run
   (refit_hd.h), in their order; the rays are traced on the CPU twin of the wide traversal.  out_nodes (20 words per node), out_records (12 floats per record) and
   out_rec_prim (the creation's primitive of every record) receive the refitted tree when they are given: info->n_nodes and info->n_triangle_refs are their sizes (call
   once without them).  PHIP_ERR_UNSUPPORTED as phip_scene_update gives it. */
int phip_debug_host_refit_trace_wide(const float *positions_a, const float *positions_b, const float *positions_c, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles,
                                     const float *camera3, const phip_ray *rays, size_t n_rays, phip_hit *hits, phip_accel_info *info,
                                     uint32_t *out_nodes, float *out_records, uint32_t *out_rec_prim, uint32_t *out_n_degenerate) {
    try {
        for (uint32_t i = 0; i < 3 * n_triangles; ++i) if (indices[i] >= n_vertices) return setErr(PHIP_ERR_INVALID, "index out of range");
        HostBVH bvh; buildBVH(positions_a, indices, n_triangles, bvh);
        if (bvh.nWNodes == 0) return setErr(PHIP_ERR_INVALID, "the scene has no wide tree");
        const size_t nRecs = bvh.wtris.size() / 12;
        std::vector<uint32_t> recPrim(nRecs), had(((size_t) n_triangles + 31) / 32 + 1, 0u);
        for (size_t r = 0; r < nRecs; ++r) { memcpy(&recPrim[r], &bvh.wtris[12 * r + 10], 4); if (recPrim[r] < n_triangles) had[recPrim[r] >> 5] |= 1u << (recPrim[r] & 31u); }
        std::vector<float4> ts((size_t) TRISHADE_FLOAT4S * n_triangles, make_float4(0, 0, 0, 0));
        std::vector<float> nodeBox(6 * (size_t) bvh.nWNodes);
        const float noCamera[3] = { 0, 0, 0 };
        detail::RefitConsts K; memset(&K, 0, sizeof(K));
        uint32_t nDegenerate = 0;
        for (const float *pos : { positions_b, positions_c }) {
            if (!pos) continue;
            uint32_t grown = 0; nDegenerate = 0;
            for (uint32_t i = 0; i < n_triangles; ++i) {            /* k_upd_check */
                float rec[12];
                const bool ok = detail::waldLoad(pos + 3 * (size_t) indices[3 * (size_t) i], pos + 3 * (size_t) indices[3 * (size_t) i + 1], pos + 3 * (size_t) indices[3 * (size_t) i + 2], i, rec);
                const bool h = (had[i >> 5] >> (i & 31u)) & 1u;
                grown += ok && !h; nDegenerate += !ok && h;
            }
            if (grown) return setErr(PHIP_ERR_UNSUPPORTED, std::to_string(grown) + " triangles that were degenerate at creation are not degenerate now");
            for (uint32_t i = 0; i < n_triangles; ++i) detail::refitShadeRecord(pos, nullptr, indices, i, ts.data() + (size_t) TRISHADE_FLOAT4S * i);      /* k_upd_shade */
            float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (uint32_t i = 0; i < n_triangles; ++i) detail::growByTriangle(ts.data(), TRISHADE_FLOAT4S, i, mn, mx);                                     /* k_upd_box */
            detail::refitConstsOf(mn, mx, camera3 ? camera3 : noCamera, K);
            for (size_t r = 0; r < nRecs; ++r) detail::refitWaldRecord(ts.data(), TRISHADE_FLOAT4S, recPrim[r], (float4 *) bvh.wtris.data() + 3 * r);     /* k_upd_wald */
            double cost = 0;
            for (size_t l = bvh.wLevels.size(); l-- > 1; )                                                                                                 /* k_upd_refit_level */
                for (uint32_t idx = bvh.wLevels[l - 1]; idx < bvh.wLevels[l]; ++idx)
                    cost += detail::refitWideNode((uint4 *) bvh.wnodes.data() + 5 * (size_t) idx, idx, ts.data(), TRISHADE_FLOAT4S, recPrim.data(), K, nodeBox.data());
            bvh.wSahCost = (float) (cost + 1.0);
            for (int a = 0; a < 3; ++a) { bvh.sceneMin[a] = K.sceneMin[a]; bvh.sceneMax[a] = K.sceneMax[a]; }
        }
        if (info) {
            memset(info, 0, sizeof(*info));
            info->n_nodes = bvh.nWNodes; info->max_depth = bvh.wMaxDepth; info->n_triangle_refs = bvh.nWTris; info->node_bytes = 80; info->triangle_bytes = 48;
            info->sah_cost = bvh.wSahCost; info->build_ms = bvh.buildMs;
        }
        if (out_nodes) memcpy(out_nodes, bvh.wnodes.data(), (size_t) bvh.nWNodes * 80);
        if (out_records) memcpy(out_records, bvh.wtris.data(), nRecs * 48);
        if (out_rec_prim) memcpy(out_rec_prim, recPrim.data(), nRecs * 4);
        if (out_n_degenerate) *out_n_degenerate = nDegenerate;
        hostTraceRays(bvh.sceneMin, bvh.sceneMax, (const float4 *) bvh.wtris.data(), nRecs, (const uint4 *) bvh.wnodes.data(), bvh.nWNodes, 1, rays, n_rays, hits, nullptr, 0);
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

/* phip_scene_rebuild ON THE HOST, sibling of the hook above with the same arguments: shading records of positions_a, then for positions_b and positions_c in turn (or for
   positions_a itself when neither is given) the pipeline of host_rebuild.h by the __host__ __device__ functions its kernels run (rebuild_hd.h), in their order -- keys,
   the sort (std::stable_sort), the binary radix tree, its boxes bottom-up with the arrival flags, the collapse level by level with a serial scan -- and the refit of
   refit_hd.h on the new topology; the rays are traced on the CPU twin of the wide traversal.  info->n_leaves = leaf slots; *out_n_degenerate = triangles without a record.
   PHIP_ERR_UNSUPPORTED for a tree the traversal stacks do not hold, as phip_scene_rebuild gives it */
int phip_debug_host_rebuild_trace_wide(const float *positions_a, const float *positions_b, const float *positions_c, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles,
                                       const float *camera3, const phip_ray *rays, size_t n_rays, phip_hit *hits, phip_accel_info *info,
                                       uint32_t *out_nodes, float *out_records, uint32_t *out_rec_prim, uint32_t *out_n_degenerate) {
    try {
        for (uint32_t i = 0; i < 3 * n_triangles; ++i) if (indices[i] >= n_vertices) return setErr(PHIP_ERR_INVALID, "index out of range");
        const uint32_t n = n_triangles;
        std::vector<float4> ts((size_t) TRISHADE_FLOAT4S * std::max(n, 1u), make_float4(0, 0, 0, 0));
        for (uint32_t i = 0; i < n; ++i) detail::refitShadeRecord(positions_a, nullptr, indices, i, ts.data() + (size_t) TRISHADE_FLOAT4S * i);
        const float noCamera[3] = { 0, 0, 0 };
        detail::RefitConsts K; memset(&K, 0, sizeof(K));
        std::vector<uint32_t> wnodes, recPrim, levels; std::vector<float4> wtris; std::vector<float> nodeBox;
        uint32_t nNodes = 0, m = 0, leafSlots = 0; float sah = 1.0f;
        const auto t0 = std::chrono::steady_clock::now();
        for (const float *pos : { positions_b, positions_c, (positions_b || positions_c) ? nullptr : positions_a }) {
            if (!pos) continue;
            for (uint32_t i = 0; i < n; ++i) detail::refitShadeRecord(pos, nullptr, indices, i, ts.data() + (size_t) TRISHADE_FLOAT4S * i);      /* k_upd_shade */
            float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (uint32_t i = 0; i < n; ++i) detail::growByTriangle(ts.data(), TRISHADE_FLOAT4S, i, mn, mx);                                     /* k_upd_box */
            detail::refitConstsOf(mn, mx, camera3 ? camera3 : noCamera, K);
            std::vector<std::pair<uint32_t, uint32_t>> pairs(n);                                                                                 /* k_rb_keys */
            m = 0;
            for (uint32_t i = 0; i < n; ++i) { pairs[i] = { detail::rebuildKey(ts.data(), TRISHADE_FLOAT4S, i, K), i }; m += pairs[i].first != REBUILD_NO_KEY; }
            std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) { return a.first < b.first; });
            std::vector<uint32_t> keys(n), tris(n);
            for (uint32_t i = 0; i < n; ++i) { keys[i] = pairs[i].first; tris[i] = pairs[i].second; }
            const uint32_t maxNodes = std::max(m, 1u);
            std::vector<int32_t> child(2 * (size_t) maxNodes), items(maxNodes), slotRef(8 * (size_t) maxNodes);
            std::vector<uint32_t> range(2 * (size_t) maxNodes), parent(2 * (size_t) maxNodes, REBUILD_NO_NODE), arrived(maxNodes, 0u);
            std::vector<float> box(12 * (size_t) maxNodes);
            detail::RebuildTree T; T.keys = keys.data(); T.tris = tris.data(); T.nValid = m; T.child = child.data(); T.range = range.data(); T.parent = parent.data();
            T.box = box.data(); T.arrived = arrived.data();
            for (uint32_t i = 0; i + 1 < m; ++i) detail::rebuildInnerNode(T, i);                                                                 /* k_rb_inner */
            for (uint32_t p = 0; p < m; ++p) {                                                                                                   /* k_rb_boxes */
                float bmn[3], bmx[3];
                detail::rebuildLeafBox(T, ts.data(), TRISHADE_FLOAT4S, p, bmn, bmx);
                uint32_t cur = m - 1u + p;
                for (;;) {
                    const uint32_t par = parent[cur];
                    if (par == REBUILD_NO_NODE) break;
                    const uint32_t before = arrived[par]++;
                    if (!detail::rebuildClimbStep(T, cur, par, before, bmn, bmx)) break;
                }
            }
            wnodes.assign(20 * (size_t) maxNodes, 0u); recPrim.assign(maxNodes, 0xFFFFFFFFu); levels.assign(1, 0u); leafSlots = 0;
            uint32_t nRecs = 0;
            if (m == 0) { nNodes = 1; levels.push_back(1u); }
            else {
                items[0] = m == 1 ? ~(int32_t) 0 : 0;
                uint32_t first = 0, count = 1;
                while (count) {
                    if (!wideDepthFits((uint32_t) levels.size())) return setErr(PHIP_ERR_UNSUPPORTED, "the new tree is deeper than the traversal stacks allow");
                    const uint32_t nextFirst = first + count;
                    std::vector<unsigned long long> scan(count + 1, 0ull);
                    for (uint32_t i = 0; i < count; ++i) {                                                                                       /* k_rb_collapse, the scan */
                        uint32_t nInner, nR;
                        detail::rebuildCollapseNode(T, items[first + i], slotRef.data() + 8 * (size_t) (first + i), nInner, nR);
                        scan[i + 1] = scan[i] + ((unsigned long long) nInner | ((unsigned long long) nR << 32));
                    }
                    if ((size_t) nextFirst + (uint32_t) scan[count] > maxNodes || (size_t) nRecs + (uint32_t) (scan[count] >> 32) > m) throw std::runtime_error("a level of the collapse does not fit the tree's bounds");
                    for (uint32_t i = 0; i < count; ++i)                                                                                         /* k_rb_emit */
                        leafSlots += detail::rebuildEmitNode(T, slotRef.data() + 8 * (size_t) (first + i), nextFirst + (uint32_t) scan[i], nRecs + (uint32_t) (scan[i] >> 32),
                                                             (uint4 *) wnodes.data() + 5 * (size_t) (first + i), recPrim.data(), items.data());
                    levels.push_back(nextFirst);
                    first = nextFirst; nRecs += (uint32_t) (scan[count] >> 32); count = (uint32_t) scan[count];
                }
                nNodes = first;
                if (nRecs != m) throw std::runtime_error("the collapse lost records");
            }
            wtris.assign(3 * (size_t) maxNodes, make_float4(0, 0, 0, 0)); nodeBox.assign(6 * (size_t) maxNodes, 0.0f);
            for (uint32_t r = 0; r < m; ++r) detail::refitWaldRecord(ts.data(), TRISHADE_FLOAT4S, recPrim[r], wtris.data() + 3 * (size_t) r);   /* k_upd_wald */
            double cost = 0;
            for (size_t l = levels.size(); l-- > 1; )                                                                                            /* k_upd_refit_level */
                for (uint32_t idx = levels[l - 1]; idx < levels[l]; ++idx)
                    cost += detail::refitWideNode((uint4 *) wnodes.data() + 5 * (size_t) idx, idx, ts.data(), TRISHADE_FLOAT4S, recPrim.data(), K, nodeBox.data());
            sah = (float) (cost + 1.0);
        }
        if (info) {
            memset(info, 0, sizeof(*info));
            info->n_nodes = nNodes; info->max_depth = (uint32_t) levels.size() - 1u; info->n_triangle_refs = m; info->n_leaves = leafSlots; info->node_bytes = 80; info->triangle_bytes = 48;
            info->sah_cost = sah; info->build_ms = (float) std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (out_nodes) memcpy(out_nodes, wnodes.data(), (size_t) nNodes * 80);
        if (out_records && m) memcpy(out_records, wtris.data(), (size_t) m * 48);
        if (out_rec_prim && m) memcpy(out_rec_prim, recPrim.data(), (size_t) m * 4);
        if (out_n_degenerate) *out_n_degenerate = n - m;
        hostTraceRays(K.sceneMin, K.sceneMax, wtris.data(), m, (const uint4 *) wnodes.data(), nNodes, 1, rays, n_rays, hits, nullptr, 0);
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

} // extern "C"

/* device execution of the phip_fmath.h functions (bitwise host/device agreement test) */
__global__ void k_debug_fmath(int op, size_t n, const float *a, const float *b, float *out) {
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s, c;
    switch (op) {
        case 0: pm_sincosf(a[i], &s, &c); out[i] = s; break;
        case 1: pm_sincosf(a[i], &s, &c); out[i] = c; break;
        case 2: out[i] = pm_expf(a[i]); break;
        case 3: out[i] = pm_logf(a[i]); break;
        case 4: out[i] = pm_acosf(a[i]); break;
        case 5: out[i] = pm_atan2f(a[i], b[i]); break;
        case 6: out[i] = pm_tanf(a[i]); break;
        case 7: out[i] = pm_powf(a[i], b[i]); break;
        case 8: out[i] = mts_erf(a[i]); break;
        case 9: out[i] = mts_erfinv(a[i]); break;
        case 10: out[i] = pm_atanf(a[i]); break;
        default: out[i] = 0;
    }
}

/* MIPMap::eval(uv, d0, d1) of dv_scene.h on the host: texture = one phip_texture (levels as delivered) */
extern "C" int phip_debug_host_mip_eval(const phip_texture *t, size_t n, const float *uv2, const float *d0, const float *d1, float *out3) {
    try {
        DevMipLevels lv; memset(&lv, 0, sizeof(lv));
        std::vector<float4> texels;
        lv.nLevels = (int32_t) std::max<uint32_t>(1, t->n_levels);
        int w = (int) t->width, h = (int) t->height;
        for (int l = 0; l < lv.nLevels; ++l) {
            lv.lw[l] = w; lv.lh[l] = h; lv.offset[l] = (uint32_t) texels.size();
            for (size_t i = 0; i < (size_t) w * h; ++i) texels.push_back(make_float4(t->levels[l][3 * i], t->levels[l][3 * i + 1], t->levels[l][3 * i + 2], 0.0f));
            w = std::max(1, (w + 1) / 2); h = std::max(1, (h + 1) / 2);
        }
        lv.bcu = t->wrap_u; lv.bcv = t->wrap_v; lv.filterType = t->filter_type; lv.maxAnisotropy = t->max_anisotropy;
        lv.uvScale[0] = lv.uvScale[1] = 1.0f;
        for (int k = 0; k < 64; ++k) { const float r2 = (float) k / 63.0f; lv.weightLut[k] = pm_expf(-2.0f * r2) - pm_expf(-2.0f); }
        for (size_t i = 0; i < n; ++i) {
            const V3 v = mipEval(texels.data(), lv, V2(uv2[2 * i], uv2[2 * i + 1]), V2(d0[2 * i], d0[2 * i + 1]), V2(d1[2 * i], d1[2 * i + 1]));
            out3[3 * i] = v.x; out3[3 * i + 1] = v.y; out3[3 * i + 2] = v.z;
        }
        return 0;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

/* The surface records of phip_trace_device on the host: the shading records come from the stages phip_scene_create runs before it builds the tree (validation, shapes,
   textures' maxima, materials, shadingRecords -- none of them calls HIP), the records from fillSurface (dv_scene.h), which k_surfaces evaluates on the device.
   hits: (t, u, v, prim) of every ray, from any ray cast of the scene. */
extern "C" int phip_debug_host_surfaces(const phip_scene_desc *desc, const phip_ray *rays, const phip_hit *hits, size_t n, phip_surface *out) {
    if (!desc || ((!rays || !hits || !out) && n)) return setErr(PHIP_ERR_INVALID, "NULL argument");
    try {
        phip_scene sc;
        SceneBuild B(&sc, *desc);
        B.validateDesc();
        B.flattenShapes(); B.packTextures(); B.materials();
        B.shadingRecords();
        DevScene S; memset(&S, 0, sizeof(S));
        S.triShade = B.ts.data(); S.triShadeStride = B.stride; S.nTriangles = desc->n_triangles;
        for (size_t i = 0; i < n; ++i) {
            if (hits[i].prim != PHIP_NO_HIT && hits[i].prim >= desc->n_triangles) return setErr(PHIP_ERR_INVALID, "hit primitive out of range");
            fillSurface(S, V3(rays[i].d[0], rays[i].d[1], rays[i].d[2]), hits[i].t, hits[i].u, hits[i].v, hits[i].prim, out[i]);
        }
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

extern "C" int phip_debug_fmath(int on_device, int op, size_t n, const float *a, const float *b, float *out) {
    if (!on_device) {
        for (size_t i = 0; i < n; ++i) {
            float s, c;
            switch (op) {
                case 0: pm_sincosf(a[i], &s, &c); out[i] = s; break;
                case 1: pm_sincosf(a[i], &s, &c); out[i] = c; break;
                case 2: out[i] = pm_expf(a[i]); break;
                case 3: out[i] = pm_logf(a[i]); break;
                case 4: out[i] = pm_acosf(a[i]); break;
                case 5: out[i] = pm_atan2f(a[i], b[i]); break;
                case 6: out[i] = pm_tanf(a[i]); break;
                case 7: out[i] = pm_powf(a[i], b[i]); break;
                case 8: out[i] = mts_erf(a[i]); break;
                case 9: out[i] = mts_erfinv(a[i]); break;
                case 10: out[i] = pm_atanf(a[i]); break;
                default: out[i] = 0;
            }
        }
        return PHIP_OK;
    }
    try {
        DevBuf<float> da, db, dout;
        da.upload(a, n); db.upload(b ? b : a, n); dout.alloc(n);
        hipLaunchKernelGGL(k_debug_fmath, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, op, n, (const float *) da.p, (const float *) db.p, dout.p);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, dout.p, n * sizeof(float), hipMemcpyDeviceToHost));
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_DEVICE, e.what()); }
}

/* PMC calibration (MI355X_MICROARCH.md, HBM section: FETCH_SIZE is uncalibrated for non-streaming access):
 * n lanes each gather one float4 from a pseudo-random index of a buffer far larger than the 256 MiB
 * Infinity Cache, and n lanes stream-write one float4.  Every gather misses all caches, so the HBM read
 * traffic is n x (line size) and the write traffic n x 16 B: comparing that with FETCH_SIZE / WRITE_SIZE of
 * this kernel gives the correction factors for the traversal kernels' access pattern. */
__global__ void k_debug_gather(const float4 *src, size_t nSrc, float4 *dst, size_t n) {
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const U4 h = pcg4d((uint32_t) i, (uint32_t) (i >> 32), 12345u, 7u);
    const size_t j = (((size_t) h.x << 32) | h.y) % nSrc;
    dst[i] = src[j];
}
__global__ void k_debug_stream(const float4 *src, float4 *dst, size_t n) {
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

extern "C" int phip_debug_pmc_calibration(size_t src_bytes, size_t n) {
    try {
        DevBuf<float4> src, dst;
        src.alloc(src_bytes / 16); dst.alloc(n);
        HIP_TRY(hipMemset(src.p, 0, src_bytes));
        HIP_TRY(hipMemset(dst.p, 0, n * 16));
        HIP_TRY(hipDeviceSynchronize());
        hipLaunchKernelGGL(k_debug_gather, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, (const float4 *) src.p, src_bytes / 16, dst.p, n);
        hipLaunchKernelGGL(k_debug_stream, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, (const float4 *) src.p, dst.p, n);
        HIP_TRY(hipDeviceSynchronize());
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_DEVICE, e.what()); }
}

/* ---- the vector-memory roof of a CU under divergence (round 3) ----
 * The ray kernels of the big scenes are bound neither by HBM (7-10 % of the peak) nor by the ALUs (VALU issue 40 %): every lane
 * fetches its own node, so what they load the chip with is LANE-LEVEL 16-byte requests to the CU's texture addresser / L1
 * (TA / TCP).  This micro-benchmark measures what that path sustains, as the ray kernels use it: every lane of a resident grid
 * issues `iters` x 4 independent loads of 16 bytes from pseudo-random places of a buffer that lives in L1 / L2 / Infinity Cache.
 *   mode 0  one random 16-byte element per lane                        (a node / record fetch of k_rays_w)
 *   mode 1  the 4 lanes of a quad read the 4 pieces of one random 64-byte block  (what a transposed, quad-cooperative node fetch would issue)
 *   mode 2  8 lanes share a random 128-byte line        mode 3  16 lanes share 256 bytes
 *   mode 4  as 0 with every second lane switched off    mode 5  as 0 with 16 of the 64 lanes active   (is the cost per instruction or per lane?)
 *   mode 6  five consecutive 16-byte pieces of one random 80-byte record per lane, as five instructions (an 80-byte wide node)
 *   mode 7  one random dword per lane                   mode 8  one random 8 bytes per lane
 *   mode 9  fully coalesced: lane i reads element base + i of a random 1-KB block
 *   mode 10 / 11  as 0 with 8 / 4 of the 64 lanes active
 * Returns the time of the launch; lane_loads = active lanes x loads.  Blocks per CU are pinned with dynamic LDS. */
template <int MODE> __global__ __launch_bounds__(256) void k_debug_vmem(const uint4 *src, uint32_t mask /* elements - 1 */, int iters, uint4 *out) {
    extern __shared__ unsigned char dummy[];
    const uint32_t lane = __lane_id(), gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t grp = MODE == 1 ? 4u : (MODE == 2 ? 8u : (MODE == 3 ? 16u : (MODE == 9 ? 64u : 1u)));
    uint32_t x = (gid / grp) * 2654435761u + 12345u;            /* the lanes of a group draw the same numbers */
    const bool on = MODE == 4 ? (lane & 1u) == 0u : (MODE == 5 ? (lane & 3u) == 0u : (MODE == 10 ? (lane & 7u) == 0u : (MODE == 11 ? (lane & 15u) == 0u : true)));
    uint4 acc = make_uint4(0, 0, 0, 0);
    if (on) {
        for (int i = 0; i < iters; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x = x * 1664525u + 1013904223u;
                const uint32_t r = x >> 4;
                if (MODE == 6) {
                    const uint32_t e = (r % ((mask + 1u) / 5u)) * 5u;
#pragma unroll
                    for (int k = 0; k < 5; ++k) { const uint4 v = src[e + k]; acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w; }
                } else if (MODE == 7) {
                    acc.x ^= ((const uint32_t *) src)[r & (4u * mask + 3u)];
                } else if (MODE == 8) {
                    const uint2 v = ((const uint2 *) src)[r & (2u * mask + 1u)]; acc.x ^= v.x; acc.y ^= v.y;
                } else {
                    const uint32_t e = grp == 1u ? (r & mask) : (((r * grp) & mask) + (lane & (grp - 1u)));
                    const uint4 v = src[e]; acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
                }
            }
        }
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) out[gid] = acc;       /* (practically never: keeps the loads alive) */
    if (dummy[0] == 77 && acc.z == 1u) out[0] = acc;
}

extern "C" int phip_debug_vmem_roof(int mode, size_t bytes, int blocks_per_cu, int iters, double *out_ms, double *out_lane_loads) {
    try {
        size_t n = 1; while (n * 2 * 16 <= bytes) n *= 2;       /* 16-byte elements, a power of two */
        DevBuf<uint4> src, out;
        src.alloc(n);
        HIP_TRY(hipMemset(src.p, 0x5a, n * 16));
        int dev = 0, nCU = 256; HIP_TRY(hipGetDevice(&dev));
        { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, dev) == hipSuccess) nCU = prop.multiProcessorCount; }
        const int grid = nCU * blocks_per_cu;
        out.alloc((size_t) grid * 256);
        const size_t lds = (size_t) (160 * 1024 / blocks_per_cu) / 1024 * 1024 - 1024;     /* exactly blocks_per_cu blocks fit a CU */
        typedef void (*K)(const uint4 *, uint32_t, int, uint4 *);
        static const K table[12] = { k_debug_vmem<0>, k_debug_vmem<1>, k_debug_vmem<2>, k_debug_vmem<3>, k_debug_vmem<4>, k_debug_vmem<5>, k_debug_vmem<6>, k_debug_vmem<7>, k_debug_vmem<8>, k_debug_vmem<9>, k_debug_vmem<10>, k_debug_vmem<11> };
        if (mode < 0 || mode > 11) return setErr(PHIP_ERR_INVALID, "mode");
        const K k = table[mode];
        if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *) k, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        hipEvent_t e0, e1; HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, 0, (const uint4 *) src.p, (uint32_t) (n - 1), std::max(1, iters / 8), out.p);     /* warm-up: caches, clocks */
        HIP_TRY(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, 0, (const uint4 *) src.p, (uint32_t) (n - 1), iters, out.p);
        HIP_TRY(hipEventRecord(e1, 0));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
        const double lanesOn = mode == 4 ? 0.5 : (mode == 5 ? 0.25 : (mode == 10 ? 0.125 : (mode == 11 ? 0.0625 : 1.0)));
        if (out_ms) *out_ms = ms;
        if (out_lane_loads) *out_lane_loads = (double) grid * 256.0 * lanesOn * (double) iters * 4.0 * (mode == 6 ? 5.0 : 1.0);
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_DEVICE, e.what()); }
}

/* The RCCL calls of the merge on whatever is there: librccl is bound as renderMultiDevice binds it, a clique is made of the first
   min(n, visible) devices -- ONE device is a valid clique --, and ncclReduce(sum) is run inside a group as the merge runs it, on a buffer
   of ones.  On the single-GPU boxes of this pool that is the only way the six entry points ever execute (the merge itself needs two distinct
   devices); returns the number of devices that took part, or a negative error code (phip_last_error). */
extern "C" int phip_debug_rccl_selftest(int n_devices, size_t n_floats) {
    try {
        int visible = 0; HIP_TRY(hipGetDeviceCount(&visible));
        const int n = std::max(1, std::min(n_devices, visible));
        std::vector<int> devices(n); for (int i = 0; i < n; ++i) devices[i] = i;
        std::lock_guard<std::mutex> g(g_rccl.lock);
        g_rccl.bind();
        const std::vector<ncclComm_t> &comm = g_rccl.clique(devices);
        std::vector<float *> buf(n, nullptr); std::vector<hipStream_t> st(n, nullptr);
        std::vector<float> ones(n_floats, 1.0f);
        for (int i = 0; i < n; ++i) {
            HIP_TRY(hipSetDevice(devices[i])); HIP_TRY(hipStreamCreate(&st[i]));
            HIP_TRY(hipMalloc((void **) &buf[i], n_floats * sizeof(float)));
            HIP_TRY(hipMemcpy(buf[i], ones.data(), n_floats * sizeof(float), hipMemcpyHostToDevice));
        }
        g_rccl.check(g_rccl.GroupStart(), "ncclGroupStart");
        for (int i = 0; i < n; ++i) {
            HIP_TRY(hipSetDevice(devices[i]));
            g_rccl.check(g_rccl.Reduce(buf[i], buf[i], n_floats, ncclFloat, ncclSum, 0, comm[i], st[i]), "ncclReduce");
        }
        g_rccl.check(g_rccl.GroupEnd(), "ncclGroupEnd");
        for (int i = 0; i < n; ++i) { HIP_TRY(hipSetDevice(devices[i])); HIP_TRY(hipStreamSynchronize(st[i])); }
        HIP_TRY(hipSetDevice(devices[0]));
        HIP_TRY(hipMemcpy(ones.data(), buf[0], n_floats * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) { HIP_TRY(hipSetDevice(devices[i])); (void) hipFree(buf[i]); (void) hipStreamDestroy(st[i]); }
        HIP_TRY(hipSetDevice(devices[0]));
        for (size_t k = 0; k < n_floats; ++k) if (ones[k] != (float) n) return setErr(PHIP_ERR_DEVICE, "ncclReduce(sum) of ones over " + std::to_string(n) + " device(s) gave " + std::to_string(ones[k]));
        return n;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_DEVICE, e.what()); }
}

/* phip_radiance_device's checks of its arguments that need no device (host_radiance.h: radianceArgsError), for a machine without one: the code the entry point would
   return for them, PHIP_OK when it would go on to the scene and the pointers' attributes; the message in phip_last_error */
extern "C" int phip_debug_host_radiance_args(const phip_render_params *params, const phip_radiance_desc *desc) {
    return radianceRefusal(params, desc);
}

/* ... and those of phip_camera_rays_device and phip_film_device (host_camera_film.h: cameraRaysArgsError, filmArgsError) */
extern "C" int phip_debug_host_camera_rays_args(const phip_render_params *params, const phip_camera_rays_desc *desc) {
    return cameraRaysRefusal(params, desc);
}
extern "C" int phip_debug_host_film_args(const phip_render_params *params, const phip_film_desc *desc) {
    return filmRefusal(params, desc);
}

/* phip_scene_update_appearance's refusals on a machine without a device (host_appearance.h): the scene's look is taken from the descriptor of its creation by the
   creation's host stages, the call's checks run on it -- with host pointers all of them, the textures' maxima and the environment map's CDF through the functions
   of appearance_hd.h the kernels run; with device_pointers = 1 those that need no texel.  The code the entry point would return, the message in phip_last_error */
extern "C" int phip_debug_host_appearance_args(const phip_scene_desc *created, const phip_appearance_desc *a) {
    if (!created) return setErr(PHIP_ERR_INVALID, "NULL argument");
    try {
        phip_scene sc;
        SceneBuild B(&sc, *created);
        B.validateDesc();
        B.flattenShapes(); B.packTextures(); B.materials(); B.emitterSelection(); B.buildEnvmap();
        B.keepAppearance();
        if (appearanceEmpty(a)) return PHIP_OK;
        AppearanceLook L;
        if (int rc = appearanceRefusal([&] { appearanceArgs(&sc, *a, L); })) return rc;
        const SceneUpdateState::Appearance &P = sc.upd.app;
        L.texMax = P.texMax;
        if (a->textures && !a->device_pointers)
            for (uint32_t i = 0; i < a->n_textures; ++i) {
                if (!a->textures[i].width) continue;
                float m = 0.0f;
                const float *c = a->textures[i].levels[0];
                for (size_t k = 0; k < (size_t) P.texDesc[i].lw[0] * P.texDesc[i].lh[0]; ++k) m = detail::texelMaxStep(m, c[3 * k], c[3 * k + 1], c[3 * k + 2]);
                L.texMax[i] = m;
            }
        if (int rc = appearanceRefusal([&] { appearanceLook(&sc, *a, L); })) return rc;
        if (a->envmap && !a->device_pointers) {
            phip_scene_desc d2 = *created; d2.envmap = *a->envmap;
            phip_scene sc2;
            SceneBuild B2(&sc2, d2);
            B2.envIsMap = true;
            if (int rc = appearanceRefusal([&] { B2.buildEnvmap(); })) return rc;
        }
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

/* the environment map's sampling tables as phip_scene_create builds them (SceneBuild::buildEnvmap, around appearance_hd.h): cdf_cols (w + 1) * h, cdf_rows h + 1,
   row_weights h floats, and the normalization */
extern "C" int phip_debug_host_envmap_cdf(const phip_envmap *envmap, float *cdf_cols, float *cdf_rows, float *row_weights, float *normalization) {
    if (!envmap || !cdf_cols || !cdf_rows || !row_weights || !normalization) return setErr(PHIP_ERR_INVALID, "NULL argument");
    try {
        phip_scene_desc d; memset(&d, 0, sizeof(d)); d.envmap = *envmap;
        phip_scene sc;
        SceneBuild B(&sc, d);
        B.envIsMap = true;
        B.buildEnvmap();
        memcpy(cdf_cols, B.envCdfCols.data(), B.envCdfCols.size() * sizeof(float)); memcpy(cdf_rows, B.envCdfRows.data(), B.envCdfRows.size() * sizeof(float));
        memcpy(row_weights, B.envRowWeights.data(), B.envRowWeights.size() * sizeof(float));
        *normalization = sc.devs[0]->dev.env.normalization;
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

/* ---- phip_bsdf_device, phip_emitter_sample_device, phip_emitter_eval_device without a device ---- */
/* their checks of the arguments (host_shading_parts.h): the code the entry point would return for them, PHIP_OK when it would go on to the device and the
   pointers' attributes; the message in phip_last_error.  have_scene = 0: the scene argument is NULL */
extern "C" int phip_debug_host_bsdf_args(int have_scene, const phip_bsdf_desc *desc) {
    return bsdfRefusal(have_scene != 0, desc);
}
extern "C" int phip_debug_host_emitter_sample_args(int have_scene, const phip_emitter_sample_desc *desc) {
    return emitterSampleRefusal(have_scene != 0, desc);
}
extern "C" int phip_debug_host_emitter_eval_args(int have_scene, const phip_emitter_eval_desc *desc) {
    return emitterEvalRefusal(have_scene != 0, desc);
}

/* phip_mip_pyramid_device's checks of the arguments (host_pyramid.h) likewise: everything but whose memory the pointers are */
extern "C" int phip_debug_host_pyramid_args(int have_scene, const phip_pyramid_desc *desc) {
    return pyramidDeviceRefusal(have_scene != 0, desc);
}

/* phip_vertex_normals_device's checks of the arguments (host_normals.h) likewise, against the counts a scene would have */
extern "C" int phip_debug_host_normals_args(int have_scene, uint32_t scene_vertices, uint32_t scene_triangles, const phip_normals_desc *desc) {
    return normalsRefusal(have_scene != 0, scene_vertices, scene_triangles, desc);
}

/* pm_asinf (phip_fmath.h) on the host: phip_debug_fmath's kernel does not know it -- on the device k_vertex_normals alone calls it */
extern "C" int phip_debug_host_asinf(size_t n, const float *a, float *out) {
    for (size_t i = 0; i < n; ++i) out[i] = pm_asinf(a[i]);
    return PHIP_OK;
}

/* The DevScene of a descriptor on the host: the stages phip_scene_create runs before it uploads (none of them calls HIP) -- shapes, textures, materials, emitters,
   the tree (for the scene box the environment emitter's sphere is made of), shading records, the emitter table, the environment map's tables -- with the
   DevScene's pointers bound to the builder's arrays instead of device buffers.  What the items of k_shading_parts.h read of a scene is all there. */
struct HostSceneTwin {
    phip_scene sc; SceneBuild B; DevScene S;
    explicit HostSceneTwin(const phip_scene_desc &d) : B(&sc, d) {
        B.validateDesc();
        B.flattenShapes(); B.packTextures(); B.materials(); B.emitterSelection();
        B.buildAccel();
        B.shadingRecords();
        B.packEmitterTable(); B.environmentSphere(); B.buildEnvmap();
        B.sceneConstants();
        S = B.D;
        S.triShade = B.ts.data(); S.materials = B.mats.data(); S.emitterTab = B.tab.data();
        S.texTexels = B.texTexels.data(); S.textures = B.texDesc.data();
        S.env.texels = B.envTexels.data(); S.env.levels = &B.envLevels; S.env.cdfRows = B.envCdfRows.data(); S.env.cdfCols = B.envCdfCols.data(); S.env.rowWeights = B.envRowWeights.data();
    }
    EmitterTab table() const { EmitterTab T; T.t = S.emitterTab; T.n = S.nEmitters; T.normalization = S.emitterNormalization; return T; }
};

/* The host twins: the statement each kernel of k_shading_parts.h evaluates per lane, over the same descriptor with HOST pointers, after the entry point's own
   argument checks (alignment included) */
extern "C" int phip_debug_host_bsdf_parts(const phip_scene_desc *created, const phip_bsdf_desc *b) {
    if (!created) return setErr(PHIP_ERR_INVALID, "NULL argument");
    if (const int rc = bsdfRefusal(true, b)) return rc;
    try {
        HostSceneTwin H(*created);
        const float4 *rays = (const float4 *) b->d_rays, *hits = (const float4 *) b->d_hits, *wo = (const float4 *) b->d_wo;
        const float2 *smp = (const float2 *) b->d_samples;
        const bool local = (b->flags & PHIP_BSDF_LOCAL) != 0;
        for (size_t i = 0; i < b->n; ++i) {
            const float4 rd = rays[2 * i + 1];
            const V3 woIn = b->d_eval ? V3(wo[i].x, wo[i].y, wo[i].z) : V3(0.0f);
            const V2 s = b->d_sampled ? V2(smp[i].x, smp[i].y) : V2(0.0f, 0.0f);
            BsdfPartsOut o;
            if (b->d_eval && b->d_sampled) bsdfPartsItem<true, true>(H.S, H.S.materials, V3(rd.x, rd.y, rd.z), hits[i], woIn, s, local, o);
            else if (b->d_eval) bsdfPartsItem<true, false>(H.S, H.S.materials, V3(rd.x, rd.y, rd.z), hits[i], woIn, s, local, o);
            else if (b->d_sampled) bsdfPartsItem<false, true>(H.S, H.S.materials, V3(rd.x, rd.y, rd.z), hits[i], woIn, s, local, o);
            else bsdfPartsItem<false, false>(H.S, H.S.materials, V3(rd.x, rd.y, rd.z), hits[i], woIn, s, local, o);
            if (b->d_eval) ((float4 *) b->d_eval)[i] = o.eval;
            if (b->d_sampled) { float4 *d = (float4 *) b->d_sampled + 3 * i; d[0] = o.s0; d[1] = o.s1; d[2] = o.s2; }
            if (b->d_wi_local) ((float4 *) b->d_wi_local)[i] = o.wi;
        }
        return PHIP_OK;
    } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, e.what()); }
}

extern "C" int phip_debug_host_emitter_sample(const phip_scene_desc *created, const phip_emitter_sample_desc *e) {
    if (!created) return setErr(PHIP_ERR_INVALID, "NULL argument");
    if (const int rc = emitterSampleRefusal(true, e)) return rc;
    try {
        HostSceneTwin H(*created);
        const EmitterTab T = H.table();
        const float4 *ref = (const float4 *) e->d_ref, *refN = (const float4 *) e->d_ref_n;
        const float2 *smp = (const float2 *) e->d_samples;
        for (size_t i = 0; i < e->n; ++i) {
            const V3 rn = refN ? V3(refN[i].x, refN[i].y, refN[i].z) : V3(0.0f);
            EmitterSampleOut o;
            if (H.S.envEmitter >= 0) emitterSampleItem<true>(H.S, T, V3(ref[i].x, ref[i].y, ref[i].z), rn, V2(smp[i].x, smp[i].y), o);
            else emitterSampleItem<false>(H.S, T, V3(ref[i].x, ref[i].y, ref[i].z), rn, V2(smp[i].x, smp[i].y), o);
            float4 *d = (float4 *) e->d_sampled + 3 * i; d[0] = o.s0; d[1] = o.s1; d[2] = o.s2;
            if (e->d_shadow_rays) { float4 *r = (float4 *) e->d_shadow_rays + 2 * i; r[0] = o.ro; r[1] = o.rd; }
        }
        return PHIP_OK;
    } catch (const std::exception &x) { return setErr(PHIP_ERR_INVALID, x.what()); }
}

extern "C" int phip_debug_host_emitter_eval(const phip_scene_desc *created, const phip_emitter_eval_desc *e) {
    if (!created) return setErr(PHIP_ERR_INVALID, "NULL argument");
    if (const int rc = emitterEvalRefusal(true, e)) return rc;
    try {
        HostSceneTwin H(*created);
        const EmitterTab T = H.table();
        const float4 *rays = (const float4 *) e->d_rays, *hits = (const float4 *) e->d_hits, *refN = (const float4 *) e->d_ref_n;
        for (size_t i = 0; i < e->n; ++i) {
            const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
            const V3 rn = refN ? V3(refN[i].x, refN[i].y, refN[i].z) : V3(0.0f);
            float4 ev; int32_t emitter;
            if (H.S.envEmitter >= 0) emitterEvalItem<true>(H.S, T, V3(ro.x, ro.y, ro.z), V3(rd.x, rd.y, rd.z), hits[i], rn, ev, emitter);
            else emitterEvalItem<false>(H.S, T, V3(ro.x, ro.y, ro.z), V3(rd.x, rd.y, rd.z), hits[i], rn, ev, emitter);
            ((float4 *) e->d_eval)[i] = ev;
            if (e->d_emitter) e->d_emitter[i] = emitter;
        }
        return PHIP_OK;
    } catch (const std::exception &x) { return setErr(PHIP_ERR_INVALID, x.what()); }
}

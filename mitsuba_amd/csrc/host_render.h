/*
 * host_render.h -- host side of libphip.so, second of three: one device's share of a render call.  The choice of the render's kernels (shadeUnit: the one table
 * over the feature sets; megaKernelOf, shadeKernelOf, shadeTraceWideKernelOf), the residency query of the persistent ones (residentBlocksPerCU), the byte model
 * of the statistics, validation of the parameters, the plans (FusedPlan, WavefrontPlan), and the render as stages over one RenderJob with renderOnDevice as
 * their one pass loop.  Every kernel launch of a render is here.
 * Host code only; included by phip.hip alone, after host_boundary.h.
 */
#pragma once
#include "host_boundary.h"

/* ---- which kernel a render runs (the look-ups of the other units: phip_common.h) ---- */
/* The look-ups of one feature set of the shading kernels (FEAT: 1 environment emitter, 2 bitmap textures, 8 the QMC samplers -- without / with both other features) */
struct ShadeUnit {
    ShadeKernel (*shade[2])(int materialMask, int tables);      /* k_shade without / with strictNormals */
    ShadeKernel (*direct)(int materialMask);
    ShadeKernel (*trace)(bool strictNormals, int materialMask);
    ShadeTraceWideKernel (*traceWide)(bool strictNormals, int materialMask);
    ShadeRaysKernel (*rays[2])(int materialMask, int tables);   /* k_shade_r without / with strictNormals (phip_radiance_device: the counter stream only, so nullptr with FEAT bit 3) */
};
/* The one place that maps a feature set to its objects */
static const ShadeUnit &shadeUnit(int feat) {
#define SHADE_UNIT(n, r0, r1) { { phipShadeKernelS0F##n, phipShadeKernelS1F##n }, phipShadeDirectKernelF##n, phipShadeTraceKernelF##n, phipShadeTraceWideKernelF##n, { r0, r1 } }
#define SHADE_UNIT_R(n) SHADE_UNIT(n, phipShadeRaysKernelS0F##n, phipShadeRaysKernelS1F##n)
    static const ShadeUnit units[6] = { SHADE_UNIT_R(0), SHADE_UNIT_R(1), SHADE_UNIT_R(2), SHADE_UNIT_R(3), SHADE_UNIT(8, nullptr, nullptr), SHADE_UNIT(11, nullptr, nullptr) };
#undef SHADE_UNIT_R
#undef SHADE_UNIT
    switch (feat & 11) {
        case 0: return units[0];
        case 1: return units[1];
        case 2: return units[2];
        case 8: return units[4];
        case 11: return units[5];
        default: return units[3];
    }
}
/* k_shade's table set: FEAT 0 (no environment emitter, no textures, the counter stream) has builds that address the emitter table and the materials (1), or the emitter
   table only (2), as LDS; every other feature set reads them through generic pointers (0) */
static int shadeTableSet(int feat, const DevScene &S) {
    if ((feat & 11) != 0 || S.emitterTabSize > EMITTER_LDS_FLOATS) return 0;
    return S.nMaterials <= MATERIAL_LDS_MAX ? 1 : 2;
}
/* The vertex kernel of the wavefront iterations that take the pool alone: k_shade_direct (`direct`), k_shade_trace (the packed leaf table in LDS) or k_shade */
static ShadeKernel shadeKernelOf(int feat, bool direct, bool shadeTrace, bool strictNormals, int materialMask, int tables) {
    const ShadeUnit &u = shadeUnit(feat);
    return direct ? u.direct(materialMask) : shadeTrace ? u.trace(strictNormals, materialMask) : u.shade[strictNormals ? 1 : 0](materialMask, tables);
}
/* ... and k_shade_trace_w, which also takes the number of staged nodes */
static ShadeTraceWideKernel shadeTraceWideKernelOf(int feat, bool strictNormals, int materialMask) {
    return shadeUnit(feat).traceWide(strictNormals, materialMask);
}
/* k_mega by integrator and traversal form (k_mega.h; >= 4: the 8-wide tree in memory); nullptr: no build of it serves the form */
static MegaKernel megaKernelOf(bool direct, int flat, int materialMask, bool strictNormals, bool qmc) {
    return direct ? phipMegaKernelDirect(materialMask, strictNormals, flat, qmc)
         : flat >= 4 ? phipMegaKernelWide(materialMask, strictNormals, flat, qmc) : phipMegaKernel(materialMask, strictNormals, flat, qmc);
}

/* Blocks of `block` threads and `lds` bytes of dynamic LDS of a kernel that the runtime finds resident on a compute unit (registers, static + dynamic LDS and the LDS
   allocation granule all enter); past 48 KB the kernel's dynamic-LDS limit is raised first.  `limit` is what that call answered -- when it refused, nothing is asked and
   blocks is 0 --, blocks is 0 too when the occupancy query fails: every caller has its own policy for the two */
struct Residency { hipError_t limit; int blocks; };
static Residency residentBlocksPerCU(const void *kernel, int block, size_t lds) {
    Residency r = { hipSuccess, 0 };
    if (lds > 48 * 1024) r.limit = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
    if (r.limit == hipSuccess && hipOccupancyMaxActiveBlocksPerMultiprocessor(&r.blocks, kernel, block, lds) != hipSuccess) r.blocks = 0;
    return r;
}

static size_t traversalLdsBytes(const DevScene &D) {               /* k_raycast_w: blocks of BLOCK threads */
    return wideLdsBytes(wideRaycastCache(D.wideNodeCache), BLOCK);
}

static void algorithmicBytes(bool mergedRays, phip_stats &st, double filmPixels) {
    /* SURVEY 8(d) with this structure's sizes: 80-byte node visits of the 8-wide tree, 48-byte triangle records
       (no separate index array: records are stored in leaf order) */
    const double film = 20.0 * filmPixels;
    const double nodeBytes = 80.0;
    st.algorithmic_bytes = nodeBytes * (double) (st.closest_node_visits + st.shadow_node_visits) +
           48.0 * (double) (st.closest_triangle_tests + st.shadow_triangle_tests) +
           (64.0 + 40.0 + 108.0) * (double) st.closest_rays + (64.0 + 4.0) * (double) st.shadow_rays +
           104.0 * (double) st.path_vertices + film;
    /* closest-hit kernel: node + triangle fetches, ray read (32 B), hit record write (16 B) ... counted with
       the SURVEY's read+write convention: ray 64 B, hit 40 B */
    st.trace_kernel_bytes = nodeBytes * (double) st.closest_node_visits + 48.0 * (double) st.closest_triangle_tests +
           (64.0 + 40.0) * (double) st.closest_rays;
    if (mergedRays)    /* k_rays_w also casts the shadow rays: their node + record fetches, entry read, 4-byte result */
        st.trace_kernel_bytes += nodeBytes * (double) st.shadow_node_visits + 48.0 * (double) st.shadow_triangle_tests +
               (64.0 + 4.0) * (double) st.shadow_rays;
}

/* hipEvents of one render call; destroyed whatever happens (an exception leaves through HIP_TRY) */
struct EventList {
    std::vector<hipEvent_t> ev;
    hipEvent_t record(hipStream_t s) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); ev.push_back(e); HIP_TRY(hipEventRecord(e, s)); return e; }
    double sumPairs() const { double ms = 0; for (size_t i = 0; i + 1 < ev.size(); i += 2) { float t = 0; (void) hipEventElapsedTime(&t, ev[i], ev[i + 1]); ms += t; } return ms; }
    ~EventList() { for (auto e : ev) (void) hipEventDestroy(e); }
};

static bool cancelRequested(const phip_scene *sc) { return __atomic_load_n(sc->cancelFlag, __ATOMIC_RELAXED) != 0; }

static void validateParams(const phip_scene *sc, const phip_render_params *p) {
    if (p->spp <= 0) throw std::invalid_argument("spp must be > 0");
    if (p->integrator > PHIP_INTEGRATOR_VOLPATH_SIMPLE) throw std::invalid_argument("unknown integrator kind");
    const bool direct = p->integrator == PHIP_INTEGRATOR_DIRECT;
    if (!direct) {
        if (p->rr_depth <= 0) throw std::invalid_argument("'rrDepth' must be set to a value greater than zero!");                       /* integrator.cpp:219-220 */
        if (p->max_depth <= 0 && p->max_depth != -1) throw std::invalid_argument("'maxDepth' must be set to -1 (infinite) or a value greater than zero!"); /* :222-223 */
    } else {
        if (p->emitter_samples < 0 || p->bsdf_samples < 0) throw std::invalid_argument("direct: emitterSamples and bsdfSamples must not be negative");
        if (p->emitter_samples + p->bsdf_samples <= 0) throw std::invalid_argument("direct: emitterSamples + bsdfSamples must be > 0");     /* Assert, direct.cpp:107 */
        if (p->emitter_samples + p->bsdf_samples >= (int) DEPTH_MASK) throw std::invalid_argument("direct: at most 65534 shading samples per camera sample");
    }
    if (p->sampler > PHIP_SAMPLER_HAMMERSLEY) throw std::invalid_argument("unknown sampler kind");
    if (p->sampler == PHIP_SAMPLER_HALTON || p->sampler == PHIP_SAMPLER_HAMMERSLEY) {
        const char *name = p->sampler == PHIP_SAMPLER_HALTON ? "PHIP_SAMPLER_HALTON" : "PHIP_SAMPLER_HAMMERSLEY";
        /* `direct`: more than one sample of a kind is a requested sample array -- hammersley has none (hammersley.cpp:293-300: Log(EError)) */
        if (direct && p->sampler == PHIP_SAMPLER_HAMMERSLEY && (p->emitter_samples > 1 || p->bsdf_samples > 1))
            throw std::invalid_argument("PHIP_SAMPLER_HAMMERSLEY: request2DArray(): Not supported for the Hammersley QMC sequence! With `direct`, emitterSamples and bsdfSamples must be at most 1");
        if (!p->qmc_primes || p->qmc_dimensions < 8 || p->qmc_dimensions > 1024) throw std::invalid_argument(std::string(name) + ": qmc_primes / qmc_dimensions (the reference's prime table, 8 .. 1024 entries) are required");
        if (p->qmc_primes[0] != 2 || p->qmc_primes[1] != 3) throw std::invalid_argument(std::string(name) + ": qmc_primes must start 2, 3 (the pixel enumeration is over those bases)");
        for (uint32_t d = 0; d < p->qmc_dimensions; ++d) if (p->qmc_primes[d] < 2 || p->qmc_primes[d] > 65535u) throw std::invalid_argument(std::string(name) + ": qmc_primes out of range");
        if (p->qmc_permutations) {
            if (p->qmc_permutations[0] > 1 || p->qmc_permutations[1] > 1 || p->qmc_permutations[0] == p->qmc_permutations[1]) throw std::invalid_argument(std::string(name) + ": qmc_permutations does not start with a permutation of {0, 1}");
            if (p->qmc_permutations[2] > 2 || p->qmc_permutations[3] > 2 || p->qmc_permutations[4] > 2) throw std::invalid_argument(std::string(name) + ": the permutation of base 3 is not one of {0, 1, 2}");
        }
        if (!direct && p->rr_depth < 2) throw std::invalid_argument(std::string(name) + ": rrDepth must be at least 2 (the dimension bookkeeping of halton.cpp:364-366 is restated for that case)");
        /* (a crop window anywhere on the film: the image blocks, and with them the pixel positions the sampler's generate() sees, are relative to the crop
           window -- renderproc.cpp:163-164 starts them at (0, 0) -- so the crop offset never reaches the sequence: nothing to restate, nothing to refuse) */
        const unsigned long long n = (unsigned long long) (p->sample_total > 0 ? p->sample_total : p->spp);
        if (n >= (1ull << 17)) throw std::invalid_argument(std::string(name) + ": at most 131071 samples per pixel (32-bit pixel offsets)");
    }
    if (p->sampler == PHIP_SAMPLER_SOBOL || p->sampler == PHIP_SAMPLER_STRATIFIED) {
        const DevScene &D0 = sc->devs[0]->dev;
        if (p->sampler == PHIP_SAMPLER_SOBOL) {
            if (!p->sobol_matrices || p->sobol_dimensions < 8) throw std::invalid_argument("PHIP_SAMPLER_SOBOL: sobol_matrices / sobol_dimensions (the reference plugin's direction numbers) are required");
            if (p->sobol_log_resolution > 26) throw std::invalid_argument("PHIP_SAMPLER_SOBOL: sobol_log_resolution out of range");
            if (!direct && p->rr_depth < 2) throw std::invalid_argument("PHIP_SAMPLER_SOBOL: rrDepth must be at least 2 (the dimension bookkeeping of sobol.cpp:241-242 is restated for that case)");
            if (direct && (p->emitter_samples > 1 || p->bsdf_samples > 1) && p->sobol_log_resolution < 2)
                throw std::invalid_argument("PHIP_SAMPLER_SOBOL: sample arrays of `direct` need a film of more than two pixels per side (SobolSampler::generate enumerates them per pixel: sobol.cpp:182,190)");
            if (p->sobol_log_resolution > 1 && (!p->sobol_vdc || !p->sobol_vdc_inv)) throw std::invalid_argument("PHIP_SAMPLER_SOBOL: sobol_vdc / sobol_vdc_inv are required when the film is enumerated per pixel");
            uint32_t need = 0; { uint32_t side = (uint32_t) std::max(D0.film.width, D0.film.height), r = 1; while (r < side) { r <<= 1; ++need; } }
            if (p->sobol_log_resolution != need) throw std::invalid_argument("PHIP_SAMPLER_SOBOL: sobol_log_resolution must be log2 of the crop window's larger side rounded up to a power of two (sobol.cpp:147-157)");
        } else {
            const unsigned n = (unsigned) (p->sample_total > 0 ? p->sample_total : p->spp);
            unsigned r = 1; while (r * r < n) ++r;
            if (r * r != n) throw std::invalid_argument("PHIP_SAMPLER_STRATIFIED: the sample count of the render must be a perfect square (stratified.cpp:64-72 rounds it up)");
        }
    }
    if (p->sampler == PHIP_SAMPLER_LD) {
        const unsigned n = (unsigned) (p->sample_total > 0 ? p->sample_total : p->spp);
        if (n == 0 || (n & (n - 1))) throw std::invalid_argument("PHIP_SAMPLER_LD: the sample count of the render must be a power of two (ldsampler.cpp:83-87)");
        if (p->integrator == PHIP_INTEGRATOR_DIRECT && (unsigned long long) n * (unsigned) std::max(p->emitter_samples, p->bsdf_samples) > 0x7fffffffull)
            throw std::invalid_argument("PHIP_SAMPLER_LD: sample array too long");
    }
    if (p->sample_offset < 0 || p->sample_total < 0) throw std::invalid_argument("sample_offset / sample_total must not be negative");
    if (p->sample_total != 0 && (long long) p->sample_offset + p->spp > p->sample_total) throw std::invalid_argument("sample_offset + spp exceeds sample_total");
    if ((p->flags & PHIP_FLAG_SAMPLE_BUFFER) && (p->flags & PHIP_FLAG_ACCUMULATE))
        throw std::invalid_argument("PHIP_FLAG_SAMPLE_BUFFER holds the samples of one call: not with PHIP_FLAG_ACCUMULATE");
    if (sc->devs[0]->dev.env.w > 0 && sc->envLevelCount <= 1 && !p->hide_emitters && !(p->flags & PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND))
        throw std::invalid_argument("envmap without MIP levels: directly visible background needs the filtered (EWA) lookup of envmap.cpp:395-407: "
                                    "pass the pyramid, render with hideEmitters or set PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND");
    const int bs = p->block_size > 0 ? p->block_size : 32;
    if (bs < 2 || bs > 128 || (bs & (bs - 1))) throw std::invalid_argument("block_size must be a power of two in [2,128] (mitsuba.cpp:233-239 allows 2..128)");
    if (bs < sc->devs[0]->dev.film.border) throw std::invalid_argument("The block size must be larger than the image reconstruction filter radius!"); /* renderproc.cpp:175-176 */
    const int shardCount = p->shard_count > 0 ? p->shard_count : 1;
    if (p->shard_index < 0 || p->shard_index >= shardCount) throw std::invalid_argument("shard_index out of range");
    if (p->n_devices < 0 || p->n_devices > PHIP_MAX_DEVICES) throw std::invalid_argument("n_devices out of range");
    if (p->n_devices > 1 && p->stream) throw std::invalid_argument("a caller's stream belongs to one device: leave `stream` NULL when n_devices > 1 (every device renders on a stream of the library)");
}

/* The work counters of `a` added to `t`: samples, rays, vertices, node visits and triangle tests (a pass into its job, a device into the call) */
static void addWork(phip_stats &t, const phip_stats &a) {
    t.samples += a.samples; t.closest_rays += a.closest_rays; t.shadow_rays += a.shadow_rays; t.path_vertices += a.path_vertices;
    t.closest_node_visits += a.closest_node_visits; t.closest_triangle_tests += a.closest_triangle_tests;
    t.shadow_node_visits += a.shadow_node_visits; t.shadow_triangle_tests += a.shadow_triangle_tests;
}

/* The fused kernel for one render call: whether it runs, in which traversal form, and its resident grid */
struct FusedPlan {
    bool on = false;                        /* the passes run on k_mega -- until one of them gives up */
    int flat = 0; bool wide = false;        /* k_mega's traversal form (k_mega.h); >= 4: the 8-wide tree in memory */
    bool strictNormals = false;
    MegaKernel kernel = nullptr;            /* the build of k_mega for the render's materials, traversal form, sampler and integrator (megaKernelOf) */
    int perCU = 0; uint32_t nodeCache = 0; size_t lds = 0;
    dim3 grid = dim3(1); MegaParams M;
#if MEGA_MB_FAULT
    uint32_t faultWaves = 0; int faultPass = -1;
#endif
};

/* The wavefront kernels for one render call (set up only when that path runs): pool, kernel choice, grids */
struct WavefrontPlan {
    bool shadeTrace = false;                /* k_shade_trace / k_shade_trace_w: the vertex kernel traces both rays of the iteration itself */
    bool wideTrace = false;                 /* ... on the 8-wide tree in memory (k_shade_trace_w: a persistent grid; a wave whose task stack overflows gives the pass up) */
    /* the vertex kernel of the iterations, its grid and dynamic LDS (selectVertexKernel): k_shade, k_shade_direct or k_shade_trace with a thread per slot, or -- with
       wideTrace -- k_shade_trace_w, a persistent grid that stages traceNodeCache nodes */
    ShadeKernel vertex = nullptr; ShadeTraceWideKernel vertexWide = nullptr;
    ShadeRaysKernel vertexRays = nullptr; RaySamples rays = { nullptr, nullptr, 0u, 0u };     /* phip_radiance_device: k_shade_r in k_shade's place, and the caller's ray array (host_radiance.h) */
    dim3 vertexGrid = dim3(1); size_t vertexLds = 0; uint32_t traceNodeCache = 0;
    uint32_t capacity = 0, nWaves = 0, nBlocks = 0;
    int feat = 0;                           /* FEAT of the shading kernels: 1 environment emitter, 2 bitmap textures, 8 the QMC samplers */
    size_t wideLds = 0;
    dim3 pgridRays = dim3(1);
};

/* One device's share of one render call: what the stages of renderOnDevice hand to each other */
struct RenderJob {
    phip_scene *sc; SceneDev &sd; const phip_render_params *p; float *dOut;
    hipStream_t stream = nullptr;
    DevScene D;                             /* sd.dev with this call's block size */
    int bs, W, H, tileShift = 0, tilesX, nCU = 256;
    bool direct, timing, keepSamples, rinv, qmc, keepJitter = false;
    uint32_t sppPerPass = 0; unsigned long long idsPerSpp = 0;
    FusedPlan F; WavefrontPlan wf;
    PathPool P;                             /* the wavefront pool; a fused pass sets its statistics rows only (k_reduce_stats) */
    RenderConst rc;                         /* of the call, then of the pass that is running */
    EventList evTrace, evShade, evFilm, evFused;
    Counters hc; phip_stats st;
    unsigned long long samplesDone = 0;     /* samples of the passes that are in the film already */
    bool cancelled = false;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();

    RenderJob(phip_scene *sc, SceneDev &sd, const phip_render_params *p, float *dOut) : sc(sc), sd(sd), p(p), dOut(dOut), D(sd.dev) {
        bs = p->block_size > 0 ? p->block_size : 32;
        D.film.blockSize = bs;
        W = D.film.width; H = D.film.height; tilesX = (W + bs - 1) / bs;
        while ((1 << tileShift) < bs) ++tileShift;
        direct = p->integrator == PHIP_INTEGRATOR_DIRECT;
        timing = (p->flags & PHIP_FLAG_KERNEL_TIMING) != 0;
        keepSamples = (p->flags & PHIP_FLAG_SAMPLE_BUFFER) != 0;
        rinv = p->sampler == PHIP_SAMPLER_HALTON || p->sampler == PHIP_SAMPLER_HAMMERSLEY;
        qmc = p->sampler == PHIP_SAMPLER_SOBOL || p->sampler == PHIP_SAMPLER_STRATIFIED || rinv;     /* served by the wavefront kernels compiled with FEAT bit 3 */
        memset(&F.M, 0, sizeof(F.M)); memset(&P, 0, sizeof(P)); memset(&rc, 0, sizeof(rc)); memset(&hc, 0, sizeof(hc)); memset(&st, 0, sizeof(st));
    }
    uint32_t sampleTotal() const { return (uint32_t) (p->sample_total > 0 ? p->sample_total : p->spp); }     /* samples per pixel of the whole render, of which this call may be a part */
    void progress(unsigned long long done) {
        if (!p->progress) return;
        std::lock_guard<std::mutex> g(sc->progressLock);
        p->progress(p->progress_user, sd.device, done, sd.localPixels * (unsigned long long) p->spp);
    }
};

/* tile -> shard assignment in the reference's spiral order (cached between calls with the same layout) */
static void shardTiles(RenderJob &J, int shardIndex, int shardCount) {
    SceneDev &sd = J.sd;
    const int bs = J.bs, W = J.W, H = J.H, tilesX = J.tilesX, tilesY = (H + bs - 1) / bs;
    if (sd.tileKey[0] == bs && sd.tileKey[1] == shardIndex && sd.tileKey[2] == shardCount) return;
    std::vector<std::pair<int, int>> spiral;
    spiralBlocks(W, H, bs, spiral);
    std::vector<int32_t> tileSlot((size_t) tilesX * tilesY, -1);
    std::vector<uint32_t> tileOrigin;
    for (size_t i = 0; i < spiral.size(); ++i) {
        if ((int) (i % (size_t) shardCount) != shardIndex) continue;
        tileSlot[(size_t) spiral[i].second * tilesX + spiral[i].first] = (int32_t) tileOrigin.size();
        tileOrigin.push_back((uint32_t) (spiral[i].first * bs) | ((uint32_t) (spiral[i].second * bs) << 16));
    }
    sd.nLocalTiles = (uint32_t) tileOrigin.size();
    sd.localPixels = 0;
    for (uint32_t o : tileOrigin) sd.localPixels += (unsigned long long) std::min(bs, W - (int) (o & 0xFFFFu)) * std::min(bs, H - (int) (o >> 16));
    if (tileOrigin.empty()) sd.tileOrigin.alloc(1);
    else sd.tileOrigin.upload(tileOrigin.data(), tileOrigin.size());
    sd.tileSlot.upload(tileSlot.data(), tileSlot.size());
    sd.tileKey[0] = bs; sd.tileKey[1] = shardIndex; sd.tileKey[2] = shardCount;
}

/* passes: bound the per-sample buffer (16 B per sample id; 24 B with the jitter the sequence samplers keep for the film pass).  idsPerSpp: the sample ids one sample
   per pixel takes -- the pixels of this device's blocks, or the rays of phip_radiance_device */
static void planPasses(RenderJob &J, unsigned long long idsPerSpp) {
    SceneDev &sd = J.sd; const phip_render_params *p = J.p;
    J.keepJitter = (p->sampler == PHIP_SAMPLER_SOBOL || p->sampler == PHIP_SAMPLER_HALTON || p->sampler == PHIP_SAMPLER_HAMMERSLEY);
    const unsigned long long maxIdsPerPass = (1ull << 32) - 1;                 /* sample ids are 32-bit in the slot state */
    unsigned long long budgetIds = (24ull << 30) / (J.keepJitter ? 24 : 16);  /* 24 GiB of sample buffer */
    if (const char *e = getenv("PHIP_MAX_PASS_SAMPLES")) budgetIds = std::max(1ull, strtoull(e, nullptr, 10));   /* test hook: force several passes */
    J.idsPerSpp = idsPerSpp;
    J.sppPerPass = (uint32_t) p->spp;
    if (J.idsPerSpp > 0) {
        unsigned long long cap = std::min(maxIdsPerPass, budgetIds) / J.idsPerSpp;
        if (cap < 1) cap = 1;
        J.sppPerPass = (uint32_t) std::min<unsigned long long>(cap, (unsigned long long) p->spp);
    }
    const unsigned long long idsFirstPass = J.idsPerSpp * J.sppPerPass;
    if (sd.L.n < idsFirstPass) sd.L.alloc((size_t) idsFirstPass);
    if (J.keepJitter && sd.jitter.n < idsFirstPass) sd.jitter.alloc((size_t) idsFirstPass);
}

/* PHIP_SAMPLER_SOBOL: the plugin's tables, uploaded once per content: ~210 KB of direction numbers + the two 52-word enumeration rows */
static void uploadSobolTables(RenderJob &J) {
    SceneDev &sd = J.sd; const phip_render_params *p = J.p;
    const size_t nm = (size_t) p->sobol_dimensions * PHIP_SOBOL_MATRIX_SIZE;
    /* (keyed by CONTENT: the tables are host pointers "read during the call" -- a caller may refill or reallocate them at the same address) */
    uint64_t key = contentHash(p->sobol_matrices, nm * sizeof(uint32_t), 0x9E3779B97F4A7C15ull);
    if (p->sobol_log_resolution > 1) { key = contentHash(p->sobol_vdc, PHIP_SOBOL_MATRIX_SIZE * sizeof(uint64_t), key); key = contentHash(p->sobol_vdc_inv, PHIP_SOBOL_MATRIX_SIZE * sizeof(uint64_t), key); }
    if (sd.sobolKey == key && sd.sobolMat.n == nm && sd.sobolLogRes == p->sobol_log_resolution) return;
    sd.sobolMat.upload(p->sobol_matrices, nm);
    std::vector<unsigned long long> v(2 * PHIP_SOBOL_MATRIX_SIZE, 0ull);
    if (p->sobol_log_resolution > 1)
        for (int i = 0; i < PHIP_SOBOL_MATRIX_SIZE; ++i) { v[i] = p->sobol_vdc[i]; v[PHIP_SOBOL_MATRIX_SIZE + i] = p->sobol_vdc_inv[i]; }
    sd.sobolVdc.upload(v.data(), v.size());
    std::vector<uint32_t> bt; std::vector<unsigned long long> vb;
    buildSobolByteTables(p->sobol_matrices, (size_t) p->sobol_dimensions, v.data(), bt, vb);
    sd.sobolBt.upload(bt.data(), bt.size()); sd.sobolVdcBt.upload(vb.data(), vb.size());
    sd.sobolKey = key; sd.sobolLogRes = p->sobol_log_resolution;
}

/* PHIP_SAMPLER_HALTON / _HAMMERSLEY: primes + permutations, keyed by content (at most ~200 KB; see the Sobol tables above) */
static void uploadRinvTables(RenderJob &J) {
    SceneDev &sd = J.sd; const phip_render_params *p = J.p;
    std::vector<uint32_t> off(p->qmc_dimensions);
    size_t total = 0;
    for (uint32_t d = 0; d < p->qmc_dimensions; ++d) { off[d] = (uint32_t) total; total += p->qmc_primes[d]; }
    uint64_t rinvKey = contentHash(p->qmc_primes, p->qmc_dimensions * sizeof(uint32_t), p->qmc_permutations ? 0x51ED270B7A5F1D3Bull : 0x2545F4914F6CDD1Dull);
    if (p->qmc_permutations) rinvKey = contentHash(p->qmc_permutations, total * sizeof(uint16_t), rinvKey);
    if (sd.rinvKey == rinvKey && sd.rinvPrimes.n == p->qmc_dimensions) return;
    /* primes, the start of every base's permutation, the permutations themselves; the inverse permutations of bases 2 and 3 (the pixel enumeration) */
    sd.rinvPrimes.upload(p->qmc_primes, p->qmc_dimensions); sd.rinvOffsets.upload(off.data(), off.size());
    sd.rinvInvPerm2 = 0x4u; sd.rinvInvPerm3 = 0x24u;
    if (p->qmc_permutations) {
        sd.rinvPerm.upload(p->qmc_permutations, total);
        const uint16_t *p2 = p->qmc_permutations, *p3 = p->qmc_permutations + 2;
        sd.rinvInvPerm2 = sd.rinvInvPerm3 = 0;
        for (uint32_t i = 0; i < 2; ++i) sd.rinvInvPerm2 |= i << (2u * p2[i]);          /* invPerm[perm[i]] = i (faure.cpp: invertPermutation) */
        for (uint32_t i = 0; i < 3; ++i) sd.rinvInvPerm3 |= i << (2u * p3[i]);
    }
    std::vector<uint32_t> di, ch, pw; std::vector<float> fc;
    sd.rinvTabDims = buildRinvTables(p->qmc_primes, p->qmc_permutations, off.data(), p->qmc_dimensions, di, ch, fc, pw);
    if (sd.rinvTabDims) { sd.rinvDimInfo.upload(di.data(), di.size()); sd.rinvChunk.upload(ch.data(), ch.size()); sd.rinvFac.upload(fc.data(), fc.size()); sd.rinvPw.upload(pw.data(), pw.size()); }
    sd.rinvKey = rinvKey;
}

/* which device path: the fused kernel when the scene fits its LDS plan (decided at scene creation) and a block of it fits a compute unit for THIS render */
static void planFused(RenderJob &J) {
    phip_scene *sc = J.sc; SceneDev &sd = J.sd; const phip_render_params *p = J.p; FusedPlan &F = J.F;
    /* (the fused kernel on the 8-wide tree: by default where it is faster than the wavefront kernels -- trees that live in L2, DESIGN.md 3.9 -- with PHIP_FLAG_FUSED_ANY wherever it can run) */
    const bool wideFused = sc->fusedWide && (sc->bvh.nWNodes <= PHIP_FUSED_WIDE_MAX_NODES || (p->flags & PHIP_FLAG_FUSED_ANY));
    F.on = (sc->fitsLds || wideFused) && !(p->flags & (PHIP_FLAG_NO_FUSED | PHIP_FLAG_NO_MEGA));
    F.flat = sc->fitsLds ? (J.D.nFlatLeaves ? (int) J.D.flatMode : 0) : sc->fusedWide;
    if (J.direct && F.flat < 2) F.on = false;      /* (round 6: `direct` rides the fused kernel too -- k_mega<.., DIRECT>, on the packed leaf tables and on the tree in memory) */
    F.wide = F.flat >= 4;
    F.strictNormals = !J.direct && p->strict_normals != 0;
    F.kernel = megaKernelOf(J.direct, F.flat, sc->materialMask, F.strictNormals, J.qmc);
    /* resident blocks of the fused kernel for THIS render (the QMC build has ~15 KB more static LDS than the plan of fitsLds priced at scene
       creation): when none fits a compute unit the render runs on the wavefront kernels, as it did before the samplers moved to k_mega */
    if (F.on) {
        if (F.wide) {
            /* the top of the tree every block stages (BFS order) */
            F.nodeCache = std::min<uint32_t>(sc->bvh.nWNodes, MEGA_WIDE_NODE_CACHE);
            const bool mailbox = false;     /* (the mailboxes' LDS would cost the tree-in-memory builds the fourth block of a CU: k_mega.h) */
            F.lds = megaWidePoolLdsBytesOf(J.D, F.nodeCache, mailbox, F.flat == 4, MB_DW * MB_NS * sizeof(uint32_t));
        } else {
            F.lds = megaLdsBytesOf(J.D);
        }
        /* (no build for the form, a refused LDS limit, a failed query, no resident block: all the same to this path) */
        const Residency r = F.kernel ? residentBlocksPerCU((const void *) F.kernel, BLOCK, F.lds) : Residency{ hipSuccess, 0 };
        F.perCU = std::min(MEGA_WAVES, r.blocks);
        if (F.perCU <= 0) F.on = false;
        if (getenv("PHIP_DEBUG_TIMING")) fprintf(stderr, "[phip] k_mega (traversal form %d): %d blocks per CU with %zu bytes of dynamic LDS\n", F.flat, F.perCU, F.lds);
    }
    sd.fused = F.on;
    /* ... or k_shade_trace: the scene's tree is the packed leaf table, but k_mega does not serve it (glass / copper / textures / environment emitter) */
    J.wf.shadeTrace = !F.on && (sc->flatTrace || sc->flatTraceToo) && !J.direct && !(p->flags & PHIP_FLAG_NO_FUSED);
    /* ... or k_shade_trace_w: the same iterations on the 8-wide tree in memory, by default where they are faster than k_shade + k_rays_w -- measured: nowhere by more than the
       step spread, PHIP_SHADE_TRACE_WIDE_MAX_NODES is 0 -- with PHIP_FLAG_FUSED_ANY wherever they can run.  (PHIP_FLAG_NO_MEGA keeps k_mega off a scene of its
       tree-in-memory builds: with both flags such a scene ends here.) */
    J.wf.wideTrace = !F.on && sc->wideTrace && (sc->bvh.nWNodes <= PHIP_SHADE_TRACE_WIDE_MAX_NODES || (p->flags & PHIP_FLAG_FUSED_ANY)) && !J.direct && !(p->flags & PHIP_FLAG_NO_FUSED);
    J.wf.shadeTrace = J.wf.shadeTrace || J.wf.wideTrace;
    if (!F.on) return;

    /* resident grid and per-wave statistics rows */
    MegaParams &M = F.M;
    F.grid = dim3((unsigned) (J.nCU * F.perCU));
    M.nWaves = F.grid.x * (BLOCK / 64);
    if (sd.stat.n < (size_t) ST_COUNT * M.nWaves) sd.stat.alloc((size_t) ST_COUNT * M.nWaves);
    M.stat = sd.stat.p; M.nextId = sd.megaNext.p;
    M.nodeCache = F.nodeCache; M.spill = nullptr;
    if (F.wide) {     /* the group stacks' overflow behind their six LDS entries: the buffer always covers the grid, as for k_rays_w (a silent out-of-bounds write otherwise) */
        const size_t spillLanes = (size_t) F.grid.x * BLOCK;
        if (sd.spill.n < spillLanes * SPILL_DEPTH) sd.spill.alloc(spillLanes * SPILL_DEPTH);
        M.spill = sd.spill.p;
    }
    int *dflag = nullptr; HIP_TRY(hipHostGetDevicePointer((void **) &dflag, sc->cancelFlag, 0));
    M.cancel = dflag;
#if MEGA_MB_FAULT
    /* fault-injection build (tests/test_gpu_parity.py), read at every call: PHIP_TEST_FAULT_WAVES = wave0 (the default) | block (the four waves of block 0) | all | none
       report that they gave up, in pass PHIP_TEST_FAULT_PASS of the call (default: every pass); PHIP_TEST_FAULT_SHORT = 1: they also under-report one sample each,
       2: they only under-report (the host's exact count must catch it) */
    {
        const char *w = getenv("PHIP_TEST_FAULT_WAVES"), *sh = getenv("PHIP_TEST_FAULT_SHORT");
        F.faultWaves = !w || !strcmp(w, "wave0") ? 1u : !strcmp(w, "block") ? 2u : !strcmp(w, "all") ? 3u : 0u;
        F.faultPass = getenv("PHIP_TEST_FAULT_PASS") ? atoi(getenv("PHIP_TEST_FAULT_PASS")) : -1;
        M.faultShort = sh ? (uint32_t) atoi(sh) : 0u;
    }
#endif
    J.P.stat = sd.stat.p; J.P.nWaves = M.nWaves;               /* k_reduce_stats reads these two */
}

/* The vertex kernel of the wavefront iterations, resolved once: k_shade_trace_w where the render wishes it (wideTrace) and a block of it is resident, else
   k_shade_trace where it wishes that (shadeTrace), else k_shade -- or k_shade_direct.  Sets the two flags to what was resolved; a pass that k_shade_trace_w gave up
   comes here again for k_shade (renderOnDevice) */
static void selectVertexKernel(RenderJob &J, bool shadeTrace, bool wideTrace) {
    phip_scene *sc = J.sc; WavefrontPlan &wf = J.wf;
    const bool strictNormals = J.p->strict_normals != 0;
    wf.vertex = nullptr; wf.vertexWide = nullptr;
    /* k_shade_trace_w: persistent -- its resident set as the runtime counts it, walking the pool's blocks of slots.  Its waves' task stacks spill into the buffer that
       covers k_rays_w's grid (setupWavefront: up to 8 blocks of 256 lanes per CU, SPILL_DEPTH words per lane), so the grid is held to the lanes that buffer has: no
       allocation of its own, nothing new for the pool's memory fit to price.  No resident block (an LDS plan the device refuses, a failed query): the wavefront kernels run */
    if (wideTrace) {
        wf.traceNodeCache = std::min<uint32_t>(sc->bvh.nWNodes, MEGA_WIDE_NODE_CACHE);
        wf.vertexLds = shadeTraceWideLdsBytes(wf.traceNodeCache, (sc->materialMask & MM_ALL) != 0);
        wf.vertexWide = shadeTraceWideKernelOf(wf.feat, strictNormals, sc->materialMask);
        const int perCU = residentBlocksPerCU((const void *) wf.vertexWide, BLOCK, wf.vertexLds).blocks;
        const size_t blocks = std::min<size_t>({ (size_t) J.nCU * (size_t) std::max(perCU, 0), (size_t) wf.capacity / BLOCK, (size_t) J.P.spillLanes / BLOCK });
        if (getenv("PHIP_DEBUG_TIMING")) fprintf(stderr, "[phip] k_shade_trace_w: %d blocks per CU with %zu bytes of dynamic LDS, grid %zu\n", perCU, wf.vertexLds, blocks);
        if (blocks == 0) { wf.vertexWide = nullptr; wideTrace = shadeTrace = false; }
        else wf.vertexGrid = dim3((unsigned) blocks);
    }
    wf.wideTrace = wideTrace; wf.shadeTrace = shadeTrace || wideTrace;
    if (wf.vertexWide) return;
    wf.vertex = shadeKernelOf(wf.feat, J.direct, wf.shadeTrace, strictNormals, sc->materialMask, shadeTableSet(wf.feat, J.D));
    wf.vertexGrid = dim3((wf.capacity + BLOCK - 1) / BLOCK);
    wf.vertexLds = wf.shadeTrace ? shadeTraceLdsBytes(J.D) : 0;        /* (k_shade_trace: the packed leaf table, the records and the tables it stages) */
}

/* The wavefront path's kernels and grids, for the pool of setupWavefront */
static void setupWavefrontGrids(RenderJob &J) {
    phip_scene *sc = J.sc; WavefrontPlan &wf = J.wf;
    const DevScene &D = J.D; const uint32_t capacity = wf.capacity; const int nCU = J.nCU;
    /* environment emitter, bitmap textures; 8: the QMC samplers (two builds: the plain one, and one with both other features) */
    const int feat0 = (D.envEmitter >= 0 ? 1 : 0) | (sc->hasTextures ? 2 : 0);
    wf.feat = J.qmc ? (feat0 ? 11 : 8) : feat0;
    /* k_rays_w: blocks of WIDE_BLOCK threads with their own LDS plan.  The grid of a persistent kernel is exactly its resident set.  Residency is asked
       of the runtime (registers, the block's static + dynamic LDS and the LDS allocation granule all enter) -- an arithmetic estimate that is one block
       per CU too high makes the surplus blocks wait for a resident one to finish: a second round that doubled the ray kernel's time when the LDS node
       cache grew to 7.5 KB (round 2). */
    wf.wideLds = wideLdsBytes(D.wideNodeCache, WIDE_BLOCK) + wideDealBytes(WIDE_BLOCK);
    const Residency rays = residentBlocksPerCU((const void *) k_rays_w, WIDE_BLOCK, wf.wideLds);
    if (rays.limit != hipSuccess) throw std::runtime_error(std::string("k_rays_w: hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize): ") + hipGetErrorString(rays.limit));
    int n = rays.blocks > 0 ? rays.blocks : 1;
    n = std::min(n, WIDE_WAVES * 256 / WIDE_BLOCK);
    if (n <= 0) n = 1;
    wf.pgridRays = dim3((unsigned) std::max(1, std::min<int>(nCU * n, (int) ((capacity + WIDE_BLOCK - 1) / WIDE_BLOCK))));
    /* k_rays_w draws its chunks from sharded counters */
    if (J.sd.drawCounters.n < 2 * RAY_SHARDS * RAY_SHARD_STRIDE) J.sd.drawCounters.alloc(2 * RAY_SHARDS * RAY_SHARD_STRIDE);
    selectVertexKernel(J, wf.shadeTrace, wf.wideTrace);     /* (as planFused wished) */
}

/* The wavefront path's pool, sized for a first pass of idsFirstPass sample ids and for the memory that is free now; then its kernels and grids */
static void setupWavefront(RenderJob &J, unsigned long long idsFirstPass) {
    SceneDev &sd = J.sd; WavefrontPlan &wf = J.wf; PathPool &P = J.P;
    /* pool size: large enough that per-launch fixed costs vanish, small enough that the tail (slots
       running dry at the end of a pass) stays a small fraction of the pass (measured: 4M / 8M slots) */
    /* (round 3) Every launch of the persistent ray kernel ends with a drain in which each wave waits for its longest ray while the
       work queue is empty: ~0.15 ms per launch on the 250 k-triangle scenes, 14 % of a launch over 4 M slots, 7 % over 8 M.  A bigger
       pool means fewer, longer launches: atrium 1920x1080x64 spp 427 / 454 / 470 / 470 Msamples/s with 4 / 8 / 16 / 32 M slots, the
       glass room at 512 spp 480 / 496 / 505 with 8 / 16 / 32 M -- so the pool grows with the job (about 0.14 KB of HBM per slot). */
    /* (round 4, after the ray kernel's triangle rounds: 8 / 16 / 32 / 64 M slots on the 4K slice (531 M ids) 610 / 636 / 646 / 657 Msamples/s, C4 at 512 spp (1062 M ids)
       flat at 64 M and -2 % at 128 M, C3 (133 M ids) flat from 16 M on: jobs of more than 256 M ids get 64 M slots) */
    /* (round 5: k_shade_trace has no persistent ray kernel whose drain a big pool amortises -- what a big pool costs it is the tail of the pass, the launches
       in which the long paths of a few slots finish: mixed Cornell box at 256 spp with 1 / 2 / 4 / 8 / 16 M slots 1518 / 1617 / 1643 / 1596 / 1450 Msamples/s,
       profiles/r05_gpu_call_e_*) */
    const unsigned long long poolCap = wf.shadeTrace ? (1ull << 22)
                                     : idsFirstPass > (256ull << 20) ? (1ull << 26) : idsFirstPass >= (64ull << 20) ? (1ull << 24)
                                     : idsFirstPass >= (16ull << 20) ? (1ull << 23) : (1ull << 22);
    uint32_t capacity = (uint32_t) std::min<unsigned long long>(std::max<unsigned long long>(idsFirstPass, BLOCK), poolCap);
    {   /* ... and with the memory that is there: the pool's state is ~144 B per slot; it may take a quarter of what is free now (a shared or partitioned GPU, n_devices replicas), never less than the 4 M slots
           every job ran with before the pool grew */
        size_t freeB = 0, totalB = 0;
        if (sd.rayO.n < capacity && hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
            unsigned long long fit = (unsigned long long) (freeB / 4) / 144ull;
            while (capacity > (1u << 22) && capacity > fit) capacity >>= 1;
        }
    }
    capacity = (capacity + BLOCK - 1) / BLOCK * BLOCK;
    const size_t laneCap = ((size_t) capacity + WIDE_BLOCK - 1) / WIDE_BLOCK * WIDE_BLOCK;      /* k_rays_w runs whole blocks of WIDE_BLOCK lanes */
    const uint32_t nWaves = (uint32_t) (laneCap / 64), nBlocks = capacity / BLOCK;
    if (sd.rayO.n < capacity) {
        sd.rayO.alloc(capacity); sd.rayD.alloc(capacity); sd.hit.alloc(capacity); sd.thr.alloc(capacity);
        sd.mis.alloc(capacity); sd.info.alloc(capacity); sd.state.alloc(capacity); sd.shadow.alloc(3 * (size_t) capacity);
        sd.shadowCount.alloc(nBlocks); sd.blockDead.alloc(nBlocks); sd.blockShard.alloc(nBlocks);
    }
    {   /* traversal-stack overflow: SPILL_DEPTH words per LANE of the ray kernel.  The wide tree is only walked by persistent grids (at most 8 resident
           blocks of 256 per CU): the buffer always covers the whole grid, also when the tree's depth says that no lane can reach it -- 200 MB of 288 GB
           against a silent out-of-bounds write should that hand-derived bound ever be off */
        const size_t spillLanes = std::min<size_t>(laneCap, (size_t) J.nCU * 8 * 256);
        if (sd.spill.n < spillLanes * SPILL_DEPTH) sd.spill.alloc(spillLanes * SPILL_DEPTH);
        P.spillLanes = (uint32_t) std::min<size_t>(sd.spill.n / SPILL_DEPTH, 0xFFFFFFFFu);
    }
    if (sd.stat.n < (size_t) ST_COUNT * nWaves) sd.stat.alloc((size_t) ST_COUNT * nWaves);
    if (J.direct && sd.camHit.n < capacity) sd.camHit.alloc(capacity);
    P.camHit = sd.camHit.p;
    P.rayO = sd.rayO.p; P.rayD = sd.rayD.p; P.hit = sd.hit.p; P.thr = sd.thr.p; P.mis = sd.mis.p; P.info = sd.info.p; P.state = sd.state.p;
    P.shadow = sd.shadow.p; P.shadowCount = sd.shadowCount.p; P.blockDead = sd.blockDead.p; P.stat = sd.stat.p; P.spill = sd.spill.p; P.capacity = capacity; P.nWaves = nWaves;
    J.rc.blockShard = sd.blockShard.p;
    wf.capacity = capacity; wf.nWaves = nWaves; wf.nBlocks = nBlocks;
    setupWavefrontGrids(J);
}

/* HaltonSampler / HammersleySampler::setFilmResolution(res, blocked = true): the partition of the sequence over the pixels */
static void rinvFilmResolution(RinvTab &T, bool halton, const uint32_t res[2]) {
    if (halton) {
        /* halton.cpp:244-266 */
        T.hammersley = 0; T.stride = 1;
        uint32_t pw[2], ex[2];
        for (int i = 0; i < 2; ++i) {
            const uint32_t prime = i ? 3u : 2u; uint32_t value = 1, e = 0;
            while (value < std::min(res[i], RINV_MAX_RESOLUTION)) { value *= prime; ++e; }
            pw[i] = value; ex[i] = e; T.stride *= value;
        }
        T.powX = pw[0]; T.powY = pw[1]; T.expX = ex[0]; T.expY = ex[1];
        /* multiplicativeInverse(a, n): x with a x = 1 (mod n), in 0 .. n - 1 (halton.cpp:214-241; n = 1 gives 0) */
        auto inverse = [](uint32_t a, uint32_t n) { for (uint32_t x = 0; x < n; ++x) if ((unsigned long long) a * x % n == 1u % n) return x; return 0u; };
        T.multInvX = inverse(T.powY, T.powX); T.multInvY = inverse(T.powX, T.powY);
    } else {
        /* hammersley.cpp:181-196 */
        T.hammersley = 1;
        uint32_t r[2];
        for (int i = 0; i < 2; ++i) { uint32_t v = 1; while (v < res[i]) v <<= 1; r[i] = std::min(RINV_MAX_RESOLUTION, v); }
        T.powX = r[0]; T.powY = r[1]; T.expX = 0; T.expY = 0; while ((1u << T.expY) < r[1]) ++T.expY;
        T.stride = r[1];
        T.factor = 1.0f / (float) ((size_t) T.sampleCount * (size_t) r[0] * (size_t) r[1]);
    }
}

/* The RenderConst fields that hold for every pass of the call (J.rc starts zeroed) */
static void callConstants(RenderJob &J) {
    phip_scene *sc = J.sc; SceneDev &sd = J.sd; const phip_render_params *p = J.p; RenderConst &rc = J.rc;
    rc.tilePixels = (uint32_t) (J.bs * J.bs); rc.tileShift = (uint32_t) J.tileShift; rc.nLocalTiles = sd.nLocalTiles;
    rc.maxDepth = p->max_depth; rc.rrDepth = p->rr_depth; rc.strictNormals = p->strict_normals; rc.hideEmitters = p->hide_emitters;
    rc.seed = p->seed; rc.tileOrigin = sd.tileOrigin.p;
    rc.sampler = (uint32_t) p->sampler; rc.ldMask = J.sampleTotal() - 1u;
    rc.stRes = 1;
    if (p->sampler == PHIP_SAMPLER_SOBOL) {
        rc.sobol.matrices = sd.sobolMat.p; rc.sobol.vdc = (const uint64_t *) sd.sobolVdc.p; rc.sobol.vdcInv = (const uint64_t *) sd.sobolVdc.p + PHIP_SOBOL_MATRIX_SIZE;
        rc.sobol.dims = p->sobol_dimensions; rc.sobol.logRes = p->sobol_log_resolution; rc.sobol.scramble = (uint32_t) p->sobol_scramble;
        rc.sobol.resolution = (float) (1u << p->sobol_log_resolution);
        rc.sobol.matBt = sd.sobolBt.p;              /* (the device code has the byte tables only: dv_math.h) */
        rc.sobol.vdcBt = (const uint64_t *) sd.sobolVdcBt.p; rc.sobol.vdcInvBt = (const uint64_t *) sd.sobolVdcBt.p + 4u * 256u;
    } else if (p->sampler == PHIP_SAMPLER_STRATIFIED) {
        const unsigned n = J.sampleTotal();
        unsigned r = 1; while (r * r < n) ++r;
        rc.stRes = r;
    }
    if (J.rinv) {
        RinvTab &T = rc.rinv;
        T.primes = sd.rinvPrimes.p; T.perm = p->qmc_permutations ? sd.rinvPerm.p : nullptr; T.permOffset = sd.rinvOffsets.p; T.dims = p->qmc_dimensions;
        T.invPerm2 = sd.rinvInvPerm2; T.invPerm3 = sd.rinvInvPerm3;
        if (sd.rinvTabDims) {
            T.dimInfo = sd.rinvDimInfo.p; T.chunk = sd.rinvChunk.p; T.fac = sd.rinvFac.p; T.pw = sd.rinvPw.p; T.tabDims = sd.rinvTabDims;
        }
        const uint32_t res[2] = { (uint32_t) J.D.film.width, (uint32_t) J.D.film.height };
        T.sampleCount = J.sampleTotal();
        rinvFilmResolution(T, p->sampler == PHIP_SAMPLER_HALTON, res);
    }
    rc.diffScaleFactor = 1.0f / sqrtf((float) (p->sample_total > 0 ? p->sample_total : p->spp));
    rc.emitterSamples = J.direct ? p->emitter_samples : 0; rc.bsdfSamples = J.direct ? p->bsdf_samples : 0;
    if (J.direct) {   /* direct.cpp:130-138 */
        const size_t sum = (size_t) p->emitter_samples + (size_t) p->bsdf_samples;
        rc.weightBSDF = 1 / (float) (size_t) p->bsdf_samples;
        rc.weightLum = 1 / (float) (size_t) p->emitter_samples;
        rc.fracBSDF = (size_t) p->bsdf_samples / (float) sum;
        rc.fracLum = (size_t) p->emitter_samples / (float) sum;
    } else {
        rc.weightBSDF = rc.weightLum = 1.0f; rc.fracBSDF = rc.fracLum = 0.5f;
    }
    rc.envFiltered = (sc->envLevelCount > 1 && !(p->flags & PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND)) ? 1u : 0u;
    rc.volpath = p->integrator == PHIP_INTEGRATOR_VOLPATH_SIMPLE ? 1u : 0u;
    rc.dynCounter = sd.dynCounter.p;        /* (blockShard: with the pool, setupWavefront) */
    rc.jitter = J.keepJitter ? sd.jitter.p : nullptr;
}

/* ... and the ones of the pass that starts at sample sppDone of the call */
static void passConstants(RenderJob &J, uint32_t sppDone) {
    RenderConst &rc = J.rc;
    rc.sppPass = std::min(J.sppPerPass, (uint32_t) J.p->spp - sppDone); rc.sppFirst = (uint32_t) J.p->sample_offset + sppDone;
    rc.sppMagic = (uint32_t) std::min<unsigned long long>((1ull << 32) / rc.sppPass, 0xFFFFFFFFull);
    rc.totalIds = J.idsPerSpp * rc.sppPass;
    rc.staticIds = 0; rc.shardIds = 0; rc.countAlive = 0; rc.draining = 0;
}

/* Rows [first, first + n) of the statistics: the waves' counts summed on the device (k_reduce_stats) and their copy into J.hc queued on the job's stream.  The caller
   synchronises -- once, however many reads its test needs */
static void readStatRows(RenderJob &J, int first, int n) {
    Counters *dc = J.sd.counters.p;
    HIP_TRY(hipMemsetAsync(&dc->total[first], 0, n * sizeof(unsigned long long), J.stream));
    hipLaunchKernelGGL(k_reduce_stats, dim3((unsigned) n, REDUCE_SPLIT), dim3(256), 0, J.stream, J.P, dc, first);
    HIP_TRY(hipMemcpyAsync(&J.hc.total[first], &dc->total[first], n * sizeof(unsigned long long), hipMemcpyDeviceToHost, J.stream));
}

enum class FusedPass { Done, GaveUp, Cancelled };

/* One launch: every path of the pass from camera sample to its last vertex (k_mega.h) */
static FusedPass fusedPass(RenderJob &J, uint32_t sppDone) {
    phip_scene *sc = J.sc; SceneDev &sd = J.sd; FusedPlan &F = J.F; hipStream_t stream = J.stream;
    const RenderConst &rc = J.rc; Counters &hc = J.hc;
    const unsigned long long samplesTotal = sd.localPixels;                  /* crop pixels of this device's blocks */
    HIP_TRY(hipMemsetAsync(sd.counters.p, 0, sizeof(Counters), stream));
    HIP_TRY(hipMemsetAsync(sd.megaNext.p, 0, sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(sd.stat.p, 0, (size_t) ST_COUNT * F.M.nWaves * sizeof(unsigned long long), stream));
#if MEGA_MB_FAULT
    F.M.faultWaves = (F.faultPass < 0 || (uint32_t) F.faultPass == sppDone / J.sppPerPass) ? F.faultWaves : 0u;
#else
    (void) sppDone;
#endif
    if (rc.totalIds) {
        if (J.timing) J.evFused.record(stream);
        hipLaunchKernelGGL(F.kernel, F.grid, dim3(BLOCK), F.lds, stream, J.D, F.M, rc, sd.L.p);
        if (J.timing) J.evFused.record(stream);
    }
    HIP_TRY(hipGetLastError());
    /* k_mega bounds every wait of its mailbox protocol and the depth of its task stacks; a wave that gave up says so in the ST_GAVE_UP row (k_mega.h).  Such a pass
       is incomplete: it is not added to the film -- this pass and the rest of the job run on the kernels that have no such protocol (round 6: degrade, do not fail).
       A pass that was not cancelled must also have counted exactly one sample per crop pixel of this device's blocks and sample of the pass (the ids of edge
       blocks outside the crop window are drawn and skipped: rc.totalIds counts them, the samples do not) */
    static_assert(ST_GAVE_UP == ST_SAMPLES + 2, "the rows the host reads after a fused pass: samples .. gave up");
    readStatRows(J, ST_SAMPLES, ST_GAVE_UP - ST_SAMPLES + 1);
    HIP_TRY(hipStreamSynchronize(stream));
    const bool cancelled = cancelRequested(sc);
    const bool gaveUp = hc.total[ST_GAVE_UP] != 0;
#if MEGA_PROFILE || MEGA_MB_DIAG
    const bool countKnown = false;              /* (measurement builds of k_mega: the sample row holds what they measure) */
#else
    const bool countKnown = true;
#endif
    if (!cancelled && (gaveUp || (countKnown && hc.total[ST_SAMPLES] != samplesTotal * rc.sppPass))) {
        fprintf(stderr, "[phip] warning: the fused kernel gave up on this pass (%s); samples %u.. of the job are rendered by the wavefront kernels\n",
                !gaveUp ? "it counted a wrong number of samples" : F.wide ? "a task stack outgrew LDS + spill buffer" : "a mailbox wait timed out",
                (unsigned) rc.sppFirst);
        return FusedPass::GaveUp;               /* (its launch is not one of the job's iterations) */
    }
    if (rc.totalIds) J.st.iterations += 1;
    return cancelled ? FusedPass::Cancelled : FusedPass::Done;
}

/* The ray kernel of one wavefront iteration: the closest-hit and the any-hit rays in one persistent launch */
static void launchRayKernels(RenderJob &J) {
    SceneDev &sd = J.sd; const WavefrontPlan &wf = J.wf; hipStream_t stream = J.stream;
    if (J.timing) J.evTrace.record(stream);
    HIP_TRY(hipMemsetAsync(sd.drawCounters.p, 0, 2 * RAY_SHARDS * RAY_SHARD_STRIDE * sizeof(unsigned int), stream));
    hipLaunchKernelGGL(k_rays_w, wf.pgridRays, dim3(WIDE_BLOCK), wf.wideLds, stream, J.D, J.P, sd.L.p, sd.drawCounters.p);
    if (J.timing) J.evTrace.record(stream);
}

/* One pass on the wavefront kernels: the pool's slots draw sample ids until none is left, one vertex of every live path per iteration.
   false: a wave of k_shade_trace_w gave the pass up (a task stack outgrew LDS + spill buffer, k_wide_wave.h) -- L is incomplete, the caller renders the pass again */
static bool wavefrontPass(RenderJob &J) {
    using clk = std::chrono::steady_clock;
    phip_scene *sc = J.sc; SceneDev &sd = J.sd; const WavefrontPlan &wf = J.wf; hipStream_t stream = J.stream;
    RenderConst &rc = J.rc; Counters &hc = J.hc;
    const uint32_t capacity = wf.capacity;
    HIP_TRY(hipMemsetAsync(sd.counters.p, 0, sizeof(Counters), stream));
    /* static share: the first 3/4 of every slot's samples; the remainder is handed out dynamically */
    {
        const unsigned long long perSlot = rc.totalIds / capacity;
        const unsigned long long staticPerSlot = perSlot - perSlot / 4;
        rc.staticIds = staticPerSlot * capacity;
        const unsigned long long dyn = rc.totalIds - rc.staticIds;
        rc.shardIds = (dyn + DYN_SHARDS - 1) / DYN_SHARDS;
        HIP_TRY(hipMemsetAsync(sd.blockShard.p, 0, wf.nBlocks * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(sd.dynCounter.p, 0, DYN_SHARDS * DYN_STRIDE * sizeof(unsigned long long), stream));
    }
    HIP_TRY(hipMemsetAsync(sd.stat.p, 0, (size_t) ST_COUNT * wf.nWaves * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(sd.shadowCount.p, 0, (size_t) wf.nBlocks * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(sd.blockDead.p, 0, (size_t) wf.nBlocks * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) sd.state.p, (int) F_FRESH, (size_t) capacity, stream));
    /* (no clear of L: the first vertex of every sample -- or its camera ray leaving the scene -- writes L[id]) */

    HIP_TRY(hipStreamSynchronize(stream));
    const auto tLoop0 = clk::now();
    uint32_t iter = 0;
    bool done = rc.totalIds == 0;
    bool drainingSeen = false;                          /* a termination test has counted fewer live slots than the pool holds: blocks may have retired */
    static_assert(ST_GAVE_UP == ST_ALIVE + 1, "the termination test of k_shade_trace_w's passes sums the live-slot row and the gave-up row in one launch");
    const int pollRows = wf.wideTrace ? 2 : 1;          /* k_shade_trace_w: ... and the row in which a wave says that it gave up */
    hc.total[ST_GAVE_UP] = 0;
    while (!done) {
        const bool check = ((iter + 1) & 7) == 0 || rc.totalIds <= (unsigned long long) capacity * 4;
        rc.countAlive = check ? 1 : 0;
        rc.draining = drainingSeen ? 1u : 0u;
        if (J.timing) J.evShade.record(stream);
        if (wf.vertexRays) hipLaunchKernelGGL(wf.vertexRays, wf.vertexGrid, dim3(BLOCK), wf.vertexLds, stream, J.D, J.P, rc, sd.L.p, wf.rays);
        else if (wf.vertexWide) hipLaunchKernelGGL(wf.vertexWide, wf.vertexGrid, dim3(BLOCK), wf.vertexLds, stream, J.D, J.P, rc, sd.L.p, wf.traceNodeCache);
        else hipLaunchKernelGGL(wf.vertex, wf.vertexGrid, dim3(BLOCK), wf.vertexLds, stream, J.D, J.P, rc, sd.L.p);
        if (J.timing) J.evShade.record(stream);
        if (!wf.shadeTrace) launchRayKernels(J);        /* (k_shade_trace traced both rays of the iteration itself: k_shade_trace.h) */
        ++iter;
        if (check) {
            /* termination test: only the live-slot row (and, for a progress callback, the finished-sample row) is summed inside the loop */
            readStatRows(J, ST_ALIVE, pollRows);
            if (J.p->progress) readStatRows(J, ST_SAMPLES, 1);
            HIP_TRY(hipStreamSynchronize(stream));
            if (hc.total[ST_ALIVE] == 0 || hc.total[ST_GAVE_UP] != 0) done = true;
            if (hc.total[ST_ALIVE] < capacity) drainingSeen = true;
            J.progress(J.samplesDone + hc.total[ST_SAMPLES]);
            if (cancelRequested(sc)) { J.cancelled = true; done = true; }
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    if (wf.wideTrace && iter && !J.cancelled && hc.total[ST_GAVE_UP] == 0) {      /* (the last termination test may lie before the launch in which a wave gave up) */
        readStatRows(J, ST_GAVE_UP, 1);
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (hc.total[ST_GAVE_UP] != 0 && !J.cancelled) return false;      /* (its launches are not iterations of the job) */
    if (getenv("PHIP_DEBUG_TIMING")) fprintf(stderr, "[phip] setup %.2f ms, loop %.2f ms (%u iterations)\n", std::chrono::duration<double, std::milli>(tLoop0 - J.t0).count(), std::chrono::duration<double, std::milli>(clk::now() - tLoop0).count(), iter);
    J.st.iterations += iter;
    return true;
}

/* round 4: one pass over L with the footprint sums in registers, then an ordered merge of the 16 x 16 patch images (k_film.h) */
template <int R> static void launchFilmSplat(RenderJob &J, dim3 fg, int acc) {
    SceneDev &sd = J.sd; hipStream_t stream = J.stream;
    const int cells = (16 + 2 * R) * (16 + 2 * R) * 5;
    const unsigned nPatches = (unsigned) sd.nLocalTiles << (2 * (J.tileShift - 4));
    if (sd.patchImg.n < (size_t) nPatches * cells) sd.patchImg.alloc((size_t) nPatches * cells);
    const float4 *Lc = (const float4 *) sd.L.p;
    if (J.qmc) hipLaunchKernelGGL((k_film_splat<R, true>), dim3(nPatches), dim3(256), 0, stream, J.D, J.rc, Lc, sd.patchImg.p, sd.invalid.p);
    else hipLaunchKernelGGL((k_film_splat<R, false>), dim3(nPatches), dim3(256), 0, stream, J.D, J.rc, Lc, sd.patchImg.p, sd.invalid.p);
    hipLaunchKernelGGL(k_film_merge<R>, fg, dim3(BLOCK), 0, stream, J.D, J.rc, (const float *) sd.patchImg.p, (const int32_t *) sd.tileSlot.p, J.tilesX, J.dOut, acc);
}

/* The pass's samples (sd.L) filtered into dOut: onto what is there (acc) or over it */
static void filmPass(RenderJob &J, int acc) {
    SceneDev &sd = J.sd; hipStream_t stream = J.stream;
    const DevScene &D = J.D; const RenderConst &rc = J.rc; float *dOut = J.dOut;
    const int W = J.W, H = J.H, bs = J.bs, tileShift = J.tileShift, tilesX = J.tilesX;
    const dim3 block(BLOCK);
    if (J.timing) J.evFilm.record(stream);
    const dim3 fg((W + 15) / 16, (H + 15) / 16);
    const int reach = (int) std::floor(D.film.radius + 0.5f);
    const bool splat = reach <= 2 && tileShift >= 4 && bs == (1 << tileShift) && sd.nLocalTiles > 0;
    if (splat) {
        if (reach <= 1) launchFilmSplat<1>(J, fg, acc);
        else launchFilmSplat<2>(J, fg, acc);
    } else if (J.qmc)
        hipLaunchKernelGGL(k_film<true>, fg, block, 0, stream, D, rc, (const float4 *) sd.L.p, (const int32_t *) sd.tileSlot.p, tilesX, dOut,
                           acc, sd.invalid.p);
    else if (reach <= FILM_MAX_REACH)
        if (reach <= 2)
            hipLaunchKernelGGL(k_film_tiled<2>, fg, block, 0, stream, D, rc, (const float4 *) sd.L.p, (const int32_t *) sd.tileSlot.p, tilesX, dOut,
                               acc, sd.invalid.p, reach);
        else
            hipLaunchKernelGGL(k_film_tiled<FILM_MAX_REACH>, fg, block, 0, stream, D, rc, (const float4 *) sd.L.p, (const int32_t *) sd.tileSlot.p, tilesX, dOut,
                               acc, sd.invalid.p, reach);
    else
        hipLaunchKernelGGL(k_film<false>, fg, block, 0, stream, D, rc, (const float4 *) sd.L.p, (const int32_t *) sd.tileSlot.p, tilesX, dOut,
                           acc, sd.invalid.p);
    if (J.timing) J.evFilm.record(stream);
}

/* After the film pass: the sample buffer's share of the pass, the pass's counters into the job's, progress */
static void passResults(RenderJob &J) {
    SceneDev &sd = J.sd; hipStream_t stream = J.stream; const RenderConst &rc = J.rc; Counters &hc = J.hc;
    if (J.keepSamples && rc.totalIds) {
        const size_t n = (size_t) J.W * J.H * rc.sppPass;
        hipLaunchKernelGGL(k_export_samples, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, J.D, rc, (const float4 *) sd.L.p,
                           (const int32_t *) sd.tileSlot.p, J.tilesX, sd.sampleOut.p, (uint32_t) J.p->spp, (uint32_t) J.p->sample_offset);
    }
    readStatRows(J, 0, ST_COUNT);
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    phip_stats pass; memset(&pass, 0, sizeof(pass));
    pass.samples = hc.total[ST_SAMPLES]; pass.closest_rays = hc.total[ST_CLOSEST_RAYS]; pass.shadow_rays = hc.total[ST_SHADOW_RAYS];
    pass.path_vertices = hc.total[ST_VERTICES]; pass.closest_node_visits = hc.total[ST_NODE]; pass.closest_triangle_tests = hc.total[ST_TRI];
    pass.shadow_node_visits = hc.total[ST_SH_NODE]; pass.shadow_triangle_tests = hc.total[ST_SH_TRI];
    addWork(J.st, pass);
    J.samplesDone += pass.samples;
    J.progress(J.samplesDone);
}

/* One device's share of a render call: the blocks whose index in the reference's spiral order is congruent to shardIndex
   modulo shardCount, into dOut (device memory of sd.device).  The caller holds the scene's render lock and has validated p. */
static int renderOnDevice(phip_scene *sc, SceneDev &sd, const phip_render_params *p, int shardIndex, int shardCount, float *dOut, phip_stats *stats) {
    HIP_TRY(hipSetDevice(sd.device));
    RenderJob J(sc, sd, p, dOut);
    J.nCU = cuCount(sd.device, J.nCU);
    shardTiles(J, shardIndex, shardCount);
    J.stream = sceneStream(sd, p->n_devices <= 1 ? p->stream : nullptr);    /* a caller's stream belongs to one device */
    planPasses(J, (unsigned long long) sd.nLocalTiles * ((unsigned long long) J.bs * J.bs));
    if (J.keepSamples) { sd.sampleOut.alloc((size_t) J.W * J.H * (size_t) p->spp); HIP_TRY(hipMemsetAsync(sd.sampleOut.p, 0, sd.sampleOut.n * sizeof(float4), J.stream)); }
    sd.haveSamples = J.keepSamples; sd.lastSpp = (uint32_t) p->spp;
    if (p->sampler == PHIP_SAMPLER_SOBOL) uploadSobolTables(J);
    if (J.rinv) uploadRinvTables(J);
    planFused(J);
    HIP_TRY(hipMemsetAsync(sd.invalid.p, 0, sizeof(unsigned long long), J.stream));
    if (!J.F.on) setupWavefront(J, J.idsPerSpp * J.sppPerPass);
    callConstants(J);

    const bool accumulate = (p->flags & PHIP_FLAG_ACCUMULATE) != 0;
    for (uint32_t sppDone = 0; sppDone < (uint32_t) p->spp && !J.cancelled; sppDone += J.sppPerPass) {
        passConstants(J, sppDone);
        if (J.F.on) {
            const FusedPass r = fusedPass(J, sppDone);
            if (r == FusedPass::Cancelled) J.cancelled = true;
            if (r == FusedPass::GaveUp) {
                /* this pass again, and the rest of the job, on k_shade + the ray kernel, which have no such protocol: the same passes, a pool sized for this one */
                J.F.on = false; sd.fused = false;
                setupWavefront(J, J.rc.totalIds);
            }
        }
        if (!J.F.on && !wavefrontPass(J)) {
            /* k_shade_trace_w gave the pass up: this pass again, and the rest of the job, on k_shade + the ray kernel -- the same pool, the same passes (k_mega's contract) */
            fprintf(stderr, "[phip] warning: the fused kernel gave up on this pass (a task stack outgrew LDS + spill buffer); samples %u.. of the job are rendered by the wavefront kernels\n",
                    (unsigned) J.rc.sppFirst);
            selectVertexKernel(J, false, false);
            wavefrontPass(J);
        }
        if (J.cancelled) break;                                 /* L is incomplete: no film pass */
        filmPass(J, (sppDone > 0 || accumulate) ? 1 : 0);
        passResults(J);
    }

    phip_stats &st = J.st;
    if ((sd.nLocalTiles == 0 || J.cancelled) && !accumulate) { HIP_TRY(hipMemsetAsync(dOut, 0, (size_t) J.W * J.H * 5 * sizeof(float), J.stream)); HIP_TRY(hipStreamSynchronize(J.stream)); }
    unsigned long long inv = 0;
    HIP_TRY(hipMemcpy(&inv, sd.invalid.p, sizeof(inv), hipMemcpyDeviceToHost));
    st.invalid_samples = inv;
    st.trace_kernel_ms = J.evTrace.sumPairs(); st.shadow_kernel_ms = 0.0;      /* (k_rays_w casts the shadow rays too: trace_kernel_ms) */
    st.shade_kernel_ms = J.evShade.sumPairs(); st.film_kernel_ms = J.evFilm.sumPairs(); st.fused_kernel_ms = J.evFused.sumPairs();
    st.fused = J.F.on ? 1u : 0u; st.n_devices = 1;
    st.vertex_traced = J.wf.shadeTrace ? 1u : 0u;
    st.render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - J.t0).count();
    algorithmicBytes(J.wf.capacity != 0 /* the wavefront kernels ran */, st, (double) J.W * J.H);
    if (stats) *stats = st;
    return J.cancelled ? PHIP_ERR_CANCELLED : PHIP_OK;
}

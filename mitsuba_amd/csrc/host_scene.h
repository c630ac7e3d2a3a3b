/*
 * host_scene.h -- host side of libphip.so, first of three: the scene.  Device buffers (DevBuf), the camera set-up and the spiral block order, everything that
 * lives on one GPU (SceneDev) and the scene of the C ABI (phip_scene), scene construction as stages over one SceneBuild (validation, host arrays, BVH build
 * via bvh.h, the choice of the device paths, one upload), the host-only table builders of the QMC samplers with the content key of a caller's table, and the
 * replicas of a scene on further GPUs (replicateScene through SceneDev's one list of buffers, ensureReplicas for a device list).
 * Host code only; included by phip.hip alone, after the kernel headers and after its error state (g_err: convertMaterials leaves a text there).
 */
#pragma once

namespace {

template <typename T> struct DevBuf {
    T *p = nullptr; size_t n = 0;
    size_t cap = 0;
    /* hipMalloc / hipFree cost milliseconds: keep the allocation when it is large enough */
    void alloc(size_t count) { if (count > cap) { release(); if (count) { HIP_TRY(hipMalloc((void **) &p, count * sizeof(T))); cap = count; } } n = count; }
    void upload(const T *src, size_t count) { alloc(count); if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice)); }
    void cloneFrom(const DevBuf<T> &src) { alloc(src.n); if (src.n) HIP_TRY(hipMemcpy(p, src.p, src.n * sizeof(T), hipMemcpyDeviceToDevice)); }   /* UVA: also across GPUs (xGMI) */
    void release() { if (p) { (void) hipFree(p); p = nullptr; } n = 0; cap = 0; }
    void swapWith(DevBuf<T> &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); }
    ~DevBuf() { release(); }
};

/* 4x4 helpers for the camera set-up: perspective.cpp:126-157, transform.cpp:33-63,99-123, matrix.inl:138-193 */
struct M4 { float m[4][4]; };
M4 m4identity() { M4 r; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) r.m[i][j] = i == j ? 1.0f : 0.0f; return r; }
M4 m4mul(const M4 &a, const M4 &b) {
    M4 r;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { float s = 0; for (int k = 0; k < 4; ++k) s += a.m[i][k] * b.m[k][j]; r.m[i][j] = s; }
    return r;
}
bool m4invert(const M4 &src, M4 &t) {
    int indxc[4], indxr[4], ipiv[4] = { 0, 0, 0, 0 };
    t = src;
    for (int i = 0; i < 4; i++) {
        int irow = -1, icol = -1; float big = 0;
        for (int j = 0; j < 4; j++) if (ipiv[j] != 1) for (int k = 0; k < 4; k++) {
            if (ipiv[k] == 0) { if (fabsf(t.m[j][k]) >= big) { big = fabsf(t.m[j][k]); irow = j; icol = k; } }
            else if (ipiv[k] > 1) return false;
        }
        ++ipiv[icol];
        if (irow != icol) for (int k = 0; k < 4; ++k) std::swap(t.m[irow][k], t.m[icol][k]);
        indxr[i] = irow; indxc[i] = icol;
        if (t.m[icol][icol] == 0) return false;
        float pivinv = 1.f / t.m[icol][icol];
        t.m[icol][icol] = 1.f;
        for (int j = 0; j < 4; j++) t.m[icol][j] *= pivinv;
        for (int j = 0; j < 4; j++) if (j != icol) {
            float save = t.m[j][icol]; t.m[j][icol] = 0;
            for (int k = 0; k < 4; k++) t.m[j][k] -= t.m[icol][k] * save;
        }
    }
    for (int j = 3; j >= 0; j--) if (indxr[j] != indxc[j]) for (int k = 0; k < 4; k++) std::swap(t.m[k][indxr[j]], t.m[k][indxc[j]]);
    return true;
}

void setupCamera(const phip_camera &c, const phip_film &f, DevCamera &out) {
    const float aspect = f.width / (float) f.height;
    const float relSizeX = (float) f.crop_width / (float) f.width, relSizeY = (float) f.crop_height / (float) f.height;
    const float relOffX = (float) f.crop_offset_x / (float) f.width, relOffY = (float) f.crop_offset_y / (float) f.height;
    /* inverse of scale(1/relSize) * translate(-relOffset) * scale(-0.5,-0.5*aspect,1) * translate(-1,-1/aspect,0) * perspective
       = perspective^-1 * translate^-1 * scale^-1 * translate^-1 * scale^-1 (Transform keeps the product of inverses) */
    M4 persp; memset(&persp, 0, sizeof(persp));
    const float recip = 1.0f / (c.far_clip - c.near_clip);
    const float cot = 1.0f / pm_tanf((c.xfov_deg / 2.0f) * (PT_PI / 180.0f));
    persp.m[0][0] = cot; persp.m[1][1] = cot; persp.m[2][2] = c.far_clip * recip; persp.m[2][3] = -c.near_clip * c.far_clip * recip; persp.m[3][2] = 1;
    M4 perspInv; m4invert(persp, perspInv);
    M4 t2i = m4identity(); t2i.m[0][3] = -(-1.0f); t2i.m[1][3] = -(-1.0f / aspect); t2i.m[2][3] = -0.0f;   /* inverse of translate(-1,-1/aspect,0) */
    M4 s2i = m4identity(); s2i.m[0][0] = 1.0f / -0.5f; s2i.m[1][1] = 1.0f / (-0.5f * aspect); s2i.m[2][2] = 1.0f / 1.0f;
    M4 t1i = m4identity(); t1i.m[0][3] = -(-relOffX); t1i.m[1][3] = -(-relOffY); t1i.m[2][3] = -0.0f;
    M4 s1i = m4identity(); s1i.m[0][0] = 1.0f / (1.0f / relSizeX); s1i.m[1][1] = 1.0f / (1.0f / relSizeY); s1i.m[2][2] = 1.0f / 1.0f;
    /* Transform::operator* : inv = t.inv * this.inv, applied left to right over the five factors */
    M4 inv = s1i;                 /* (scale1)^-1 */
    inv = m4mul(t1i, inv);        /* (scale1*translate1)^-1 = translate1^-1 * scale1^-1 */
    inv = m4mul(s2i, inv);
    inv = m4mul(t2i, inv);
    inv = m4mul(perspInv, inv);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) out.s2c[4 * i + j] = inv.m[i][j];
    for (int i = 0; i < 12; ++i) out.c2w[i] = c.to_world[i];
    out.nearClip = c.near_clip; out.farClip = c.far_clip;
    out.invResX = 1.0f / (float) f.crop_width; out.invResY = 1.0f / (float) f.crop_height;
    /* position differentials on the near plane, perspective.cpp:159-163 (Transform::operator()(Point), transform.h:108-125) */
    auto s2cPoint = [&](float px, float py, float pz) {
        const float x = inv.m[0][0] * px + inv.m[0][1] * py + inv.m[0][2] * pz + inv.m[0][3];
        const float y = inv.m[1][0] * px + inv.m[1][1] * py + inv.m[1][2] * pz + inv.m[1][3];
        const float z = inv.m[2][0] * px + inv.m[2][1] * py + inv.m[2][2] * pz + inv.m[2][3];
        const float w = inv.m[3][0] * px + inv.m[3][1] * py + inv.m[3][2] * pz + inv.m[3][3];
        return (w == 1.0f) ? V3(x, y, z) : V3(x, y, z) / w;
    };
    const V3 p0 = s2cPoint(0.0f, 0.0f, 0.0f);
    const V3 dx = s2cPoint(out.invResX, 0.0f, 0.0f) - p0, dy = s2cPoint(0.0f, out.invResY, 0.0f) - p0;
    out.dx[0] = dx.x; out.dx[1] = dx.y; out.dx[2] = dx.z; out.dy[0] = dy.x; out.dy[1] = dy.y; out.dy[2] = dy.z;
}

/* spiral block order, src/librender/imageproc.cpp:28-78 */
void spiralBlocks(int sizeX, int sizeY, int bs, std::vector<std::pair<int, int>> &out) {
    const int nbx = (int) std::ceil((float) sizeX / (float) bs), nby = (int) std::ceil((float) sizeY / (float) bs);
    const int total = nbx * nby; int generated = 0;
    int cx = nbx / 2, cy = nby / 2, dir = 0, stepsLeft = 1, numSteps = 1;
    out.clear();
    while (generated < total) {
        out.push_back({ cx, cy });
        if (++generated == total) break;
        do {
            switch (dir) { case 0: ++cx; break; case 1: ++cy; break; case 2: --cx; break; case 3: --cy; break; }
            if (--stepsLeft == 0) { dir = (dir + 1) % 4; if (dir == 2 || dir == 0) ++numSteps; stepsLeft = numSteps; }
        } while (cx < 0 || cy < 0 || cx >= nbx || cy >= nby);
    }
}

} // namespace
/* Everything that lives on ONE GPU: the scene arrays (written by the creation and by phip_scene_update, never by a render) and the render-time buffers of the jobs that run there.
   devs[0] of a phip_scene is the device of phip_scene_create; further entries are replicas made by device-to-device copies.
   A new scene buffer is declared below, added to forEachSceneBuffer (the one list replicateScene clones through) and given its line in bind()
   (the only code that writes a buffer pointer into the DevScene); SceneBuild::uploadScene fills it. */
struct SceneDev {
    int device = 0;
    /* ---- scene (immutable after build / replication) ---- */
    DevBuf<float4> tris, wtris, triShade, flatLeaves;      /* tris: the binary tree's leaf order (LDS-resident scenes only), wtris: the wide tree's */
    bool trisAreWide = false;                                      /* scenes past the packed leaf table: DevScene::tris = wtris */
    DevBuf<uint4> wnodes;                                                                     /* compressed wide BVH (big scenes) */
    DevBuf<DevMaterial> materials;
    DevBuf<float> emitterTab;
    DevBuf<float4> texTexels; DevBuf<DevMipLevels> texDesc;                                   /* bitmap textures */
    DevBuf<float4> envTexels; DevBuf<DevMipLevels> envLevels; DevBuf<float> envCdfRows, envCdfCols, envRowWeights;     /* `envmap` emitter */
    DevScene dev;
    /* ---- render-time buffers (grown on demand, reused between calls) ---- */
    DevBuf<float4> rayO, rayD, hit, thr, camHit, shadow, L, sampleOut;
    DevBuf<float2> jitter;                                                                     /* sequence samplers: the camera sample's pixel jitter per sample id (RenderConst::jitter) */
    DevBuf<uint4> info; DevBuf<uint32_t> state; DevBuf<float2> mis;
    DevBuf<Counters> counters;
    DevBuf<uint32_t> tileOrigin, shadowCount, blockDead, spill, blockShard; DevBuf<int32_t> tileSlot;
    DevBuf<uint32_t> sobolMat, sobolBt; DevBuf<unsigned long long> sobolVdc, sobolVdcBt; uint64_t sobolKey = 0; uint32_t sobolLogRes = 0;    /* PHIP_SAMPLER_SOBOL: the plugin's tables */
    DevBuf<uint32_t> rinvDimInfo, rinvChunk, rinvPw; DevBuf<float> rinvFac; uint32_t rinvTabDims = 0;   /* ... and their multi-digit tables (buildRinvTables) */
    DevBuf<uint32_t> rinvPrimes, rinvOffsets; DevBuf<uint16_t> rinvPerm; uint64_t rinvKey = 0;   /* PHIP_SAMPLER_HALTON / _HAMMERSLEY: primes + permutations */
    uint32_t rinvInvPerm2 = 0x4u, rinvInvPerm3 = 0x24u;                                                                         /* inverse permutations of bases 2 and 3, two bits per digit */
    DevBuf<unsigned long long> dynCounter, stat, invalid, megaNext;
    DevBuf<unsigned int> drawCounters;                                                       /* k_rays_w, k_raycast_p: 2 x RAY_SHARDS sharded work counters */
    /* phip_trace_device (host_raycast.h): the persistent ray server's kernels, LDS plan and resident grid, resolved for a tree whose node cache is `nodeCache` */
    struct RaycastPlan { RaycastKernels k = { nullptr, nullptr }; uint32_t nodeCache = 0; size_t lds = 0; unsigned blocks = 0; } raycast;
    /* phip_radiance_device (host_radiance.h): k_shade_r without / with strictNormals and k_radiance_out, resolved at the scene's first call; the running float64 sums of
       a call that takes several passes, two double2 per ray -- the one buffer of that call that grows with its ray count */
    struct RadiancePlan { ShadeRaysKernel vertex[2] = { nullptr, nullptr }; RadianceOutKernel out = nullptr; } radiance;
    DevBuf<double2> radianceAcc;
    DevBuf<float> pyramidScratch;                                                           /* phip_mip_pyramid_device (host_pyramid.h): the float32 chain and the X-pass temporary; grow-only */
    /* phip_vertex_normals_device (host_normals.h): the incidence lists of the scene's vertices (a CSR over its indices: offsets, entries in ascending order), its own
       copy of the indices, the count of invalid vertices and the two events of kernel_ms; made at the scene's first call, valid for its life (the topology is fixed) */
    struct NormalsState { DevBuf<uint32_t> offsets, entries, indices; DevBuf<unsigned int> invalid; hipEvent_t t0 = nullptr, t1 = nullptr; bool ready = false; } normals;
    DevBuf<float> film, patchImg;                                                           /* patchImg: k_film_splat's 16 x 16 patch images (k_film.h) */
    uint32_t lastSpp = 0, nLocalTiles = 0; unsigned long long localPixels = 0;
    int tileKey[3] = { -1, -1, -1 };
    bool haveSamples = false;
    bool fused = false;              /* last render used k_mega */
    hipStream_t stream = nullptr;
    /* phip_render's device-to-host copy of the film into PAGEABLE memory: two pinned staging chunks (filmToHost) */
    float *stage[2] = { nullptr, nullptr }; hipEvent_t stageDone[2] = { nullptr, nullptr };

    /* THE list of the immutable scene buffers, as pointers to members */
    template <typename F> static void forEachSceneBuffer(F f) {
        f(&SceneDev::wnodes); f(&SceneDev::tris); f(&SceneDev::wtris); f(&SceneDev::triShade); f(&SceneDev::flatLeaves);
        f(&SceneDev::materials); f(&SceneDev::emitterTab); f(&SceneDev::texTexels); f(&SceneDev::texDesc);
        f(&SceneDev::envTexels); f(&SceneDev::envLevels); f(&SceneDev::envCdfRows); f(&SceneDev::envCdfCols); f(&SceneDev::envRowWeights);
    }
    /* the pointer members of the DevScene (everything else in it is plain data, equal on every device) */
    void bind() {
        dev.wnodes = wnodes.p; dev.wtris = wtris.p; dev.tris = trisAreWide ? wtris.p : tris.p; dev.triShade = triShade.p; dev.flatLeaves = flatLeaves.p; dev.materials = materials.p;
        dev.texTexels = texTexels.p; dev.textures = texDesc.p; dev.emitterTab = emitterTab.p;
        dev.env.texels = envTexels.p; dev.env.levels = envLevels.p; dev.env.cdfRows = envCdfRows.p; dev.env.cdfCols = envCdfCols.p;
        dev.env.rowWeights = envRowWeights.p;
    }
    /* the fixed per-device work counters of the render kernels */
    void allocCounters() { counters.alloc(1); invalid.alloc(1); dynCounter.alloc(DYN_SHARDS * DYN_STRIDE); megaNext.alloc(1); }
    ~SceneDev() {
        (void) hipSetDevice(device);
        if (stream) (void) hipStreamDestroy(stream);
        for (int i = 0; i < 2; ++i) { if (stage[i]) (void) hipHostFree(stage[i]); if (stageDone[i]) (void) hipEventDestroy(stageDone[i]); }
        if (normals.t0) (void) hipEventDestroy(normals.t0);
        if (normals.t1) (void) hipEventDestroy(normals.t1);
    }
};

/* What phip_scene_update needs of the creation (host_update.h): the topology it keeps fixed.  The host side is filled by SceneBuild::keepForUpdate; the device side is
   made by the first update, so a scene that is never updated pays a few host copies and no device memory */
struct SceneUpdateState {
    uint32_t nVertices = 0, nTriangles = 0; bool hasNormals = false;
    std::vector<uint32_t> indices;                   /* 3 x nTriangles */
    std::vector<uint32_t> wRecPrim, recPrim;         /* the primitive of every Wald record of wtris / tris (0xFFFFFFFF: a leaf's never-hit placeholder): the side table that lets a collapsed triangle come back */
    std::vector<uint32_t> hadRecord;                 /* one bit per triangle: it got a Wald record (degenerate triangles are dropped by makeLeaf: a refit cannot give them one) */
    std::vector<uint8_t> triClass;                   /* the shade class of every triangle (tagShadeClasses): phip_scene_rebuild writes it into the records of its new tree */
    std::vector<uint32_t> wLevels;                   /* HostBVH::wLevels */
    std::vector<int32_t> leafRefs;                   /* the references of the packed leaf table's leaves, in its order */
    struct EmitterMesh { uint32_t emitter, firstTri, nTris, firstVertex, endVertex; };      /* area emitters: their triangles and the vertex range those use */
    std::vector<EmitterMesh> emitterMeshes;
    std::vector<float> tab; size_t ecdfSize = 0;     /* the packed emitter table as uploaded; its selection cdf's length */
    std::vector<float> hostPositions;                /* device-pointer updates: the emitter meshes' vertex ranges, copied back */
    uint32_t nDegenerate = 0;
    bool onDevice = false;
    /* phip_scene_update_appearance (host_appearance.h): what the creation knew of the scene's look and the call validates a new look against -- the shapes (material,
       emitter, triangle range, normals / texture coordinates), the materials and emitters as last given, every texture's and the environment map's descriptor with
       its level-0 maximum; on the device the triangle -> shape map and the per-shape table of the records pass, made by the first call */
    struct Appearance {
        std::vector<DevShape> shapes; std::vector<phip_material> materials; std::vector<phip_emitter> emitters;
        std::vector<DevMipLevels> texDesc; std::vector<float> texMax; DevMipLevels envLevels; bool envIsMap = false;
        DevBuf<uint32_t> dTriShape, dTexMax; DevBuf<detail::ShapeWords> dShapeWords; DevBuf<float> dScratch, dRowTerms, dRowSum;
    } app;
    DevBuf<uint32_t> dIndices, dWRecPrim, dRecPrim, dHadRecord, dCounters; DevBuf<int32_t> dLeafRefs;
    DevBuf<float> dPositions, dNormals, dNodeBox, dSahTerm, dPartials; DevBuf<detail::RefitConsts> dConsts;
    /* phip_scene_rebuild (host_rebuild.h): from the first rebuild on the host vectors wRecPrim, hadRecord and wLevels above are what they were for -- the source of the
       first upload and the counts -- and no more: wRecPrim keeps its size up to date, not its content.  The scratch of the pipeline, kept between calls: */
    struct RebuildScratch {
        DevBuf<uint32_t> keys, tris, sortedKeys, sortedTris, range, parent, arrived; DevBuf<int32_t> child, items, slotRef; DevBuf<float> box;
        DevBuf<unsigned long long> scanIn, scanOut; DevBuf<unsigned char> temp; DevBuf<uint8_t> triClass;
    } rb;
};

struct phip_scene {
    phip_scene_desc descCopy;        /* scalar fields only */
    HostBVH bvh;                     /* tree statistics (the node / record arrays are released after the upload) */
    bool hasTextures = false; uint32_t triShadeStride = TRISHADE_FLOAT4S;
    int envLevelCount = 0;           /* MIP levels of the envmap (0: no envmap) */
    int materialMask = MM_ALL;       /* leaf BSDF models present: selects the k_shade instantiation */
    bool flatTraceToo = false;       /* a scene of k_mega that k_shade_trace could serve as well (PHIP_FLAG_NO_MEGA) */
    bool flatTrace = false;          /* not a scene of k_mega, but its tree is the packed leaf table (<= 64 Wald records) and emitter table + materials fit LDS: k_shade_trace */
    bool wideOnly = false;           /* the device holds the compressed 8-wide BVH the ray kernels walk (every scene has it) and nothing else (more than 64 Wald records): no leaf table, no LDS-resident kernels */
    bool fitsLds = false;            /* tree, Wald records, shading records, emitter table and materials fit the fused kernel's LDS plan */
    bool wideTrace = false;          /* k_shade_trace_w can run the scene's iterations: it is on the 8-wide tree only, with any feature set k_shade serves (textures, UVs, `constant`, `envmap`) */
    int fusedWide = 0;               /* round 6: 4 / 5 = the fused kernel walks the 8-wide tree from memory (k_mega<.., FLAT 4 / 5, ..>: emitter table in LDS; materials in LDS / in memory) */
    SceneUpdateState upd;
    std::vector<std::unique_ptr<SceneDev>> devs;
    int *cancelFlag = nullptr;       /* host-pinned (portable, mapped): phip_cancel writes it, host loops and k_mega poll it */
    std::mutex renderLock;
    std::mutex progressLock;         /* the progress callback is entered by one device thread at a time (renderMultiDevice runs one host thread per GPU) */
    phip_scene() { devs.emplace_back(new SceneDev()); }
    ~phip_scene() { devs.clear(); if (cancelFlag) (void) hipHostFree(cancelFlag); }
};

static std::vector<DevMaterial> convertMaterials(const phip_material *materials, uint32_t nMaterials, const std::vector<float> *textureMax = nullptr) {
    if (nMaterials && !materials) throw std::runtime_error("materials is NULL");
    std::vector<DevMaterial> mats(nMaterials);
    /* the maximum of bitmap texture `id` (1-based, not 0) */
    auto textureMaxOf = [&](uint32_t id) -> float {
        if (!textureMax || id > textureMax->size()) throw std::runtime_error("material texture id out of range");
        return (*textureMax)[id - 1];
    };
    /* a `bitmap` texture on specularReflectance (dielectric.cpp:159-160, roughconductor.cpp:173-174,236: ensureEnergyConservation) */
    auto specularTexture = [&](const phip_material &m, DevMaterial &o) {
        if (m.reflectance_texture == 0) return;
        if (textureMaxOf(m.reflectance_texture) > 1.0f) throw std::runtime_error("specularReflectance texture > 1 (ensureEnergyConservation)");
        o.reflTexture = m.reflectance_texture;
    };
    for (uint32_t i = 0; i < nMaterials; ++i) {
        const phip_material &m = materials[i];
        DevMaterial &o = mats[i];
        memset(&o, 0, sizeof(o));
        o.type = m.type; o.nested0 = m.nested[0]; o.nested1 = m.nested[1];
        for (int k = 0; k < 3; ++k) { o.refl[k] = m.reflectance[k]; o.trans[k] = m.transmittance[k]; o.eta[k] = m.eta[k]; o.k[k] = m.k[k]; }
        o.distribution = m.distribution; o.sampleVisible = m.sample_visible ? 1 : 0;
        switch (m.type) {
            case PHIP_BSDF_DIFFUSE: {
                float mx = std::max(m.reflectance[0], std::max(m.reflectance[1], m.reflectance[2]));
                if (m.reflectance_texture != 0) {            /* m_reflectance->getMaximum().max() of the bitmap */
                    mx = textureMaxOf(m.reflectance_texture);
                    o.reflTexture = m.reflectance_texture;
                }
                if (mx > 1.0f) throw std::runtime_error("diffuse reflectance > 1 (ensureEnergyConservation, diffuse.cpp:95)");
                if (mx > 0) o.flags |= MF_SMOOTH;            /* component list empty otherwise, diffuse.cpp:97-100 */
            } break;
            case PHIP_BSDF_DIELECTRIC:
                if (!(m.eta[0] > 0)) throw std::runtime_error("dielectric eta must be positive");
                o.flags |= MF_TRANS_OR_BACK;
                specularTexture(m, o);
                if (m.transmittance_texture != 0) {          /* dielectric.cpp:161-162,207-208: ensureEnergyConservation(specularTransmittance) */
                    if (textureMaxOf(m.transmittance_texture) > 1.0f) throw std::runtime_error("specularTransmittance texture > 1 (ensureEnergyConservation)");
                    o.transTexture = m.transmittance_texture;
                }
                break;
            case PHIP_BSDF_ROUGHCONDUCTOR: {
                specularTexture(m, o);
                if (m.distribution > PHIP_MF_GGX) { g_err = "unsupported microfacet distribution"; throw std::invalid_argument("unsupported microfacet distribution (only beckmann, ggx)"); }
                o.flags |= MF_SMOOTH;
                /* alpha = ConstantFloatTexture.eval().average() (roughconductor.cpp:275-280), clamp microfacet.h:113-114 */
                o.alphaU = std::max(V3(m.alpha_u).average(), 1e-4f);
                o.alphaV = std::max(V3(m.alpha_v).average(), 1e-4f);
                /* a `bitmap` texture as the child "alpha" / "alphaU" / "alphaV" (roughconductor.cpp:424-431): evaluated per vertex */
                for (uint32_t t : { m.alpha_u_texture, m.alpha_v_texture })
                    if (t != 0) (void) textureMaxOf(t);
                o.alphaUTexture = m.alpha_u_texture; o.alphaVTexture = m.alpha_v_texture;
            } break;
            case PHIP_BSDF_TWOSIDED: {
                if (m.nested[0] >= i || m.nested[1] >= i) throw std::runtime_error("twosided: nested materials must precede the adapter");
                const DevMaterial &a = mats[m.nested[0]], &b = mats[m.nested[1]];
                if ((a.type != PHIP_BSDF_DIFFUSE && a.type != PHIP_BSDF_ROUGHCONDUCTOR) || (b.type != PHIP_BSDF_DIFFUSE && b.type != PHIP_BSDF_ROUGHCONDUCTOR))
                    throw std::runtime_error("twosided: only materials without a transmission component can be nested (twosided.cpp:104-106)");
                if ((a.flags | b.flags) & MF_SMOOTH) o.flags |= MF_SMOOTH;
                o.flags |= MF_TRANS_OR_BACK;                  /* EBackSide, twosided.cpp:96-100 */
            } break;
            default: throw std::runtime_error("unknown bsdf type");
        }
    }
    return mats;
}

/* level sizes of a complete MIP pyramid down to 1x1 (mipmap.h:182-192); n_levels is 1 or that pyramid's own count.  `what` = "texture" / "envmap" */
static void pyramidLevels(DevMipLevels &lv, int sx, int sy, uint32_t nLevels, int maxLevels, const std::string &what) {
    int n = 1;
    lv.lw[0] = sx; lv.lh[0] = sy;
    if (nLevels > 1) {
        while (sx > 1 || sy > 1) {
            sx = std::max(1, (sx + 1) / 2); sy = std::max(1, (sy + 1) / 2);
            if (n >= maxLevels) throw std::runtime_error(what + ": too many MIP levels");
            lv.lw[n] = sx; lv.lh[n] = sy; ++n;
        }
        if ((uint32_t) n != nLevels) throw std::runtime_error(what + ": n_levels must be 1 or the complete pyramid down to 1x1");
    }
    lv.nLevels = n;
}
/* EWA weight table, mipmap.h:296-301 */
static void ewaWeightLut(float *lut) { for (int k = 0; k < 64; ++k) { const float r2 = (float) k / 63.0f; lut[k] = pm_expf(-2.0f * r2) - pm_expf(-2.0f); } }

/* m_alphaU != m_alphaV as OBJECTS (one texture for both is isotropic, roughconductor.cpp:228-229); twosided.cpp:96-100 inherits the flag */
static bool anisotropic(const phip_material *materials, uint32_t nMaterials, uint32_t m, int depth = 0) {
    if (m >= nMaterials || depth > 2) return false;
    const phip_material &M = materials[m];
    if (M.type == PHIP_BSDF_ROUGHCONDUCTOR)
        return (M.alpha_u_texture | M.alpha_v_texture) ? M.alpha_u_texture != M.alpha_v_texture : std::max(M.alpha_u, 1e-4f) != std::max(M.alpha_v, 1e-4f);
    if (M.type == PHIP_BSDF_TWOSIDED) return anisotropic(materials, nMaterials, M.nested[0], depth + 1) || anisotropic(materials, nMaterials, M.nested[1], depth + 1);
    return false;
}
/* TriMesh::computeUVTangents, trimesh.cpp:683-693: an anisotropic BSDF (roughconductor.cpp:196-200,230-231: the clamped
   alphaU != alphaV) needs texture coordinates for its tangent frame -- an error there.  (DevShape::pad: the mesh has them) */
static void requireTexcoordsOfAnisotropic(const phip_material *materials, uint32_t nMaterials, const std::vector<DevShape> &shapes) {
    for (const DevShape &s : shapes)
        if (!s.pad && anisotropic(materials, nMaterials, s.material))
            throw std::runtime_error("computeUVTangents(): texture coordinates are required to generate tangent vectors (anisotropic BSDF on a shape without them)");
}
/* the leaf BSDF models present (MM_*): selects the instantiation of the shading kernels */
static int materialMaskOf(const std::vector<DevMaterial> &mats) {
    int mask = 0;
    for (const DevMaterial &m : mats) {
        if (m.type == PHIP_BSDF_ROUGHCONDUCTOR) mask |= MM_ROUGH;
        if (m.type == PHIP_BSDF_DIELECTRIC) mask |= MM_DIELECTRIC;
    }
    return mask;
}
/* what the shading records of a shape's triangles say of its material: the leaf seen from either side (a `twosided` adapter's nested ids, or the material itself
   twice), the material's flag bits (TS_MATERIAL_BITS), and the shade class of its Wald records -- 0 diffuse, 1 rough conductor, 2 dielectric, the heavier of the
   two sides of a two-sided surface */
static uint32_t shadeClassOf(const std::vector<DevMaterial> &mats, uint32_t front, uint32_t back) {
    auto classOf = [&](uint32_t leaf) { const int t = mats[leaf].type; return t == PHIP_BSDF_ROUGHCONDUCTOR ? 1u : (t == PHIP_BSDF_DIELECTRIC ? 2u : 0u); };
    const uint32_t a = classOf(front), b = classOf(back);
    return (a == 1u || b == 1u) ? 1u : std::max(a, b);
}
static detail::ShapeWords shapeWordsOf(const std::vector<DevMaterial> &mats, uint32_t material) {
    const DevMaterial &m = mats[material];
    const bool twosided = m.type == PHIP_BSDF_TWOSIDED;
    detail::ShapeWords w;
    w.front = twosided ? m.nested0 : material; w.back = twosided ? m.nested1 : material;
    w.flags = (twosided ? TS_TWOSIDED : 0u) | ((m.flags & MF_SMOOTH) ? TS_MF_SMOOTH : 0u) | ((m.flags & MF_TRANS_OR_BACK) ? TS_TRANS_OR_BACK : 0u);
    w.cls = shadeClassOf(mats, w.front, w.back);
    return w;
}
/* the emitter selection CDF (scene.cpp:375-381 + DiscreteDistribution::normalize): n + 1 entries; returns the normalization (0 for a sum that is not positive) */
static float emitterCdfOf(const phip_emitter *emitters, uint32_t nEmitters, std::vector<float> &ecdf) {
    ecdf.assign(1, 0.0f);
    for (uint32_t i = 0; i < nEmitters; ++i) ecdf.push_back(ecdf.back() + emitters[i].sampling_weight);
    float emNorm = 0;
    if (nEmitters) {
        const float sum = ecdf.back();
        if (sum > 0) { emNorm = 1.0f / sum; for (size_t j = 1; j < ecdf.size(); ++j) ecdf[j] *= emNorm; ecdf.back() = 1.0f; }
    }
    return emNorm;
}
/* the sampling fields of a bitmap texture's descriptor (everything but the pyramid's sizes and offsets) */
static void textureSampling(const phip_texture &t, DevMipLevels &lv) {
    if (t.wrap_u > PHIP_WRAP_ONE || t.wrap_v > PHIP_WRAP_ONE || t.filter_type > PHIP_FILTER_EWA) throw std::runtime_error("bad texture wrap mode / filter type");
    lv.bcu = t.wrap_u; lv.bcv = t.wrap_v; lv.filterType = t.filter_type; lv.maxAnisotropy = t.max_anisotropy;
    lv.uvScale[0] = t.uv_scale[0]; lv.uvScale[1] = t.uv_scale[1]; lv.uvOffset[0] = t.uv_offset[0]; lv.uvOffset[1] = t.uv_offset[1];
}
/* the environment map's transforms, scale and normalization from its CDF's total (envmap.cpp:318-328), after the refusals of a map that cannot be sampled */
static void envmapConstants(const phip_envmap &e, float rowSum, DevEnvMap &E) {
    if (rowSum == 0) throw std::runtime_error("The environment map is completely black -- this is not allowed.");
    if (!std::isfinite(rowSum)) throw std::runtime_error("The environment map contains an invalid floating point value (nan/inf) -- giving up.");
    M4 tw, tl;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) tw.m[i][j] = e.to_world[4 * i + j];
    if (!m4invert(tw, tl)) throw std::runtime_error("envmap toWorld is singular");
    const int w = (int) e.width, h = (int) e.height;
    E.w = w; E.h = h; E.scale = e.scale;
    E.normalization = 1.0f / (rowSum * (2 * PT_PI / w) * (PT_PI / h));
    E.pixelSizeX = 2 * PT_PI / w; E.pixelSizeY = PT_PI / h;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { E.toWorld[3 * i + j] = tw.m[i][j]; E.toLocal[3 * i + j] = tl.m[i][j]; }
}

/* TriMesh::prepareSamplingTable, trimesh.cpp:388-404 + DiscreteDistribution::normalize: the area CDF of a mesh's triangles (n + 1 entries); returns 1 / surface area */
static float areaCdfOf(const float *positions, const uint32_t *indices, uint32_t firstTri, uint32_t nTris, std::vector<float> &cdf) {
    cdf.assign(1, 0.0f);
    for (uint32_t j = 0; j < nTris; ++j) {
        const uint32_t *ix = indices + 3 * (size_t) (firstTri + j);
        const float *p0 = positions + 3 * (size_t) ix[0], *p1 = positions + 3 * (size_t) ix[1], *p2 = positions + 3 * (size_t) ix[2];
        V3 a(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]), b(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]);
        cdf.push_back(cdf.back() + 0.5f * cross(a, b).length());
    }
    const float sum = cdf.back();
    if (!(sum > 0)) throw std::runtime_error("area emitter with zero surface area");
    const float norm = 1.0f / sum;
    for (size_t j = 1; j < cdf.size(); ++j) cdf[j] *= norm;
    cdf.back() = 1.0f;
    return 1.0f / sum;
}

/* ConstantBackgroundEmitter::createShape (constant.cpp:67-72) as seen from Scene::initializeBidirectional
   (scene.cpp:384-413): bounding sphere (aabb.cpp:44-47) of the kd-tree's enlarged box expanded by the sensor
   position (track.cpp:79-83), radius x 1.5 */
static void environmentSphereOf(const float *sceneMin, const float *sceneMax, uint32_t nTriangles, const phip_camera &camera, DevScene &D) {
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
        mn[a] = nTriangles ? sceneMin[a] : INFINITY; mx[a] = nTriangles ? sceneMax[a] : -INFINITY;
    }
    const float *m = camera.to_world;
    V3 sp(m[3], m[7], m[11]);
    if (m[15] != 1.0f) sp = sp / m[15];
    const float spv[3] = { sp.x, sp.y, sp.z };
    for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], spv[a]); mx[a] = std::max(mx[a], spv[a]); }
    const V3 center = (V3(mx[0], mx[1], mx[2]) + V3(mn[0], mn[1], mn[2])) * 0.5f;
    const float radius = (center - V3(mx[0], mx[1], mx[2])).length();
    D.envCenter[0] = center.x; D.envCenter[1] = center.y; D.envCenter[2] = center.z;
    D.envRadius = std::max(PT_EPSILON, radius * 1.5f);
}

/* What follows from the counts of the 8-wide tree, stated once for the creation (chooseTraversal, chooseDevicePaths) and for phip_scene_rebuild, whose tree has other counts:
   whether its depth fits the traversal stacks (one group per level) ... */
static bool wideDepthFits(uint32_t wMaxDepth) { return (int) wMaxDepth + 2 <= WIDE_STACK_LDS + SPILL_DEPTH / 2; }
/* ... the top of the tree the ray kernels stage in LDS (its nodes are in breadth-first order), and the kernels that walk it from memory beside the wavefront's: fusedWide
   (round 6: k_mega on a tree that does not fit LDS, k_wide_wave.h -- every scene on the 8-wide tree whose emitter table fits LDS and that needs none of the feature sets k_mega
   is not compiled with: bitmap textures, an environment emitter) and wideTrace (k_shade_trace_w).  Reads the DevScene's constants (sceneConstants) and the tree's statistics */
static void wideTreePaths(phip_scene *sc, DevScene &D) {
    const HostBVH &bvh = sc->bvh;
    D.wideNodeCache = std::min<uint32_t>(bvh.nWNodes, WIDE_NODE_CACHE_MAX);
    const bool addressable = bvh.nWTris < WP_TRI_MAX;
    sc->fusedWide = (sc->wideOnly && !sc->hasTextures && D.envEmitter < 0 && sc->triShadeStride == TRISHADE_FLOAT4S && D.emitterTabSize <= EMITTER_LDS_FLOATS && addressable)
                  ? (D.nMaterials <= MATERIAL_LDS_MAX ? 4 : 5) : 0;
    sc->wideTrace = sc->wideOnly && addressable;
}

/* which device path serves the scene: fitsLds (k_mega on the LDS-resident tree), fusedWide (k_mega on the 8-wide tree), flatTrace (k_shade_trace), wideTrace (k_shade_trace_w);
   the deal region at the front of k_mega's dynamic LDS, the lane deal of the shading kernels.
   Reads the DevScene's counts (sceneConstants, flatLeafTable) and the material mask: phip_scene_update_appearance calls it again when the mask has changed */
static void devicePathsOf(phip_scene *sc, DevScene &D, bool fitsLdsBase) {
    const int mask = sc->materialMask;
    sc->fitsLds = fitsLdsBase;                              /* (implies the packed leaf table: recordsInLds) */
    /* round 6: the fused kernel on a tree that does not fit LDS (k_wide_wave.h) -- every scene on the 8-wide tree whose emitter table fits LDS and that needs none of the
       feature sets k_mega is not compiled with (bitmap textures, an environment emitter) */
    wideTreePaths(sc, D);
    const bool traceable = D.flatMode >= 2 && D.emitterTabSize <= EMITTER_LDS_FLOATS && D.nMaterials <= MATERIAL_LDS_MAX;
    sc->flatTrace = !sc->fitsLds && traceable; sc->flatTraceToo = sc->fitsLds && traceable;
    /* k_mega deals the Wald tests of the packed table over the wave through LDS buffers at the front of its dynamic LDS
       (k_traverse.h: traverseFlat2W); k_mega<MM_ALL> keeps its mailbox of copper vertices in MEGA_DEAL_DWORDS x BLOCK dwords of LDS that lie there too (k_mega.h) */
    const uint32_t dealList = D.flatMode >= 2 ? (uint32_t) (((BLOCK / 64) * BAL_WAVE_BYTES + BLOCK * sizeof(uint32_t) - 1) / (BLOCK * sizeof(uint32_t))) : 0u;
    const uint32_t mailbox = (sc->fitsLds && mask != 0) ? (uint32_t) MEGA_DEAL_DWORDS : 0u;
    D.dealDwords = std::max(dealList, mailbox);
    /* the lane deal of k_shade pays where the expensive model is rare: rough conductors (microfacet sampling: atrium, 8 % of the vertices,
       k_shade -7 %); on a diffuse + dielectric mix the extra round trip costs more than the cheap Fresnel branch (glass room: +8 %).
       k_shade_trace deals its lanes by BSDF model where there is more than one (the kernel traces its own rays and leaves the class in the hit word) */
    D.shadeSort = ((mask & MM_ROUGH) || (traceable && mask != 0)) ? 1u : 0u;
}

/* One phip_scene_create: what the stages of buildScene hand to each other.  Every stage up to chooseDevicePaths works on host arrays and calls no HIP
   function; uploadScene is the only one that allocates or copies scene buffers. */
struct SceneBuild {
    phip_scene *sc; SceneDev &sd; const phip_scene_desc &d; DevScene &D;
    std::vector<DevShape> shapes; std::vector<uint32_t> triShape; std::vector<float> areaCdf;
    std::vector<float4> texTexels; std::vector<DevMipLevels> texDesc; std::vector<float> texMax;
    std::vector<DevMaterial> mats;
    std::vector<DevEmitter> ems; std::vector<float> ecdf; float emNorm = 0; int32_t envEmitter = -1; bool envIsMap = false;
    std::vector<float4> ts; uint32_t stride = TRISHADE_FLOAT4S;     /* shading records */
    std::vector<float> tab;                                         /* packed emitter table */
    std::vector<float4> envTexels; DevMipLevels envLevels; std::vector<float> envCdfRows, envCdfCols, envRowWeights;
    std::vector<float4> flat;                                       /* packed leaf table (flatMode != 0) */
    bool recordsInLds = false, fitsLdsBase = false;                 /* ldsPlan -> flatLeafTable, chooseDevicePaths */
    std::vector<uint8_t> triClass;                                  /* tagShadeClasses -> keepForUpdate */

    SceneBuild(phip_scene *sc, const phip_scene_desc &d) : sc(sc), sd(*sc->devs[0]), d(d), D(sd.dev) { memset(&D, 0, sizeof(D)); }

    /* ABI version, NULL arrays, film / crop / filter, index range */
    void validateDesc() {
        if (d.abi_version != PHIP_ABI_VERSION) throw std::runtime_error("phip_scene_desc.abi_version mismatch");
        if (d.n_vertices && !d.positions) throw std::runtime_error("positions is NULL");
        if (d.n_triangles && !d.indices) throw std::runtime_error("indices is NULL");
        if (d.film.crop_width <= 0 || d.film.crop_height <= 0 || d.film.width <= 0 || d.film.height <= 0)
            throw std::runtime_error("invalid film size");
        if (d.film.crop_offset_x < 0 || d.film.crop_offset_y < 0 || d.film.crop_offset_x + d.film.crop_width > d.film.width ||
            d.film.crop_offset_y + d.film.crop_height > d.film.height)
            throw std::runtime_error("invalid crop window");          /* film.cpp:44-48 */
        if (d.film.crop_width >= 65536 || d.film.crop_height >= 65536)
            throw std::runtime_error("crop window of 65536 pixels or more per side (block origins are packed into 16 bits)");
        if (!(d.film.filter_radius > 0)) throw std::runtime_error("filter radius must be > 0");
        for (uint32_t i = 0; i < 3 * d.n_triangles; ++i)
            if (d.indices[i] >= d.n_vertices) throw std::runtime_error("triangle index out of range");
    }

    /* DevShapes, the triangle -> shape map, the area CDFs of the emitter meshes */
    void flattenShapes() {
        shapes.resize(d.n_shapes); triShape.resize(d.n_triangles);
        uint32_t expect = 0;
        for (uint32_t i = 0; i < d.n_shapes; ++i) {
            const phip_shape &s = d.shapes[i];
            if (s.first_triangle != expect) throw std::runtime_error("shape triangle ranges must tile the index array in order");
            if (s.material >= d.n_materials) throw std::runtime_error("shape material id out of range");
            if (s.emitter >= (int32_t) d.n_emitters) throw std::runtime_error("shape emitter id out of range");
            if (s.emitter >= 0 && d.emitters[s.emitter].type != PHIP_EMITTER_AREA) throw std::runtime_error("a shape can only carry an area emitter");
            if (s.has_normals && !d.normals) throw std::runtime_error("shape has_normals but normals is NULL");
            expect += s.n_triangles;
            DevShape &o = shapes[i];
            if (s.has_texcoords && !d.texcoords) throw std::runtime_error("shape has_texcoords but texcoords is NULL");
            o.material = s.material; o.emitter = s.emitter; o.hasNormals = s.has_normals ? 1 : 0;
            o.firstTri = s.first_triangle; o.nTris = s.n_triangles; o.cdfOffset = 0; o.invSurfaceArea = 0; o.pad = s.has_texcoords ? 1 : 0;    /* pad: the mesh has texture coordinates */
            for (uint32_t j = 0; j < s.n_triangles; ++j) triShape[s.first_triangle + j] = i;
            if (s.emitter >= 0) {
                /* TriMesh::prepareSamplingTable, trimesh.cpp:388-404 + DiscreteDistribution::normalize */
                if (s.n_triangles == 0) throw std::runtime_error("area emitter on an empty mesh");
                o.cdfOffset = (uint32_t) areaCdf.size();
                std::vector<float> cdf;
                o.invSurfaceArea = areaCdfOf(d.positions, d.indices, s.first_triangle, s.n_triangles, cdf);
                areaCdf.insert(areaCdf.end(), cdf.begin(), cdf.end());
            }
        }
        if (expect != d.n_triangles) throw std::runtime_error("shape triangle ranges do not cover the index array");
    }

    /* bitmap textures: every pyramid (as delivered) in one float4 texel array + one descriptor each, the maximum of every level 0 */
    void packTextures() {
        texDesc.resize(d.n_textures); texMax.assign(d.n_textures, 0.0f);
        if (d.n_textures && !d.textures) throw std::runtime_error("textures is NULL");
        for (uint32_t i = 0; i < d.n_textures; ++i) {
            const phip_texture &t = d.textures[i];
            if (t.width == 0 || t.height == 0 || !t.levels[0]) throw std::runtime_error("texture without level 0");
            DevMipLevels &lv = texDesc[i]; memset(&lv, 0, sizeof(lv));
            textureSampling(t, lv);
            pyramidLevels(lv, (int) t.width, (int) t.height, t.n_levels, PHIP_MIP_MAX_LEVELS, "texture");
            for (int l = 0; l < lv.nLevels; ++l) {
                if (!t.levels[l]) throw std::runtime_error("texture: level pointer is NULL");
                lv.offset[l] = (uint32_t) texTexels.size();
                const size_t cnt = (size_t) lv.lw[l] * lv.lh[l];
                for (size_t k = 0; k < cnt; ++k) {
                    const float *c = t.levels[l] + 3 * k;
                    texTexels.push_back(make_float4(c[0], c[1], c[2], 0.0f));
                    if (l == 0) texMax[i] = detail::texelMaxStep(texMax[i], c[0], c[1], c[2]);
                }
            }
            if (texTexels.size() >= (1ull << 32)) throw std::runtime_error("textures too large");
            ewaWeightLut(lv.weightLut);
        }
        sc->hasTextures = d.n_textures > 0;
    }

    /* DevMaterials, the leaf BSDF models present, the texture-coordinate requirement of anisotropic BSDFs */
    void materials() {
        mats = convertMaterials(d.materials, d.n_materials, &texMax);
        requireTexcoordsOfAnisotropic(d.materials, d.n_materials, shapes);
        sc->materialMask = materialMaskOf(mats);
    }

    /* DevEmitters + selection pdf (scene.cpp:375-381), the single environment emitter */
    void emitterSelection() {
        ems.resize(d.n_emitters);
        for (uint32_t i = 0; i < d.n_emitters; ++i) {
            const phip_emitter &e = d.emitters[i];
            if (e.type == PHIP_EMITTER_CONSTANT || e.type == PHIP_EMITTER_ENVMAP) {
                if (envEmitter >= 0) throw std::runtime_error("The scene may only contain one environment emitter");   /* scene.cpp:510-513 */
                envEmitter = (int32_t) i;
                envIsMap = e.type == PHIP_EMITTER_ENVMAP;
            } else if (e.type != PHIP_EMITTER_AREA) throw std::runtime_error("unknown emitter type");
            else if (e.shape >= d.n_shapes || d.shapes[e.shape].emitter != (int32_t) i) throw std::runtime_error("emitter/shape back reference mismatch");
            memset(&ems[i], 0, sizeof(DevEmitter));
            for (int k = 0; k < 3; ++k) ems[i].radiance[k] = e.radiance[k];
            ems[i].samplingWeight = e.sampling_weight; ems[i].shape = e.type == PHIP_EMITTER_AREA ? e.shape : 0xFFFFFFFFu;
        }
        emNorm = emitterCdfOf(d.emitters, d.n_emitters, ecdf);
    }

    /* acceleration structure (bvh.h) and the two limits of its encodings */
    void buildAccel() {
        const float camPos[3] = { d.camera.to_world[3], d.camera.to_world[7], d.camera.to_world[11] };
        buildBVH(d.positions, d.indices, d.n_triangles, sc->bvh, camPos);
        if (sc->bvh.tris.size() / 12 >= (1u << 28)) throw std::runtime_error("too many triangle records for the leaf reference encoding");
        if (d.n_triangles > HIT_PRIM_MASK) throw std::runtime_error("too many triangles for the hit record (30-bit primitive index)");
    }

    /* shading records (dv_scene.h): the per-triangle constants come from the same __host__ __device__
       functions the kernel would run, so precomputing them does not change a single bit */
    void shadingRecords() {
        bool anyTexcoords = false;
        for (uint32_t i = 0; i < d.n_shapes; ++i) anyTexcoords |= d.shapes[i].has_texcoords != 0;
        stride = anyTexcoords ? TRISHADE_FLOAT4S_UV : TRISHADE_FLOAT4S;
        sc->triShadeStride = stride;
        ts.assign((size_t) stride * d.n_triangles, make_float4(0, 0, 0, 0));
        for (uint32_t i = 0; i < d.n_triangles; ++i) {
            const DevShape &sh = shapes[triShape[i]];
            const uint32_t *ix = d.indices + 3 * (size_t) i;
            const V3 p0(d.positions[3 * ix[0]], d.positions[3 * ix[0] + 1], d.positions[3 * ix[0] + 2]);
            const V3 p1(d.positions[3 * ix[1]], d.positions[3 * ix[1] + 1], d.positions[3 * ix[1] + 2]);
            const V3 p2(d.positions[3 * ix[2]], d.positions[3 * ix[2] + 1], d.positions[3 * ix[2] + 2]);
            const bool texcoords = sh.pad != 0;
            const detail::ShapeWords mw = shapeWordsOf(mats, sh.material);
            const uint32_t front = mw.front, back = mw.back;     /* (tagShadeClasses reads them back from the record) */
            uint32_t flags = (sh.hasNormals ? TS_VERTEX_NORMALS : 0u) | (texcoords ? TS_TEXCOORDS : 0u) | mw.flags;
            float4 *r = ts.data() + (size_t) stride * i;
            V2 t0(0, 0), t1(0, 0), t2(0, 0);
            if (texcoords) {
                const float *c0 = d.texcoords + 2 * (size_t) ix[0], *c1 = d.texcoords + 2 * (size_t) ix[1], *c2 = d.texcoords + 2 * (size_t) ix[2];
                t0 = V2(c0[0], c0[1]); t1 = V2(c1[0], c1[1]); t2 = V2(c2[0], c2[1]);
            }
            V3 n0(0.0f), n1(0.0f), n2(0.0f);
            if (sh.hasNormals) {
                n0 = V3(d.normals[3 * ix[0]], d.normals[3 * ix[0] + 1], d.normals[3 * ix[0] + 2]);
                n1 = V3(d.normals[3 * ix[1]], d.normals[3 * ix[1] + 1], d.normals[3 * ix[1] + 2]);
                n2 = V3(d.normals[3 * ix[2]], d.normals[3 * ix[2] + 1], d.normals[3 * ix[2] + 2]);
            }
            /* dpdu / dpdv (skdtree.h:378-379, or TriMesh::computeUVTangents) and the frame or the vertex normals: refit_hd.h, which the update's kernel runs too */
            V3 dpdu, dpdv, a, b, c;
            detail::triShadeGeometry(p0, p1, p2, texcoords, t0, t1, t2, sh.hasNormals != 0, n0, n1, n2, dpdu, dpdv, a, b, c);
            if (texcoords) {
                r[6] = make_float4(t0.x, t0.y, t1.x, t1.y);
                r[7] = make_float4(t2.x, t2.y, dpdu.x, dpdu.y);
                r[8] = make_float4(dpdu.z, dpdv.x, dpdv.y, dpdv.z);
            }
            r[0] = make_float4(p0.x, p0.y, p0.z, pm_from_bits(front));
            r[1] = make_float4(p1.x, p1.y, p1.z, pm_from_bits(back));
            r[2] = make_float4(p2.x, p2.y, p2.z, pm_from_bits((uint32_t) sh.emitter));
            r[3] = make_float4(a.x, a.y, a.z, pm_from_bits(flags));
            r[4] = make_float4(b.x, b.y, b.z, 0.0f);
            r[5] = make_float4(c.x, c.y, c.z, 0.0f);
        }
    }

    /* shade class of every triangle in the spare word of its Wald record(s): 0 diffuse, 1 rough conductor, 2 dielectric -- the heavier
       of the two sides of a two-sided surface; k_rays_w passes it on in the hit record and k_shade deals its lanes by it (k_pool.h) */
    void tagShadeClasses() {
        std::vector<uint8_t> &cls = triClass; cls.assign(d.n_triangles, 0);
        for (uint32_t i = 0; i < d.n_triangles; ++i) {
            const float4 *r = ts.data() + (size_t) stride * i;          /* front and back material: shadingRecords */
            cls[i] = (uint8_t) shadeClassOf(mats, pm_to_bits(r[0].w), pm_to_bits(r[1].w));
        }
        for (std::vector<float> *recs : { &sc->bvh.tris, &sc->bvh.wtris })
            for (size_t r = 0; r + 12 <= recs->size(); r += 12) {
                uint32_t prim; memcpy(&prim, &(*recs)[r + 10], 4);
                const uint32_t c = prim < d.n_triangles ? cls[prim] : 0u;
                memcpy(&(*recs)[r + 11], &c, 4);
            }
    }

    /* what the device holds beside the 8-wide tree the ray kernels walk (wideOnly) and whether that tree's depth fits their stacks */
    void chooseTraversal() {
        /* the compressed 8-wide tree: every scene the packed leaf table of the LDS-resident kernels does not serve (more than 64 Wald records) runs k_mega on the wide tree / k_rays_w.
           (The rule was "64 nodes of the 4-wide tree or more, or more than 64 records".  Its first half could not decide anything: with at most 64 records the binary tree has at
           most 63 inner nodes, a collapsed node that keeps an inner child absorbed three of them, so that tree never exceeded 42 nodes.) */
        if (sc->bvh.nWNodes == 0) {      /* a scene without triangles: one node without children (all-zero meta bytes hit nothing) -- the ray kernels need a root to reject */
            sc->bvh.wnodes.assign(20, 0u); sc->bvh.nWNodes = 1; sc->bvh.wMaxDepth = 1;
        }
        static_assert(FLAT2_LEAVES_MAX == 64 && LEAF_LIST_MAX == FLAT2_LEAVES_MAX, "the packed leaf table has one mask bit per record, two words; bvh.h collects the leaf list up to that size");
        sc->wideOnly = sc->bvh.tris.size() / 12 > FLAT2_LEAVES_MAX;
        /* ... and, round 6, EVERY scene has the wide tree on the device: the ray kernels of the wavefront path (k_rays_w) and phip_trace (k_raycast_w) walk nothing else.
           The LDS-resident scenes keep their records in the binary tree's leaf order and the packed leaf table for k_mega / k_shade_trace beside it */
        /* the stack of the wide tree: one group per level */
        if (!wideDepthFits(sc->bvh.wMaxDepth)) throw std::runtime_error("wide BVH too deep for the traversal stack");
    }

    /* packed emitter table (dv_scene.h: EmitterTab) */
    void packEmitterTable() {
        tab = ecdf;
        tab.resize(ecdf.size() + (size_t) EM_STRIDE * d.n_emitters, 0.0f);
        const size_t cdfBase = tab.size();
        size_t nEmTris = 0;
        auto isArea = [&](uint32_t i) { return ems[i].shape != 0xFFFFFFFFu; };
        for (uint32_t i = 0; i < d.n_emitters; ++i) if (isArea(i)) nEmTris += shapes[ems[i].shape].nTris;
        const size_t recBase = (cdfBase + areaCdf.size() + 3) / 4 * 4;                /* 16-byte aligned */
        const bool withRecs = recBase + nEmTris * 4 * TRISHADE_FLOAT4S <= EMITTER_LDS_FLOATS;
        size_t recPos = recBase;
        for (uint32_t i = 0; i < d.n_emitters; ++i) {
            float *r = tab.data() + ecdf.size() + (size_t) EM_STRIDE * i;
            for (int k = 0; k < 3; ++k) r[EM_RADIANCE + k] = ems[i].radiance[k];
            r[EM_WEIGHT] = ems[i].samplingWeight;
            r[EM_TYPE] = pm_from_bits(d.emitters[i].type);
            if (!isArea(i)) continue;
            const DevShape &sh = shapes[ems[i].shape];
            r[EM_FIRST_TRI] = pm_from_bits(sh.firstTri); r[EM_N_TRIS] = pm_from_bits(sh.nTris);
            r[EM_CDF] = pm_from_bits((uint32_t) (cdfBase + sh.cdfOffset));             /* area CDFs follow the records */
            r[EM_INV_AREA] = sh.invSurfaceArea;
            r[EM_REC] = pm_from_bits(withRecs ? (uint32_t) recPos : 0u);
            recPos += (size_t) sh.nTris * 4 * TRISHADE_FLOAT4S;
        }
        tab.insert(tab.end(), areaCdf.begin(), areaCdf.end());
        if (withRecs) {
            tab.resize(recBase, 0.0f);
            for (uint32_t i = 0; i < d.n_emitters; ++i) {
                if (!isArea(i)) continue;
                const DevShape &sh = shapes[ems[i].shape];
                for (uint32_t k = 0; k < sh.nTris; ++k) {       /* the first six float4s of each record (positions, normal / vertex normals) */
                    const float *src = (const float *) (ts.data() + (size_t) stride * (sh.firstTri + k));
                    tab.insert(tab.end(), src, src + 4 * TRISHADE_FLOAT4S);
                }
            }
        }
        if (tab.size() >= (1ull << 31)) throw std::runtime_error("emitter table too large");
        tab.resize((tab.size() + 3) / 4 * 4, 0.0f);              /* whole float4s: the shading kernels stage the table in LDS with 16-byte loads */
    }

    /* the environment emitter's bounding sphere (environmentSphereOf) */
    void environmentSphere() {
        if (envEmitter >= 0) environmentSphereOf(sc->bvh.sceneMin, sc->bvh.sceneMax, d.n_triangles, d.camera, D);
    }

    /* EnvironmentMap::configure, envmap.cpp:262-328: the pyramid's texels, marginal / conditional CDFs over luminance * sin(theta), the transforms */
    void buildEnvmap() {
        if (!envIsMap) return;
        const phip_envmap &e = d.envmap;
        if (!e.texels || e.width == 0 || e.height == 0) throw std::runtime_error("envmap emitter without texels");
        if (std::max(e.width, e.height) > 0xFFFF) throw std::runtime_error("Environment maps images must be smaller than 65536 pixels in width and height");
        const int w = (int) e.width, h = (int) e.height;
        std::vector<float4> &tex = envTexels;
        tex.resize((size_t) w * h);
        for (size_t i = 0; i < tex.size(); ++i) tex[i] = make_float4(e.texels[3 * i], e.texels[3 * i + 1], e.texels[3 * i + 2], 0.0f);
        /* MIP pyramid + EWA weight table */
        DevMipLevels &lv = envLevels; memset(&lv, 0, sizeof(lv));
        lv.bcu = PHIP_WRAP_REPEAT; lv.bcv = PHIP_WRAP_CLAMP; lv.filterType = PHIP_FILTER_EWA; lv.maxAnisotropy = 10.0f;   /* envmap.cpp:138-139,176-178 */
        pyramidLevels(lv, w, h, e.n_levels, PHIP_ENVMAP_MAX_LEVELS, "envmap");
        for (int l = 1; l < lv.nLevels; ++l) {
            if (!e.levels[l]) throw std::runtime_error("envmap: level pointer is NULL");
            lv.offset[l] = (uint32_t) tex.size();
            const size_t cnt = (size_t) lv.lw[l] * lv.lh[l];
            for (size_t i = 0; i < cnt; ++i) tex.push_back(make_float4(e.levels[l][3 * i], e.levels[l][3 * i + 1], e.levels[l][3 * i + 2], 0.0f));
        }
        ewaWeightLut(lv.weightLut);
        sc->envLevelCount = lv.nLevels;
        std::vector<float> &cdfCols = envCdfCols, &cdfRows = envCdfRows, &rowWeights = envRowWeights;
        cdfCols.resize((size_t) (w + 1) * h); cdfRows.resize((size_t) h + 1); rowWeights.resize((size_t) h);
        /* the conditional and the marginal CDF: appearance_hd.h, which the kernels of phip_scene_update_appearance run too */
        std::vector<float> rowTerms((size_t) h);
        for (int y = 0; y < h; ++y) rowTerms[y] = detail::envmapRowCdf(tex.data() + (size_t) y * w, w, h, y, cdfCols.data() + (size_t) y * (w + 1), &rowWeights[y]);
        const float rowSum = detail::envmapMarginalCdf(rowTerms.data(), h, cdfRows.data());
        envmapConstants(e, rowSum, D.env);
    }

    /* the plain-data fields of the DevScene: counts, box, camera, film; the scalar copy of the descriptor */
    void sceneConstants() {
        D.nMaterials = (uint32_t) mats.size(); D.triShadeStride = sc->triShadeStride;
        D.emitterTabSize = (uint32_t) tab.size();
        D.nEmitters = d.n_emitters; D.emitterNormalization = emNorm;
        D.envEmitter = envEmitter;
        D.nTriangles = d.n_triangles;
        for (int a = 0; a < 3; ++a) { D.sceneMin[a] = sc->bvh.sceneMin[a]; D.sceneMax[a] = sc->bvh.sceneMax[a]; }
        setupCamera(d.camera, d.film, D.cam);
        D.film.width = d.film.crop_width; D.film.height = d.film.crop_height;
        D.film.radius = d.film.filter_radius;
        D.film.scaleFactor = PHIP_FILTER_RESOLUTION / d.film.filter_radius;     /* rfilter.cpp:50 */
        D.film.border = (int) std::ceil(d.film.filter_radius - 0.5f);           /* rfilter.cpp:51 */
        D.film.blockSize = 32;
        for (int i = 0; i <= PHIP_FILTER_RESOLUTION; ++i) D.film.table[i] = d.film.filter_table[i];
        sc->descCopy = d;
        sc->descCopy.positions = nullptr; sc->descCopy.normals = nullptr; sc->descCopy.indices = nullptr;
        sc->descCopy.shapes = nullptr; sc->descCopy.materials = nullptr; sc->descCopy.emitters = nullptr;
    }

    /* LDS staging plan: the top of the wide tree for the ray kernels (its nodes are in breadth-first order); for the LDS-resident kernels every Wald record, if the
       scene has a leaf list -- and what follows from it for the fused kernel */
    void ldsPlan() {
        const HostBVH &bvh = sc->bvh;
        /* (recordsInLds: the packed leaf table and every Wald record are staged in LDS -- also true of small scenes with glass, copper, textures or an environment
           emitter, which k_shade_trace serves on the same table: k_shade_trace.h.  A scene that is ONE leaf has no leaf list, bvh.h: the ray kernels serve it) */
        recordsInLds = !sc->wideOnly && !bvh.leaves.empty() && bvh.tris.size() / 12 <= TRI_CACHE_MAX;
        D.triCache = recordsInLds ? (uint32_t) (bvh.tris.size() / 12) : 0u;
        D.preclip = 1u;                          /* k_rays_w traverses rays the shading kernels have clipped (k_clip.h) */
        /* the fused kernel's LDS plan (k_mega.h): the leaf table, every Wald and shading record, the emitter table and the materials in LDS (phip_mega.hip); leaf BSDF
           models: any (round 5) */
        fitsLdsBase = !sc->hasTextures && envEmitter < 0 && stride == TRISHADE_FLOAT4S
            && recordsInLds && d.n_triangles <= MEGA_TRISHADE_MAX
            && tab.size() <= EMITTER_LDS_FLOATS && mats.size() <= MATERIAL_LDS_MAX;
    }

    /* the leaf list (bvh.h) in the packed form with record masks (k_traverse.h: flat2Pass1).  A leaf reference is
       ~((first record << 3) | records - 1); a triangle referenced by several leaves (spatial splits) has one record per
       reference -- the copies carry the same 12 words, so only the first copy's bit is set.
       Round 5: 33..64 records keep the packed form with a two-word mask (flatMode 3; the centre / half-extent table of the dealt
       traversal only -- the high word rides in the centre's spare word) */
    void packLeafTable() {
        const size_t nRec = sc->bvh.tris.size() / 12;
        std::vector<uint32_t> firstCopy(nRec);
        for (size_t i = 0; i < nRec; ++i) {
            firstCopy[i] = (uint32_t) i;
            for (size_t j = 0; j < i; ++j) if (!memcmp(&sc->bvh.tris[12 * i], &sc->bvh.tris[12 * j], 48)) { firstCopy[i] = (uint32_t) j; break; }
        }
        for (const HostBVH::LeafBox &leaf : sc->bvh.leaves) {
            const uint32_t r = ~(uint32_t) leaf.ref, first = r >> 3, count = (r & 7u) + 1u;
            unsigned long long bits64 = 0;
            for (uint32_t i = 0; i < count; ++i) bits64 |= 1ull << firstCopy[first + i];
            const uint32_t bits = (uint32_t) bits64, bitsHi = (uint32_t) (bits64 >> 32);
            /* centre / half extent (k_traverse.h: flat2Pass1).  c -+ h must cover the (padded) box whatever the rounding of c, and the
               distances c' -+ h |rcp| are rounded differently from the plane form the pad of bvh.h was sized for (two roundings of
               magnitude |c rcp| + |o rcp| instead of one): h gets the rounding of c and another 4e-6 of the scene's extent on top */
            const float ext = std::max(sc->bvh.tightMax[0] - sc->bvh.tightMin[0], std::max(sc->bvh.tightMax[1] - sc->bvh.tightMin[1], sc->bvh.tightMax[2] - sc->bvh.tightMin[2]));
            const float camMax = std::max(std::fabs(d.camera.to_world[3]), std::max(std::fabs(d.camera.to_world[7]), std::fabs(d.camera.to_world[11])));
            float c[3], h[3];
            /* (the arithmetic: detail::leafCentreHalf, refit_hd.h -- h = nextafter(need) + 2.4e-7 |c| + 4e-6 ext + 4.8e-7 camMax, need = the larger distance from c to a face) */
            {
                /* ... and the rounding of o rcp, which grows with the ORIGIN's magnitude (two roundings of |o rcp| move a plane by ~2^-23 |o|): the only rays
                   that start outside the scene box are the camera's, so the camera position pays for it (a camera 60 scene extents away used to lose
                   leaf boxes; tests/test_gpu_parity.py: far camera) */
                detail::leafCentreHalf(leaf.mn, leaf.mx, ext, camMax, c, h);      /* (the camera's largest component on every axis: bvh.h, buildBVH) */
            }
            flat.push_back(make_float4(c[0], c[1], c[2], pm_from_bits(bitsHi)));
            flat.push_back(make_float4(h[0], h[1], h[2], pm_from_bits(bits)));
        }
    }

    /* for trees of few leaves (the Cornell box: 17), the leaves as a table: the LDS-resident kernels test every leaf box in one uniform pass, no walk.
       flatMode: 0 no table, 2 / 3 the packed form of at most 32 / 64 Wald records (1 was a table of plain boxes; its kernel is retired) */
    void flatLeafTable() {
        if (recordsInLds) packLeafTable();
        D.flatMode = flat.empty() ? 0u : (sc->bvh.tris.size() / 12 <= 32 ? 2u : 3u); D.nFlatLeaves = (uint32_t) (flat.size() / 2);
    }

    void chooseDevicePaths() { devicePathsOf(sc, D, fitsLdsBase); }

    /* the topology a later phip_scene_update keeps fixed (SceneUpdateState); before uploadScene releases the builder's arrays */
    void keepForUpdate() {
        SceneUpdateState &U = sc->upd;
        const HostBVH &bvh = sc->bvh;
        U.nVertices = d.n_vertices; U.nTriangles = d.n_triangles; U.hasNormals = d.normals != nullptr;
        U.indices.assign(d.indices, d.indices + 3 * (size_t) d.n_triangles);
        U.hadRecord.assign(((size_t) d.n_triangles + 31) / 32 + 1, 0u);
        auto prims = [&](const std::vector<float> &recs, std::vector<uint32_t> &out) {
            out.resize(recs.size() / 12);
            for (size_t r = 0; r < out.size(); ++r) {
                memcpy(&out[r], &recs[12 * r + 10], 4);
                if (out[r] < d.n_triangles) U.hadRecord[out[r] >> 5] |= 1u << (out[r] & 31u);
            }
        };
        prims(bvh.wtris, U.wRecPrim);
        if (!sc->wideOnly) prims(bvh.tris, U.recPrim);
        U.wLevels = bvh.wLevels; U.triClass = triClass;
        if (!flat.empty()) for (const HostBVH::LeafBox &leaf : bvh.leaves) U.leafRefs.push_back(leaf.ref);
        for (uint32_t i = 0; i < d.n_emitters; ++i) {
            if (ems[i].shape == 0xFFFFFFFFu) continue;
            const DevShape &sh = shapes[ems[i].shape];
            SceneUpdateState::EmitterMesh m = { i, sh.firstTri, sh.nTris, 0xFFFFFFFFu, 0u };
            for (size_t k = 3 * (size_t) sh.firstTri; k < 3 * (size_t) (sh.firstTri + sh.nTris); ++k) { m.firstVertex = std::min(m.firstVertex, d.indices[k]); m.endVertex = std::max(m.endVertex, d.indices[k] + 1u); }
            U.emitterMeshes.push_back(m);
        }
        U.tab = tab; U.ecdfSize = ecdf.size();
        keepAppearance();
    }
    /* ... and the look a later phip_scene_update_appearance starts from (SceneUpdateState::Appearance); host arrays only */
    void keepAppearance() {
        SceneUpdateState::Appearance &P = sc->upd.app;
        P.shapes = shapes; P.texDesc = texDesc; P.texMax = texMax; P.envLevels = envLevels; P.envIsMap = envIsMap;
        P.materials.assign(d.materials, d.materials + (d.materials ? d.n_materials : 0)); P.emitters.assign(d.emitters, d.emitters + (d.emitters ? d.n_emitters : 0));
    }

    /* every immutable scene buffer of the device (placeholders where a kernel argument must not be NULL), the DevScene's pointers, the per-device counters */
    void uploadScene() {
        HostBVH &bvh = sc->bvh;
        HIP_TRY(hipSetDevice(sd.device));
        if (ts.empty()) sd.triShade.alloc(TRISHADE_FLOAT4S_UV); else sd.triShade.upload(ts.data(), ts.size());
        if (texTexels.empty()) sd.texTexels.alloc(1); else sd.texTexels.upload(texTexels.data(), texTexels.size());
        if (texDesc.empty()) sd.texDesc.alloc(1); else sd.texDesc.upload(texDesc.data(), texDesc.size());
        if (WIDE_NODE_STRIDE == 5) sd.wnodes.upload((const uint4 *) bvh.wnodes.data(), bvh.wnodes.size() / 4);
        else {                                                   /* one node per WIDE_NODE_STRIDE * 16 bytes (a 128-byte line) */
            const size_t n = bvh.wnodes.size() / 20;
            std::vector<uint4> padded(n * WIDE_NODE_STRIDE, make_uint4(0, 0, 0, 0));
            for (size_t i = 0; i < n; ++i) memcpy(&padded[i * WIDE_NODE_STRIDE], &bvh.wnodes[i * 20], 80);
            sd.wnodes.upload(padded.data(), padded.size());
        }
        if (bvh.wtris.empty()) sd.wtris.alloc(3); else sd.wtris.upload((const float4 *) bvh.wtris.data(), bvh.wtris.size() / 4);
        sd.trisAreWide = sc->wideOnly;                           /* DevScene::tris = wtris: SceneDev::bind */
        if (sc->wideOnly) sd.tris.alloc(3); else sd.tris.upload((const float4 *) bvh.tris.data(), bvh.tris.size() / 4);
        sd.materials.upload(mats.data(), mats.size());
        sd.emitterTab.upload(tab.data(), tab.size());
        if (envIsMap) {
            sd.envLevels.upload(&envLevels, 1);
            sd.envTexels.upload(envTexels.data(), envTexels.size());
            sd.envCdfRows.upload(envCdfRows.data(), envCdfRows.size()); sd.envCdfCols.upload(envCdfCols.data(), envCdfCols.size());
            sd.envRowWeights.upload(envRowWeights.data(), envRowWeights.size());
        }
        if (flat.empty()) sd.flatLeaves.alloc(2); else sd.flatLeaves.upload(flat.data(), flat.size());
        sd.bind();
        sd.allocCounters();
        std::vector<float>().swap(bvh.tris);                    /* keep the statistics, drop the arrays */
        std::vector<uint32_t>().swap(bvh.wnodes); std::vector<float>().swap(bvh.wtris);
        HIP_TRY(hipHostMalloc((void **) &sc->cancelFlag, sizeof(int), hipHostMallocPortable | hipHostMallocMapped));
        *sc->cancelFlag = 0;
    }
};

/* phip_scene_create: descriptor -> host arrays -> the decisions which kernels serve the scene -> one upload */
static void buildScene(phip_scene *sc, const phip_scene_desc &d) {
    SceneBuild B(sc, d);
    B.validateDesc();
    B.flattenShapes(); B.packTextures(); B.materials(); B.emitterSelection();
    B.buildAccel();
    B.shadingRecords(); B.tagShadeClasses();
    B.chooseTraversal();
    B.packEmitterTable(); B.environmentSphere(); B.buildEnvmap();
    B.sceneConstants();
    B.ldsPlan(); B.flatLeafTable(); B.chooseDevicePaths();
    B.keepForUpdate();
    B.uploadScene();
}

/* Byte tables of the Sobol' direction numbers (dv_math.h: SobolTab::matBt / vdcBt / vdcInvBt): entry [v] of byte b = the XOR of the rows 8 b + j over the
   set bits j of v, built as entry [v without its lowest set bit] ^ row 8 b + that bit.  `rows2` = the two enumeration rows (vdc, then vdc_inv), 52 words each. */
static void buildSobolByteTables(const uint32_t *matrices, size_t dims, const unsigned long long *rows2, std::vector<uint32_t> &bt, std::vector<unsigned long long> &vb) {
    bt.assign(dims * SOBOL_BT_BYTES * 256u, 0u);
    for (size_t d = 0; d < dims; ++d)
        for (uint32_t b = 0; b < SOBOL_BT_BYTES; ++b) {
            uint32_t *t = &bt[(d * SOBOL_BT_BYTES + b) * 256u];
            for (uint32_t x = 1; x < 256u; ++x) {
                const uint32_t j = 8u * b + (uint32_t) __builtin_ctz(x);
                /* (sampleSingle indexes matrices[i + dimension * 52] for every set bit i of the index: above bit 51 that is the next dimension's rows) */
                const size_t row = d * PHIP_SOBOL_MATRIX_SIZE + j;
                t[x] = t[x & (x - 1u)] ^ (row < dims * PHIP_SOBOL_MATRIX_SIZE ? matrices[row] : 0u);
            }
        }
    vb.assign((4u + 7u) * 256u, 0ull);
    for (uint32_t b = 0; b < 4u + 7u; ++b) {
        const unsigned long long *rows = b < 4u ? rows2 : rows2 + PHIP_SOBOL_MATRIX_SIZE;
        const uint32_t bb = b < 4u ? b : b - 4u;
        unsigned long long *t = &vb[(size_t) b * 256u];
        for (uint32_t x = 1; x < 256u; ++x) {
            const uint32_t j = 8u * bb + (uint32_t) __builtin_ctz(x);
            t[x] = t[x & (x - 1u)] ^ (j < (uint32_t) PHIP_SOBOL_MATRIX_SIZE ? rows[j] : 0ull);
        }
    }
}

/* Multi-digit tables of the radical inverses (dv_math.h: RinvTab::dimInfo / chunk / fac / pw) for the leading dimensions whose base is below 1024 (at most
   RINV_TAB_DIMS): the permuted value of every chunk of k digits, the float factors radical^m as the digit loop multiplies them up, the powers base^n */
static uint32_t buildRinvTables(const uint32_t *primes, const uint16_t *perm /* concatenated, or NULL */, const uint32_t *permOffset, uint32_t dims,
                                std::vector<uint32_t> &dimInfo, std::vector<uint32_t> &chunk, std::vector<float> &fac, std::vector<uint32_t> &pw) {
    uint32_t nd = 0;
    while (nd < dims && nd < RINV_TAB_DIMS && primes[nd] < 1024u) ++nd;
    dimInfo.assign((size_t) 8 * nd, 0u); chunk.clear(); fac.assign((size_t) RINV_FAC_STRIDE * nd, 0.0f); pw.assign((size_t) RINV_PW_STRIDE * nd, 0u);
    for (uint32_t d = 0; d < nd; ++d) {
        const uint32_t base = primes[d];
        const uint16_t *P = perm ? perm + permOffset[d] : nullptr;
        uint32_t k = 1, B = base;
        while ((unsigned long long) B * base <= 1024ull && k < RINV_PW_STRIDE - 1u) { B *= base; ++k; }
        const uint32_t first = (uint32_t) chunk.size();
        dimInfo[8 * d] = base; dimInfo[8 * d + 1] = B; dimInfo[8 * d + 2] = k | (first << 8);
        dimInfo[8 * d + 3] = (uint32_t) ((1ull << 32) / B) + 1u;
        for (uint32_t c = 0; c < B; ++c) {
            uint32_t vFull = 0, vSig = 0, n = 0, t = c;
            for (uint32_t j = 0; j < k; ++j) { const uint32_t digit = t % base; t /= base; vFull = vFull * base + (P ? (uint32_t) P[digit] : digit); }
            for (t = c; t; t /= base, ++n) { const uint32_t digit = t % base; vSig = vSig * base + (P ? (uint32_t) P[digit] : digit); }
            chunk.push_back(vFull | (vSig << 10) | (n << 20));
        }
        const float radical = 1.0f / (float) (int) base;
        const float tail = P ? radical * (float) (int) P[0] / (1.0f - radical) : 0.0f;        /* the constant of scrambledRadicalInverse, by its own expression */
        dimInfo[8 * d + 4] = pm_to_bits(radical); dimInfo[8 * d + 5] = pm_to_bits(tail);
        float f = 1.0f;
        for (uint32_t m = 0; m < RINV_FAC_STRIDE; ++m) { fac[(size_t) RINV_FAC_STRIDE * d + m] = f; f *= radical; }
        uint32_t pwr = 1;
        for (uint32_t n = 0; n <= k; ++n) { pw[(size_t) RINV_PW_STRIDE * d + n] = pwr; pwr *= base; }
    }
    return nd;
}

/* 64-bit content key of a caller's table (word-wise multiply-xorshift; ~2 GB/s: 0.1 ms for the Sobol direction numbers) */
static uint64_t contentHash(const void *data, size_t bytes, uint64_t h) {
    const unsigned char *b = (const unsigned char *) data;
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, b + i, 8); h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    uint64_t w = 0; if (i < bytes) memcpy(&w, b + i, bytes - i);
    h = (h ^ w ^ (uint64_t) bytes) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 29;
    return h ? h : 1;
}

/* Replica of the scene on another GPU: device-to-device copies of the immutable arrays (xGMI), same DevScene. */
static SceneDev *replicateScene(phip_scene *sc, int device) {
    SceneDev &src = *sc->devs[0];
    std::unique_ptr<SceneDev> dst(new SceneDev());
    dst->device = device;
    HIP_TRY(hipSetDevice(device));
    SceneDev::forEachSceneBuffer([&](auto buf) { ((*dst).*buf).cloneFrom(src.*buf); });
    dst->trisAreWide = src.trisAreWide;
    dst->dev = src.dev;
    dst->bind();
    dst->allocCounters();
    HIP_TRY(hipDeviceSynchronize());
    sc->devs.emplace_back(std::move(dst));
    return sc->devs.back().get();
}

/* The scene's replicas for a device list: position i of the list renders on devs[i].  The list is checked before anything is replicated -- devices[0] is the
   scene's device, every ordinal is in [0, visible): the text of what is wrong with it is returned and nothing has happened --; then replicas are kept while
   they match the list, and a different list rebuilds them from its first mismatch.  nullptr: devs[0 .. n) serve the list.  The caller holds the render lock. */
static const char *ensureReplicas(phip_scene *sc, const int *devices, int n) {
    int visible = 0; HIP_TRY(hipGetDeviceCount(&visible));
    if (devices[0] != sc->devs[0]->device) return "devices[0] must be the scene's device";
    for (int i = 0; i < n; ++i) if (devices[i] < 0 || devices[i] >= visible) return "device ordinal out of range";
    for (int i = 1; i < n; ++i) {
        if ((int) sc->devs.size() > i && sc->devs[i]->device == devices[i]) continue;
        if ((int) sc->devs.size() > i) sc->devs.resize(i);          /* a different device list: rebuild from here */
        replicateScene(sc, devices[i]);
    }
    return nullptr;
}

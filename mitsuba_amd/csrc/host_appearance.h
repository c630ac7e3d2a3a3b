/*
 * host_appearance.h -- host side of phip_scene_update_appearance: new materials, emitter radiances and weights, texture contents and a new environment map on the
 * scene as created.  The geometry, the tree and every count stay; what restates a material, an emitter, a texture or the map in the device arrays is rewritten
 * where it is -- the DevMaterial array and the emitter table by the creation's own stages (host_scene.h: convertMaterials, shapeWordsOf,
 * emitterCdfOf, devicePathsOf), the per-triangle words, the texels and the map's CDFs by the kernels of k_appearance.h around the arithmetic of appearance_hd.h that
 * the creation runs too.  So every entry point gives the bits it gives on a scene created with the new look.
 * Order: the checks that need no device (appearanceArgs), the caller's texels to the device (device_pointers = 0: the same kernels run on the uploaded copy),
 * the new textures' maxima, the material / emitter stages (appearanceLook), the environment map into FRESH buffers and its refusals -- and only then the writes.
 * Host code only; included by phip.hip alone, after host_update.h.  The caller holds the scene's render lock and has made the scene's device current.
 */
#pragma once
#include "host_update.h"

/* the look after the call: what SceneUpdateState::Appearance keeps, and what the creation's stages derive from it */
struct AppearanceLook {
    std::vector<phip_material> materials; std::vector<phip_emitter> emitters; std::vector<DevMipLevels> texDesc; std::vector<float> texMax;
    std::vector<DevMaterial> mats; int mask = 0; std::vector<detail::ShapeWords> words;        /* per shape */
    std::vector<float> ecdf; float emNorm = 0;
};

/* the complete pyramid of a texture or the map, as the creation checks it; the level count */
static int appearanceLevels(uint32_t w, uint32_t h, uint32_t nLevels, int maxLevels, const char *what) {
    DevMipLevels lv; memset(&lv, 0, sizeof(lv));
    pyramidLevels(lv, (int) w, (int) h, nLevels, maxLevels, what);
    return lv.nLevels;
}

/* the refusals that need neither a device nor the texels: counts, what has to be the creation's, NULL level pointers, the sampling settings.  Fills L.texDesc */
static void appearanceArgs(const phip_scene *sc, const phip_appearance_desc &a, AppearanceLook &L) {
    const SceneUpdateState::Appearance &P = sc->upd.app;
    if (a.materials && a.n_materials != P.materials.size()) throw std::runtime_error("n_materials is not the scene's");
    if (a.emitters && a.n_emitters != P.emitters.size()) throw std::runtime_error("n_emitters is not the scene's");
    if (a.textures && a.n_textures != P.texDesc.size()) throw std::runtime_error("n_textures is not the scene's");
    if (a.emitters)
        for (uint32_t i = 0; i < a.n_emitters; ++i)
            if (a.emitters[i].type != P.emitters[i].type || (a.emitters[i].type == PHIP_EMITTER_AREA && a.emitters[i].shape != P.emitters[i].shape))
                throw std::runtime_error("emitter " + std::to_string(i) + ": type and shape must be the creation's");
    L.texDesc = P.texDesc;
    if (a.textures)
        for (uint32_t i = 0; i < a.n_textures; ++i) {
            const phip_texture &t = a.textures[i];
            if (t.width == 0) continue;
            const DevMipLevels &lv = P.texDesc[i];
            if ((int) t.width != lv.lw[0] || (int) t.height != lv.lh[0] || t.height == 0 || appearanceLevels(t.width, t.height, t.n_levels, PHIP_MIP_MAX_LEVELS, "texture") != lv.nLevels)
                throw std::runtime_error("texture " + std::to_string(i) + ": width, height and n_levels must be the creation's");
            if (!t.levels[0]) throw std::runtime_error("texture without level 0");
            for (int l = 1; l < lv.nLevels; ++l) if (!t.levels[l]) throw std::runtime_error("texture: level pointer is NULL");
            textureSampling(t, L.texDesc[i]);
        }
    if (a.envmap) {
        const phip_envmap &e = *a.envmap;
        if (!P.envIsMap) throw std::runtime_error("envmap for a scene that was created without an envmap emitter");
        if (!e.texels || e.width == 0 || e.height == 0) throw std::runtime_error("envmap emitter without texels");
        const DevMipLevels &lv = P.envLevels;
        if ((int) e.width != lv.lw[0] || (int) e.height != lv.lh[0] || appearanceLevels(e.width, e.height, e.n_levels, PHIP_ENVMAP_MAX_LEVELS, "envmap") != lv.nLevels)
            throw std::runtime_error("envmap: width, height and n_levels must be the creation's");
        for (int l = 1; l < lv.nLevels; ++l) if (!e.levels[l]) throw std::runtime_error("envmap: level pointer is NULL");
    }
}

/* the creation's material and emitter stages on the new look; L.texMax holds the maxima of the textures as they will be */
static void appearanceLook(const phip_scene *sc, const phip_appearance_desc &a, AppearanceLook &L) {
    const SceneUpdateState::Appearance &P = sc->upd.app;
    L.materials = P.materials; L.emitters = P.emitters;
    if (a.materials) L.materials.assign(a.materials, a.materials + a.n_materials);
    if (a.emitters)
        for (uint32_t i = 0; i < a.n_emitters; ++i) {
            for (int k = 0; k < 3; ++k) L.emitters[i].radiance[k] = a.emitters[i].radiance[k];
            L.emitters[i].sampling_weight = a.emitters[i].sampling_weight;
        }
    if (a.materials || a.textures) {
        L.mats = convertMaterials(L.materials.data(), (uint32_t) L.materials.size(), &L.texMax);
        requireTexcoordsOfAnisotropic(L.materials.data(), (uint32_t) L.materials.size(), P.shapes);
        L.mask = materialMaskOf(L.mats);
        L.words.resize(P.shapes.size());
        for (size_t i = 0; i < P.shapes.size(); ++i) L.words[i] = shapeWordsOf(L.mats, P.shapes[i].material);
    }
    if (a.emitters) L.emNorm = emitterCdfOf(L.emitters.data(), (uint32_t) L.emitters.size(), L.ecdf);
}

/* a refusal of the stages above: the creation's message and the creation's code (an unsupported microfacet distribution: PHIP_ERR_UNSUPPORTED) */
template <typename Stage> static int appearanceRefusal(Stage stage) {
    try { stage(); return PHIP_OK; }
    catch (const std::invalid_argument &e) { return setErr(PHIP_ERR_UNSUPPORTED, std::string("phip_scene_update_appearance: ") + e.what()); }
    catch (const std::runtime_error &e) { return setErr(PHIP_ERR_INVALID, std::string("phip_scene_update_appearance: ") + e.what()); }
}

static bool appearanceEmpty(const phip_appearance_desc *a) { return !a || (!a->materials && !a->emitters && !a->textures && !a->envmap); }

static int updateAppearance(phip_scene *sc, const phip_appearance_desc &a, phip_appearance_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::string who = "phip_scene_update_appearance: ";
    SceneUpdateState &U = sc->upd;
    SceneUpdateState::Appearance &P = U.app;
    SceneDev &sd = *sc->devs[0];
    DevScene &D = sd.dev;
    AppearanceLook L;
    if (int rc = appearanceRefusal([&] { appearanceArgs(sc, a, L); })) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const AppearanceKernels K = phipAppearanceKernels();
    auto blocks = [](size_t items) { return dim3((unsigned) ((items + APP_BLOCK - 1) / APP_BLOCK)); };

    /* ---- the caller's texel arrays, on the device: (texture or -1 = the map, level, source) ---- */
    struct Source { int texture, level; const float *p; size_t texels; };
    std::vector<Source> sources;
    if (a.textures)
        for (uint32_t i = 0; i < a.n_textures; ++i)
            if (a.textures[i].width)
                for (int l = 0; l < P.texDesc[i].nLevels; ++l) sources.push_back({ (int) i, l, a.textures[i].levels[l], (size_t) P.texDesc[i].lw[l] * P.texDesc[i].lh[l] });
    if (a.envmap)
        for (int l = 0; l < P.envLevels.nLevels; ++l) sources.push_back({ -1, l, l ? a.envmap->levels[l] : a.envmap->texels, (size_t) P.envLevels.lw[l] * P.envLevels.lh[l] });
    if (a.device_pointers) {
        for (const Source &s : sources)
            if (!onSceneDevice(s.p, sd.device)) return setErr(PHIP_ERR_INVALID, who + "device_pointers = 1, but a texel pointer is not device memory of the scene's device");
        HIP_TRY(hipStreamSynchronize((hipStream_t) a.stream));           /* ordered after the caller's producer */
    } else {
        size_t total = 0;
        for (const Source &s : sources) total += 3 * s.texels;
        P.dScratch.alloc(total);
        size_t at = 0;
        for (Source &s : sources) {
            HIP_TRY(hipMemcpy(P.dScratch.p + at, s.p, 3 * s.texels * sizeof(float), hipMemcpyHostToDevice));
            s.p = P.dScratch.p + at; at += 3 * s.texels;
        }
    }
    EventList ev;

    /* ---- validate: nothing of the scene is written before the last refusal ---- */
    L.texMax = P.texMax;
    if (a.textures && !L.texMax.empty()) {
        P.dTexMax.alloc(L.texMax.size());
        HIP_TRY(hipMemsetAsync(P.dTexMax.p, 0, L.texMax.size() * sizeof(uint32_t), 0));          /* +0: where packTextures starts */
        ev.record(0);
        for (const Source &s : sources)
            if (s.texture >= 0 && s.level == 0)
                hipLaunchKernelGGL(K.texmax, dim3(std::min(1024u, blocks(s.texels).x)), dim3(APP_BLOCK), 0, 0, s.p, (uint32_t) s.texels, P.dTexMax.p + s.texture);
        ev.record(0);
        std::vector<float> mx(L.texMax.size());
        HIP_TRY(hipMemcpy(mx.data(), P.dTexMax.p, mx.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipGetLastError());
        for (uint32_t i = 0; i < a.n_textures; ++i) if (a.textures[i].width) L.texMax[i] = mx[i];
    }
    if (int rc = appearanceRefusal([&] { appearanceLook(sc, a, L); })) return rc;
    /* the environment map: texels and CDFs into fresh buffers -- the refusal of a black or non-finite map needs the CDF's total */
    DevBuf<float4> envTexels; DevBuf<float> envCdfRows, envCdfCols, envRowWeights;
    DevEnvMap E = D.env;
    if (a.envmap) {
        const DevMipLevels &lv = P.envLevels;
        const int w = lv.lw[0], h = lv.lh[0];
        envTexels.alloc(sd.envTexels.n); envCdfRows.alloc((size_t) h + 1); envCdfCols.alloc((size_t) (w + 1) * h); envRowWeights.alloc((size_t) h);
        P.dRowTerms.alloc((size_t) h); P.dRowSum.alloc(1);
        ev.record(0);
        for (const Source &s : sources)
            if (s.texture < 0) hipLaunchKernelGGL(K.texels, blocks(s.texels), dim3(APP_BLOCK), 0, 0, s.p, envTexels.p + lv.offset[s.level], (uint32_t) s.texels);
        hipLaunchKernelGGL(K.envRows, dim3((unsigned) ((h + 63) / 64)), dim3(64), 0, 0, (const float4 *) envTexels.p, w, h, envCdfCols.p, envRowWeights.p, P.dRowTerms.p);
        hipLaunchKernelGGL(K.envMarginal, dim3(1), dim3(64), 0, 0, (const float *) P.dRowTerms.p, h, envCdfRows.p, P.dRowSum.p);
        ev.record(0);
        float rowSum = 0;
        HIP_TRY(hipMemcpy(&rowSum, P.dRowSum.p, sizeof(rowSum), hipMemcpyDeviceToHost));
        HIP_TRY(hipGetLastError());
        if (int rc = appearanceRefusal([&] { envmapConstants(*a.envmap, rowSum, E); })) return rc;
    }

    /* ---- write (nothing below fails but the runtime) ---- */
    const bool newMaterials = a.materials || a.textures;
    const bool maskChanged = newMaterials && L.mask != sc->materialMask;
    ev.record(0);
    if (a.textures) {
        for (const Source &s : sources)
            if (s.texture >= 0) hipLaunchKernelGGL(K.texels, blocks(s.texels), dim3(APP_BLOCK), 0, 0, s.p, sd.texTexels.p + P.texDesc[s.texture].offset[s.level], (uint32_t) s.texels);
        if (!L.texDesc.empty()) sd.texDesc.upload(L.texDesc.data(), L.texDesc.size());
    }
    if (newMaterials) {
        sd.materials.upload(L.mats.data(), L.mats.size());
        sc->materialMask = L.mask;
        devicePathsOf(sc, D, sc->fitsLds);          /* dealDwords and shadeSort follow the mask; what follows from counts comes out as it was */
        if (U.nTriangles > 0) {
            updateDeviceTables(sc);
            if (P.dTriShape.n != U.nTriangles) {          /* the triangle -> shape map: uploaded once and kept */
                std::vector<uint32_t> triShape(U.nTriangles);
                for (size_t i = 0; i < P.shapes.size(); ++i) for (uint32_t j = 0; j < P.shapes[i].nTris; ++j) triShape[P.shapes[i].firstTri + j] = (uint32_t) i;
                P.dTriShape.upload(triShape.data(), triShape.size());
            }
            P.dShapeWords.upload(L.words.data(), L.words.size());
            U.rb.triClass.alloc(U.nTriangles);          /* phip_scene_rebuild tags its next tree from this array (host_rebuild.h) */
            hipLaunchKernelGGL(K.records, blocks(U.nTriangles), dim3(APP_BLOCK), 0, 0, sd.triShade.p, sc->triShadeStride, U.nTriangles, (const uint32_t *) P.dTriShape.p,
                               (const detail::ShapeWords *) P.dShapeWords.p, U.rb.triClass.p);
            if (!U.wRecPrim.empty()) hipLaunchKernelGGL(K.classes, blocks(U.wRecPrim.size()), dim3(APP_BLOCK), 0, 0, sd.wtris.p, (const uint32_t *) U.dWRecPrim.p, (uint32_t) U.wRecPrim.size(), (const uint8_t *) U.rb.triClass.p, U.nTriangles);
            if (!U.recPrim.empty()) hipLaunchKernelGGL(K.classes, blocks(U.recPrim.size()), dim3(APP_BLOCK), 0, 0, sd.tris.p, (const uint32_t *) U.dRecPrim.p, (uint32_t) U.recPrim.size(), (const uint8_t *) U.rb.triClass.p, U.nTriangles);
        }
        /* the copies of the emitter meshes' records inside the emitter table (packEmitterTable): the same three words */
        for (const SceneUpdateState::EmitterMesh &m : U.emitterMeshes) {
            const uint32_t recOffset = pm_to_bits(U.tab[U.ecdfSize + (size_t) EM_STRIDE * m.emitter + EM_REC]);
            if (!recOffset) continue;
            const detail::ShapeWords &sw = L.words[P.emitters[m.emitter].shape];
            for (uint32_t k = 0; k < m.nTris; ++k) {
                float *r = U.tab.data() + recOffset + (size_t) k * 4 * TRISHADE_FLOAT4S;
                r[3] = pm_from_bits(sw.front); r[7] = pm_from_bits(sw.back);
                r[15] = pm_from_bits((pm_to_bits(r[15]) & ~TS_MATERIAL_BITS) | sw.flags);
            }
        }
        sd.radiance = SceneDev::RadiancePlan();          /* phip_radiance_device resolved its vertex kernels from the material mask: again at its next call */
    }
    if (a.emitters) {
        memcpy(U.tab.data(), L.ecdf.data(), L.ecdf.size() * sizeof(float));
        for (size_t i = 0; i < L.emitters.size(); ++i) {
            float *r = U.tab.data() + U.ecdfSize + (size_t) EM_STRIDE * i;
            for (int k = 0; k < 3; ++k) r[EM_RADIANCE + k] = L.emitters[i].radiance[k];
            r[EM_WEIGHT] = L.emitters[i].sampling_weight;
        }
        D.emitterNormalization = L.emNorm;
    }
    if (newMaterials || a.emitters) sd.emitterTab.upload(U.tab.data(), U.tab.size());
    if (a.envmap) {
        sd.envTexels.swapWith(envTexels); sd.envCdfRows.swapWith(envCdfRows); sd.envCdfCols.swapWith(envCdfCols); sd.envRowWeights.swapWith(envRowWeights);
        D.env = E;
        sd.bind();
    }
    ev.record(0);
    if (newMaterials && U.nTriangles > 0) HIP_TRY(hipMemcpy(U.triClass.data(), U.rb.triClass.p, U.nTriangles, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipGetLastError());
    P.materials.swap(L.materials); P.emitters.swap(L.emitters); P.texDesc.swap(L.texDesc); P.texMax.swap(L.texMax);
    /* replicas on other devices are copies of what the scene was: dropped, ensureReplicas copies again before the next multi-device render */
    if (sc->devs.size() > 1) sc->devs.resize(1);
    HIP_TRY(hipSetDevice(sd.device));
    if (info) {
        info->kernel_ms = ev.sumPairs();
        info->material_mask_changed = maskChanged ? 1u : 0u;
        info->update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return PHIP_OK;
}

/*
 * host_update.h -- host side of phip_scene_update: new vertex positions, normals and camera on the scene as created.  The topology stays (indices, shapes,
 * materials, emitters, textures, film; node, record and leaf counts), so the device paths a render resolves do not change; what depends on the vertices or the
 * camera is recomputed -- O(triangles) and O(nodes) work by the kernels of k_update.h from the positions where they are, the small sequential rest (area CDFs, the
 * emitter table, the environment emitter's sphere, the camera) by the creation's own stages.  The closest hit does not depend on the structure (winsTie) and the
 * refitted boxes are conservative, so every entry point gives the bits it gives on a scene created from the new arrays.
 * Order: validate (the check kernel's three counters and the emitter meshes' areas are read BEFORE anything is written: on an error the scene is what it was),
 * then shading records, scene box, Wald records, the wide tree level by level from the deepest, the packed leaf table, then the host stages.
 * phip_scene_rebuild is the same call with one more step (rebuild = true; scenes on the 8-wide tree only): behind the scene box a new topology is built on the
 * device (host_rebuild.h), the Wald and refit passes run on IT, and everything the call writes goes to fresh buffers that are swapped in at the end -- the
 * depth of the new tree is known only then, and a refusal has to leave the scene unchanged.
 * Host code only; included by phip.hip alone, after host_boundary.h.  The caller holds the scene's render lock and has made the scene's device current.
 */
#pragma once
#include "host_boundary.h"
#include "host_rebuild.h"

/* the creation's side tables on the device, the scratch of the passes: made by a scene's first update */
static void updateDeviceTables(phip_scene *sc) {
    SceneUpdateState &U = sc->upd;
    if (U.onDevice) return;
    auto up = [](auto &buf, const auto &v) { if (v.empty()) buf.alloc(1); else buf.upload(v.data(), v.size()); };
    up(U.dIndices, U.indices); up(U.dWRecPrim, U.wRecPrim); up(U.dRecPrim, U.recPrim); up(U.dHadRecord, U.hadRecord); up(U.dLeafRefs, U.leafRefs);
    U.dCounters.alloc(4); U.dConsts.alloc(1);
    U.dNodeBox.alloc(6 * (size_t) sc->bvh.nWNodes); U.dSahTerm.alloc(sc->bvh.nWNodes);
    U.dPartials.alloc(6 * 256);
    U.onDevice = true;
}

static int updateScene(phip_scene *sc, const phip_update_desc &u, phip_update_info *info, bool rebuild = false) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::string who = rebuild ? "phip_scene_rebuild: " : "phip_scene_update: ";
    SceneUpdateState &U = sc->upd;
    SceneDev &sd = *sc->devs[0];
    DevScene &D = sd.dev;
    if (u.normals && !U.hasNormals) return setErr(PHIP_ERR_INVALID, who + "normals for a scene that was created without normals");
    const phip_camera cam = u.camera ? *u.camera : sc->descCopy.camera;
    for (int i = 0; i < 16; ++i) if (!std::isfinite(cam.to_world[i])) return setErr(PHIP_ERR_INVALID, who + "non-finite camera transform");
    HIP_TRY(hipDeviceSynchronize());          /* (a render on a caller's stream has been waited for by its call; this costs nothing then) */
    const bool newVertices = (u.positions || u.normals) && U.nTriangles > 0;
    UpdateArgs A; memset(&A, 0, sizeof(A));
    if (U.nTriangles > 0) {
        updateDeviceTables(sc);
        if (u.device_pointers) {
            if (!allOnSceneDevice(sd, { u.positions, u.normals }))
                return setErr(PHIP_ERR_INVALID, who + "device_pointers = 1, but positions / normals are not device memory of the scene's device");
            HIP_TRY(hipStreamSynchronize((hipStream_t) u.stream));           /* ordered after the caller's producer */
            A.positions = u.positions; A.normals = u.normals;
        } else {
            if (u.positions) { U.dPositions.upload(u.positions, 3 * (size_t) U.nVertices); A.positions = U.dPositions.p; }
            if (u.normals) { U.dNormals.upload(u.normals, 3 * (size_t) U.nVertices); A.normals = U.dNormals.p; }
        }
    }
    A.indices = U.dIndices.p; A.nVertices = U.nVertices; A.nTriangles = U.nTriangles; A.hadRecord = U.dHadRecord.p;
    A.triShade = sd.triShade.p; A.stride = sc->triShadeStride;
    A.wnodes = sd.wnodes.p; A.nodeStride = WIDE_NODE_STRIDE; A.wRecPrim = U.dWRecPrim.p; A.nodeBox = U.dNodeBox.p; A.sahTerm = U.dSahTerm.p;
    A.flatLeaves = sd.flatLeaves.p; A.leafRefs = U.dLeafRefs.p; A.nFlatLeaves = (uint32_t) U.leafRefs.size(); A.recPrim = U.dRecPrim.p;
    A.consts = U.dConsts.p; A.partials = U.dPartials.p; A.counters = U.dCounters.p;
    A.camPos[0] = cam.to_world[3]; A.camPos[1] = cam.to_world[7]; A.camPos[2] = cam.to_world[11];
    const UpdateKernels K = phipUpdateKernels();
    const unsigned triBlocks = (unsigned) ((U.nTriangles + UPD_BLOCK - 1) / UPD_BLOCK);
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
    struct Events { hipEvent_t *e[4]; ~Events() { for (hipEvent_t *p : e) if (*p) (void) hipEventDestroy(*p); } } events = { { &e0, &e1, &e2, &e3 } };
    for (hipEvent_t *p : events.e) HIP_TRY(hipEventCreate(p));

    /* ---- validate: nothing is written before the host has read the counters and the emitter meshes have an area ---- */
    uint32_t counters[4] = { 0, 0, 0, 0 };
    std::vector<std::vector<float>> cdfs(U.emitterMeshes.size()); std::vector<float> invArea(U.emitterMeshes.size(), 0.0f);
    HIP_TRY(hipEventRecord(e0, 0));
    if (newVertices) {
        HIP_TRY(hipMemsetAsync(U.dCounters.p, 0, 4 * sizeof(uint32_t), 0));
        const unsigned n = std::max(U.nVertices, U.nTriangles);
        hipLaunchKernelGGL(K.check, dim3((n + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, 0, A);
        HIP_TRY(hipEventRecord(e1, 0));
        HIP_TRY(hipMemcpy(counters, U.dCounters.p, sizeof(counters), hipMemcpyDeviceToHost));
        HIP_TRY(hipGetLastError());
        if (counters[0]) return setErr(PHIP_ERR_INVALID, who + std::to_string(counters[0]) + " vertices with a non-finite position or normal");
        if (counters[1] && !rebuild) return setErr(PHIP_ERR_UNSUPPORTED, who + std::to_string(counters[1]) + " triangles that were degenerate when the scene was created are not "
                                       "degenerate now: they have no Wald record, and a refit cannot give them one (create the scene again)");
    } else HIP_TRY(hipEventRecord(e1, 0));
    if (u.positions && U.nTriangles > 0 && !U.emitterMeshes.empty()) {
        const float *hostPos = u.positions;
        if (u.device_pointers) {          /* only the vertex ranges of the emitter meshes come back */
            U.hostPositions.resize(3 * (size_t) U.nVertices);
            for (const SceneUpdateState::EmitterMesh &m : U.emitterMeshes)
                if (m.endVertex > m.firstVertex) HIP_TRY(hipMemcpy(&U.hostPositions[3 * (size_t) m.firstVertex], u.positions + 3 * (size_t) m.firstVertex, 3 * (size_t) (m.endVertex - m.firstVertex) * sizeof(float), hipMemcpyDeviceToHost));
            hostPos = U.hostPositions.data();
        }
        try {
            for (size_t i = 0; i < U.emitterMeshes.size(); ++i) invArea[i] = areaCdfOf(hostPos, U.indices.data(), U.emitterMeshes[i].firstTri, U.emitterMeshes[i].nTris, cdfs[i]);
        } catch (const std::exception &e) { return setErr(PHIP_ERR_INVALID, who + e.what()); }
    }

    /* ---- mutate (a rebuild: into `fresh`, the scene's own buffers are read only until the commit below) ---- */
    HIP_TRY(hipEventRecord(e2, 0));
    RebuildFresh fresh;
    float4 *wtris = sd.wtris.p; const uint32_t *wRecPrim = U.dWRecPrim.p; uint32_t nWRecs = (uint32_t) U.wRecPrim.size();
    const std::vector<uint32_t> *levels = &U.wLevels;
    if (U.nTriangles > 0) {
        if (rebuild && newVertices) { fresh.triShade.cloneFrom(sd.triShade); A.triShade = fresh.triShade.p; }
        if (newVertices) hipLaunchKernelGGL(K.shade, dim3(triBlocks), dim3(UPD_BLOCK), 0, 0, A);
        const unsigned boxBlocks = std::min(256u, triBlocks);
        hipLaunchKernelGGL(K.box, dim3(boxBlocks), dim3(UPD_BLOCK), 0, 0, A);
        hipLaunchKernelGGL(K.boxFinal, dim3(1), dim3(UPD_BLOCK), 0, 0, A, boxBlocks);
        if (rebuild) {
            const int rc = rebuildTopology(sc, A, fresh);
            if (rc != PHIP_OK) return rc;
            wtris = fresh.wtris.p; wRecPrim = fresh.wRecPrim.p; nWRecs = fresh.nRecs; levels = &fresh.wLevels;
        }
        if (u.positions || rebuild) {
            if (nWRecs) hipLaunchKernelGGL(K.wald, dim3((nWRecs + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, 0, A, wtris, wRecPrim, nWRecs);
            if (!U.recPrim.empty()) hipLaunchKernelGGL(K.wald, dim3((unsigned) ((U.recPrim.size() + UPD_BLOCK - 1) / UPD_BLOCK)), dim3(UPD_BLOCK), 0, 0, A, sd.tris.p, (const uint32_t *) U.dRecPrim.p, (uint32_t) U.recPrim.size());
        }
        for (size_t l = levels->size(); l-- > 1; ) {          /* level l - 1 = nodes wLevels[l - 1] .. wLevels[l]: the deepest first */
            const uint32_t first = (*levels)[l - 1], count = (*levels)[l] - first;
            if (count) hipLaunchKernelGGL(K.refitLevel, dim3((count + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, 0, A, first, count);
        }
        if (A.nFlatLeaves) hipLaunchKernelGGL(K.leafTable, dim3(1), dim3(64), 0, 0, A);
    }
    HIP_TRY(hipEventRecord(e3, 0));
    HIP_TRY(hipGetLastError());
    HostBVH &bvh = sc->bvh;
    if (U.nTriangles > 0) {
        detail::RefitConsts C;
        HIP_TRY(hipMemcpy(&C, U.dConsts.p, sizeof(C), hipMemcpyDeviceToHost));
        std::vector<float> terms(rebuild ? fresh.nNodes : bvh.nWNodes);
        HIP_TRY(hipMemcpy(terms.data(), A.sahTerm, terms.size() * sizeof(float), hipMemcpyDeviceToHost));
        if (rebuild) rebuildCommit(sc, fresh, newVertices);          /* (nothing below fails but the runtime) */
        double cost = 0; for (float t : terms) cost += t;
        bvh.wSahCost = (float) (cost + 1.0);
        for (int a = 0; a < 3; ++a) {
            bvh.tightMin[a] = C.tightMin[a]; bvh.tightMax[a] = C.tightMax[a]; bvh.sceneMin[a] = C.sceneMin[a]; bvh.sceneMax[a] = C.sceneMax[a];
            D.sceneMin[a] = C.sceneMin[a]; D.sceneMax[a] = C.sceneMax[a];
        }
    }
    /* ---- the creation's host stages: the emitter meshes' CDFs, areas and records inside the emitter table; the environment sphere; the camera ---- */
    if (newVertices && !U.emitterMeshes.empty()) {
        std::vector<float4> recs;
        for (size_t i = 0; i < U.emitterMeshes.size(); ++i) {
            const SceneUpdateState::EmitterMesh &m = U.emitterMeshes[i];
            float *r = U.tab.data() + U.ecdfSize + (size_t) EM_STRIDE * m.emitter;
            if (u.positions) {
                memcpy(U.tab.data() + pm_to_bits(r[EM_CDF]), cdfs[i].data(), cdfs[i].size() * sizeof(float));
                r[EM_INV_AREA] = invArea[i];
            }
            const uint32_t recOffset = pm_to_bits(r[EM_REC]);
            if (!recOffset) continue;
            /* the first six float4s of each record, as packEmitterTable takes them from the shading records -- which the kernel above has just written */
            recs.resize((size_t) A.stride * m.nTris);
            HIP_TRY(hipMemcpy(recs.data(), sd.triShade.p + (size_t) A.stride * m.firstTri, recs.size() * sizeof(float4), hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < m.nTris; ++k) memcpy(U.tab.data() + recOffset + (size_t) k * 4 * TRISHADE_FLOAT4S, &recs[(size_t) A.stride * k], 4 * TRISHADE_FLOAT4S * sizeof(float));
        }
        sd.emitterTab.upload(U.tab.data(), U.tab.size());
    }
    sc->descCopy.camera = cam;
    if (D.envEmitter >= 0) environmentSphereOf(bvh.sceneMin, bvh.sceneMax, U.nTriangles, cam, D);
    setupCamera(cam, sc->descCopy.film, D.cam);
    if (newVertices && u.positions) U.nDegenerate = counters[2];
    if (rebuild) U.nDegenerate = 0;          /* the new tree has no record for a degenerate triangle, as a creation's */
    /* replicas on other devices are copies of what the scene was: dropped, ensureReplicas copies again before the next multi-device render */
    if (sc->devs.size() > 1) sc->devs.resize(1);
    HIP_TRY(hipSetDevice(sd.device));
    HIP_TRY(hipDeviceSynchronize());
    if (info) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, e0, e1)); HIP_TRY(hipEventElapsedTime(&b, e2, e3));
        info->kernel_ms = (double) a + (double) b;
        info->sah_cost = bvh.wSahCost; info->n_degenerate = U.nDegenerate;
        info->update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return PHIP_OK;
}

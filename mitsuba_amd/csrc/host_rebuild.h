/*
 * host_rebuild.h -- host side of phip_scene_rebuild's own part: a new topology of the 8-wide tree, built on the device (k_rebuild.h, rebuild_hd.h) into FRESH buffers,
 * from the shading records the update's triangle pass has just written.  updateScene (host_update.h) calls it between its scene-box pass and its Wald / refit passes,
 * which then run on these buffers, and swaps them in when everything has succeeded (commit) -- so that on any error the scene is what it was.
 * The host reads back scalars only: the number of triangles in the tree, one 8-byte total per level, the leaf slots.
 * Host code only; included by host_update.h.  The caller holds the scene's render lock.
 */
#pragma once
#include "rebuild_hd.h"

struct RebuildFresh {
    DevBuf<float4> triShade, wtris; DevBuf<uint4> wnodes; DevBuf<uint32_t> wRecPrim, hadRecord; DevBuf<float> nodeBox, sahTerm;
    std::vector<uint32_t> wLevels;
    uint32_t nNodes = 0, nRecs = 0, nLeafSlots = 0;
};

/* A: the update's arguments, triShade and consts valid on the device.  On success A points at the fresh tree (wnodes, wRecPrim, nodeBox, sahTerm).
   PHIP_ERR_UNSUPPORTED for a tree the traversal stacks do not hold */
static int rebuildTopology(phip_scene *sc, UpdateArgs &A, RebuildFresh &F) {
    SceneUpdateState &U = sc->upd;
    SceneUpdateState::RebuildScratch &S = U.rb;
    const uint32_t n = U.nTriangles;
    const RebuildKernels K = phipRebuildKernels();
    auto blocks = [](uint32_t items) { return dim3((items + UPD_BLOCK - 1) / UPD_BLOCK); };
    if (S.triClass.n != n) S.triClass.upload(U.triClass.data(), n);
    S.keys.alloc(n); S.tris.alloc(n); S.sortedKeys.alloc(n); S.sortedTris.alloc(n);
    F.hadRecord.alloc(((size_t) n + 31) / 32 + 1);
    HIP_TRY(hipMemsetAsync(F.hadRecord.p, 0, F.hadRecord.n * sizeof(uint32_t), 0));
    HIP_TRY(hipMemsetAsync(U.dCounters.p, 0, 4 * sizeof(uint32_t), 0));
    RebuildArgs R; memset(&R, 0, sizeof(R));
    R.triShade = A.triShade; R.stride = A.stride; R.nTriangles = n; R.consts = A.consts;
    R.keysOut = S.keys.p; R.trisOut = S.tris.p; R.hadRecord = F.hadRecord.p; R.counters = U.dCounters.p; R.triClass = S.triClass.p;

    /* ---- keys, sort ---- */
    hipLaunchKernelGGL(K.keys, blocks(n), dim3(UPD_BLOCK), 0, 0, R);
    size_t tempBytes = 0;
    HIP_TRY(phipRebuildSortPairs(nullptr, tempBytes, S.keys.p, S.sortedKeys.p, S.tris.p, S.sortedTris.p, n, 0));
    S.temp.alloc(std::max<size_t>(tempBytes, 16));
    HIP_TRY(phipRebuildSortPairs(S.temp.p, tempBytes, S.keys.p, S.sortedKeys.p, S.tris.p, S.sortedTris.p, n, 0));
    uint32_t counters[4];
    HIP_TRY(hipMemcpy(counters, U.dCounters.p, sizeof(counters), hipMemcpyDeviceToHost));
    HIP_TRY(hipGetLastError());
    const uint32_t m = counters[0];             /* the triangles waldLoad gives a record: the first m of the sorted order */
    if (m > n) throw std::runtime_error("phip_scene_rebuild: the key pass counted more triangles than the scene has");

    /* ---- the binary radix tree and its boxes ---- */
    const uint32_t maxNodes = std::max(m, 1u);
    S.child.alloc(2 * (size_t) maxNodes); S.range.alloc(2 * (size_t) maxNodes); S.parent.alloc(2 * (size_t) maxNodes); S.box.alloc(12 * (size_t) maxNodes); S.arrived.alloc(maxNodes);
    S.items.alloc(maxNodes); S.slotRef.alloc(8 * (size_t) maxNodes); S.scanIn.alloc((size_t) maxNodes + 1); S.scanOut.alloc((size_t) maxNodes + 1);
    R.tree.keys = S.sortedKeys.p; R.tree.tris = S.sortedTris.p; R.tree.nValid = m;
    R.tree.child = S.child.p; R.tree.range = S.range.p; R.tree.parent = S.parent.p; R.tree.box = S.box.p; R.tree.arrived = S.arrived.p;
    R.items = S.items.p; R.slotRef = S.slotRef.p; R.scanIn = S.scanIn.p; R.scanOut = S.scanOut.p;
    F.wnodes.alloc((size_t) WIDE_NODE_STRIDE * maxNodes); F.wRecPrim.alloc(maxNodes); F.wtris.alloc(3 * (size_t) maxNodes);
    F.nodeBox.alloc(6 * (size_t) maxNodes); F.sahTerm.alloc(maxNodes);
    R.wnodes = F.wnodes.p; R.nodeStride = WIDE_NODE_STRIDE; R.wRecPrim = F.wRecPrim.p; R.wtris = F.wtris.p;
    HIP_TRY(hipMemsetAsync(S.parent.p, 0xff, S.parent.n * sizeof(uint32_t), 0));
    HIP_TRY(hipMemsetAsync(S.arrived.p, 0, S.arrived.n * sizeof(uint32_t), 0));
    if (m > 1) hipLaunchKernelGGL(K.inner, blocks(m - 1), dim3(UPD_BLOCK), 0, 0, R);
    if (m > 0) hipLaunchKernelGGL(K.boxes, blocks(m), dim3(UPD_BLOCK), 0, 0, R);

    /* ---- the 8-wide tree, level by level from the root ---- */
    F.wLevels.assign(1, 0u);
    if (m == 0) {                                /* no triangle has a record: one node without children, as the creation makes it for a scene without triangles */
        HIP_TRY(hipMemsetAsync(F.wnodes.p, 0, (size_t) WIDE_NODE_STRIDE * sizeof(uint4), 0));
        F.nNodes = 1; F.nRecs = 0; F.wLevels.push_back(1u);
    } else {
        const int32_t root = m == 1 ? ~(int32_t) 0 : 0;
        HIP_TRY(hipMemcpyAsync(S.items.p, &root, sizeof(root), hipMemcpyHostToDevice, 0));
        uint32_t first = 0, count = 1, recBase = 0;
        while (count) {
            if (!wideDepthFits((uint32_t) F.wLevels.size()))
                return setErr(PHIP_ERR_UNSUPPORTED, "phip_scene_rebuild: the new tree is deeper than the traversal stacks allow (more than " + std::to_string(F.wLevels.size() - 1) +
                                                    " levels: millions of triangles in one cell of the 1024^3 key grid); the scene is unchanged");
            const uint32_t nextFirst = first + count;
            hipLaunchKernelGGL(K.collapse, blocks(count + 1), dim3(UPD_BLOCK), 0, 0, R, first, count);
            HIP_TRY(phipRebuildScan(nullptr, tempBytes, S.scanIn.p, S.scanOut.p, count + 1, 0));
            S.temp.alloc(std::max<size_t>(tempBytes, 16));
            HIP_TRY(phipRebuildScan(S.temp.p, tempBytes, S.scanIn.p, S.scanOut.p, count + 1, 0));
            unsigned long long total = 0;
            HIP_TRY(hipMemcpy(&total, S.scanOut.p + count, sizeof(total), hipMemcpyDeviceToHost));
            const uint32_t nInner = (uint32_t) total, nRecs = (uint32_t) (total >> 32);
            if ((size_t) nextFirst + nInner > maxNodes || (size_t) recBase + nRecs > m) throw std::runtime_error("phip_scene_rebuild: a level of the collapse does not fit the tree's bounds");
            hipLaunchKernelGGL(K.emit, blocks(count), dim3(UPD_BLOCK), 0, 0, R, first, count, nextFirst, recBase);
            F.wLevels.push_back(nextFirst);
            first = nextFirst; count = nInner; recBase += nRecs;
        }
        F.nNodes = first; F.nRecs = recBase;
        if (F.nRecs != m) throw std::runtime_error("phip_scene_rebuild: the collapse placed " + std::to_string(F.nRecs) + " of " + std::to_string(m) + " records");
        hipLaunchKernelGGL(K.shadeClass, blocks(F.nRecs), dim3(UPD_BLOCK), 0, 0, R, F.nRecs);
    }
    HIP_TRY(hipMemcpy(counters, U.dCounters.p, sizeof(counters), hipMemcpyDeviceToHost));
    HIP_TRY(hipGetLastError());
    F.nLeafSlots = counters[1];
    A.wnodes = F.wnodes.p; A.wRecPrim = F.wRecPrim.p; A.nodeBox = F.nodeBox.p; A.sahTerm = F.sahTerm.p; A.hadRecord = F.hadRecord.p;
    return PHIP_OK;
}

/* the fresh tree becomes the scene's: buffers, counts, and what the creation derives from the counts */
static void rebuildCommit(phip_scene *sc, RebuildFresh &F, bool newShading) {
    SceneUpdateState &U = sc->upd;
    SceneDev &sd = *sc->devs[0];
    HostBVH &bvh = sc->bvh;
    sd.wnodes.swapWith(F.wnodes); sd.wtris.swapWith(F.wtris);
    if (newShading) sd.triShade.swapWith(F.triShade);
    U.dWRecPrim.swapWith(F.wRecPrim); U.dHadRecord.swapWith(F.hadRecord); U.dNodeBox.swapWith(F.nodeBox); U.dSahTerm.swapWith(F.sahTerm);
    U.wLevels = F.wLevels; U.wRecPrim.resize(F.nRecs);
    bvh.nWNodes = F.nNodes; bvh.nWTris = F.nRecs; bvh.nTriRefs = F.nRecs; bvh.nLeaves = F.nLeafSlots; bvh.wMaxDepth = (uint32_t) F.wLevels.size() - 1u; bvh.wLevels = F.wLevels;
    sd.bind();
    wideTreePaths(sc, sd.dev);
}

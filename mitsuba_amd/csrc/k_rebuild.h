/*
 * k_rebuild.h -- the kernels of phip_scene_rebuild: a new topology of the 8-wide tree, built on the device from the triangles where they are.  As in k_update.h every
 * kernel is one lane per item around a __host__ __device__ body (rebuild_hd.h explains the steps), which the host twin of the test hook runs too.  In launch order
 * (host_rebuild.h):
 *   k_rb_keys      one lane per triangle: (Morton key, triangle), the bitmap of the triangles that are in the tree, their number
 *   (a stable radix sort of the pairs: rocPRIM, phip_rebuild.hip)
 *   k_rb_inner     one lane per inner node of the binary radix tree: range, split, children
 *   k_rb_boxes     one lane per leaf: its box, then up the tree.  Every inner node has one arrival flag; the child that arrives first is done, the one that arrives
 *                  second has both boxes -- its own in registers, its sibling's in memory, published by the sibling's agent-scope release (the acq_rel increment
 *                  of the flag) and read behind this lane's acquire (the same increment) -- and goes on.  Nobody waits for anybody: there is no loop that polls.
 *                  min / max are exact in any order, so the boxes do not depend on who arrives first
 *   k_rb_collapse  one lane per wide node of one level: its children by slot, how many inner children and records it has
 *   (an exclusive scan over the level: rocPRIM; the host reads the two totals -- one 8-byte word per level)
 *   k_rb_emit      one lane per wide node of that level: the node's topology words, the primitives of its records, the next level's work items
 *   k_rb_class     one lane per record: the shade class of its triangle in word 11, which the Wald pass of the refit (k_upd_wald) keeps
 * Every index is bounded by construction: the tree has nValid leaves and nValid - 1 inner nodes, a wide node below the root stands for a distinct inner node of more
 * than three triangles (fewer than nValid wide nodes), every leaf is in exactly one slot (nValid records).
 */
#pragma once
#include "rebuild_hd.h"

__global__ __launch_bounds__(UPD_BLOCK) void k_rb_keys(RebuildArgs A) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    uint32_t key = REBUILD_NO_KEY;
    if (i < A.nTriangles) {
        const pt::detail::RefitConsts K = *A.consts;
        key = pt::detail::rebuildKey(A.triShade, A.stride, i, K);
        A.keysOut[i] = key; A.trisOut[i] = i;
    }
    /* a wave is 64 consecutive triangles: two words of the bitmap (the grid covers whole words; the bitmap has a spare word) */
    const unsigned long long in = __ballot(key != REBUILD_NO_KEY);
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0u || lane == 32u) {
        if (i < A.nTriangles) A.hadRecord[i >> 5] = (uint32_t) (lane ? in >> 32 : in);
        if (lane == 0u && in) atomicAdd(&A.counters[0], (uint32_t) __popcll(in));
    }
}

__global__ __launch_bounds__(UPD_BLOCK) void k_rb_inner(RebuildArgs A) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (i + 1u >= A.tree.nValid) return;
    pt::detail::rebuildInnerNode(A.tree, i);
}

__global__ __launch_bounds__(UPD_BLOCK) void k_rb_boxes(RebuildArgs A) {
    const uint32_t p = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (p >= A.tree.nValid) return;
    float mn[3], mx[3];
    pt::detail::rebuildLeafBox(A.tree, A.triShade, A.stride, p, mn, mx);
    uint32_t cur = A.tree.nValid - 1u + p;
    for (;;) {          /* up the tree: at most its depth steps */
        const uint32_t par = A.tree.parent[cur];
        if (par == REBUILD_NO_NODE) break;
        const uint32_t before = __hip_atomic_fetch_add(&A.tree.arrived[par], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (!pt::detail::rebuildClimbStep(A.tree, cur, par, before, mn, mx)) break;
    }
}

__global__ __launch_bounds__(UPD_BLOCK) void k_rb_collapse(RebuildArgs A, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (i > count) return;
    if (i == count) { A.scanIn[i] = 0ull; return; }          /* the scan's last output is the level's total */
    uint32_t nInner, nRecs;
    pt::detail::rebuildCollapseNode(A.tree, A.items[first + i], A.slotRef + 8 * (size_t) (first + i), nInner, nRecs);
    A.scanIn[i] = (unsigned long long) nInner | ((unsigned long long) nRecs << 32);
}

__global__ __launch_bounds__(UPD_BLOCK) void k_rb_emit(RebuildArgs A, uint32_t first, uint32_t count, uint32_t nextFirst, uint32_t recBase) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (i >= count) return;
    const unsigned long long before = A.scanOut[i];
    const uint32_t leaves = pt::detail::rebuildEmitNode(A.tree, A.slotRef + 8 * (size_t) (first + i), nextFirst + (uint32_t) before, recBase + (uint32_t) (before >> 32),
                                                        A.wnodes + (size_t) A.nodeStride * (first + i), A.wRecPrim, A.items);
    if (leaves) atomicAdd(&A.counters[1], leaves);
}

__global__ __launch_bounds__(UPD_BLOCK) void k_rb_class(RebuildArgs A, uint32_t nRecs) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (i >= nRecs) return;
    A.wtris[3 * (size_t) i + 2].w = pt::detail::bits2f((uint32_t) A.triClass[A.wRecPrim[i]]);
}

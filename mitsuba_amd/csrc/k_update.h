/*
 * k_update.h -- the kernels of phip_scene_update: new vertex positions / normals / camera on a tree whose topology stays (a refit, not a rebuild).
 * Every kernel is one lane per item around a __host__ __device__ body of refit_hd.h -- the builder's own arithmetic, which the host builder calls too --, so what they
 * write are the bits a fresh build would write from the same boxes.  The work is bandwidth-trivial (about 40 MB for a 250 k-triangle scene): plain, coalesced where the
 * layout allows, no atomics on floats.  In launch order (host_update.h):
 *   k_upd_check        one lane per vertex and per triangle: non-finite values, "had no Wald record at creation, is non-degenerate now", records that become never-hit;
 *                      three integer counters the host reads BEFORE anything is written
 *   k_upd_shade        one lane per triangle: the shading record from the vertex arrays
 *   k_upd_box          the tight box: min / max are exact in any order -- wave shuffles, one LDS merge per block, one partial per block; k_upd_box_final merges the
 *                      partials in one block and leaves the RefitConsts (scene box, pad terms) in memory for the passes below
 *   k_upd_wald         one lane per Wald record (wtris, and the LDS-resident scenes' tris)
 *   k_upd_refit_level  one lane per node of one level of the 8-wide tree.  The nodes are in breadth-first order, so a level is a contiguous range whose children all
 *                      lie in the levels below: one launch per level, from the deepest up (a tree of 250 k triangles has about ten).  The alternative -- one
 *                      launch with per-parent arrival counters -- saves those few launches and pays for them with an inter-workgroup release / acquire protocol
 *                      and an order of execution that differs from run to run; nothing here is worth that.
 *   k_upd_leaf_table   the packed leaf table of a scene of at most 64 records: one small block
 */
#pragma once
#include "refit_hd.h"

/* (UpdateArgs, what every kernel here gets, and UPD_BLOCK: refit_hd.h) */

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_check(UpdateArgs A) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    bool bad = false, grown = false, lost = false;
    if (i < A.nVertices) {
        if (A.positions) for (int a = 0; a < 3; ++a) bad |= !isfinite(A.positions[3 * (size_t) i + a]);
        if (A.normals) for (int a = 0; a < 3; ++a) bad |= !isfinite(A.normals[3 * (size_t) i + a]);
    }
    if (i < A.nTriangles && A.positions) {
        const float *p0 = A.positions + 3 * (size_t) A.indices[3 * (size_t) i], *p1 = A.positions + 3 * (size_t) A.indices[3 * (size_t) i + 1],
                    *p2 = A.positions + 3 * (size_t) A.indices[3 * (size_t) i + 2];
        float rec[12];
        const bool ok = pt::detail::waldLoad(p0, p1, p2, i, rec);
        const bool had = (A.hadRecord[i >> 5] >> (i & 31u)) & 1u;
        grown = ok && !had; lost = !ok && had;
    }
    const unsigned long long b0 = __ballot(bad), b1 = __ballot(grown), b2 = __ballot(lost);
    if ((threadIdx.x & 63u) == 0u) {
        if (b0) atomicAdd(&A.counters[0], (uint32_t) __popcll(b0));
        if (b1) atomicAdd(&A.counters[1], (uint32_t) __popcll(b1));
        if (b2) atomicAdd(&A.counters[2], (uint32_t) __popcll(b2));
    }
}

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_shade(UpdateArgs A) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (i >= A.nTriangles) return;
    pt::detail::refitShadeRecord(A.positions, A.normals, A.indices, i, A.triShade + (size_t) A.stride * i);
}

/* min / max of six floats over the block; the result is valid in thread 0 */
__device__ inline void updBlockBox(float *mn, float *mx) {
    __shared__ float part[UPD_BLOCK / 64][6];
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) {
            mn[a] = pt::detail::hmin(mn[a], __shfl_xor(mn[a], off, 64));
            mx[a] = pt::detail::hmax(mx[a], __shfl_xor(mx[a], off, 64));
        }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) for (int a = 0; a < 3; ++a) { part[wave][a] = mn[a]; part[wave][3 + a] = mx[a]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < UPD_BLOCK / 64; ++w)
            for (int a = 0; a < 3; ++a) { mn[a] = pt::detail::hmin(mn[a], part[w][a]); mx[a] = pt::detail::hmax(mx[a], part[w][3 + a]); }
}

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_box(UpdateArgs A) {
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x; i < A.nTriangles; i += gridDim.x * UPD_BLOCK)
        pt::detail::growByTriangle(A.triShade, A.stride, i, mn, mx);
    updBlockBox(mn, mx);
    if (threadIdx.x == 0) for (int a = 0; a < 3; ++a) { A.partials[6 * blockIdx.x + a] = mn[a]; A.partials[6 * blockIdx.x + 3 + a] = mx[a]; }
}

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_box_final(UpdateArgs A, uint32_t nPartials) {
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t i = threadIdx.x; i < nPartials; i += UPD_BLOCK)
        for (int a = 0; a < 3; ++a) { mn[a] = pt::detail::hmin(mn[a], A.partials[6 * i + a]); mx[a] = pt::detail::hmax(mx[a], A.partials[6 * i + 3 + a]); }
    updBlockBox(mn, mx);
    if (threadIdx.x == 0) { pt::detail::RefitConsts K; pt::detail::refitConstsOf(mn, mx, A.camPos, K); *A.consts = K; }
}

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_wald(UpdateArgs A, float4 *recs, const uint32_t *recPrim, uint32_t nRecs) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (i >= nRecs) return;
    pt::detail::refitWaldRecord(A.triShade, A.stride, recPrim[i], recs + 3 * (size_t) i);
}

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_refit_level(UpdateArgs A, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (i >= count) return;
    const uint32_t idx = first + i;
    const pt::detail::RefitConsts K = *A.consts;
    A.sahTerm[idx] = pt::detail::refitWideNode(A.wnodes + (size_t) A.nodeStride * idx, idx, A.triShade, A.stride, A.wRecPrim, K, A.nodeBox);
}

__global__ __launch_bounds__(64) void k_upd_leaf_table(UpdateArgs A) {
    const uint32_t i = threadIdx.x;
    if (i >= A.nFlatLeaves) return;
    const pt::detail::RefitConsts K = *A.consts;
    pt::detail::refitLeafEntry(A.flatLeaves + 2 * (size_t) i, A.leafRefs[i], A.triShade, A.stride, A.recPrim, K);
}

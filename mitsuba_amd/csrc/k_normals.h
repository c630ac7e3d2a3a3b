/*
 * k_normals.h -- the kernel of phip_vertex_normals_device: the angle-weighted vertex normals of the reference's TriMesh::computeNormals from positions in device
 * memory.  The arithmetic is normals_hd.h's, which the host call phip_vertex_normals runs too; the kernel only says which lane computes which vertex.
 *   k_vertex_normals   one lane per vertex, a gather: the lane walks its vertex's incidence list (offsets[v] .. offsets[v + 1] of `entries`, each entry 3 * triangle +
 *                      corner = the place of the corner in the index array, in ascending order -- the reference's order of summation), loads the triangle's three
 *                      indices and positions, makes the face normal and its own corner's angle, adds, normalises, writes three floats.  No float atomics.
 *                      Invalid vertices (a zero sum: (1, 0, 0)) are counted per wave and added with one integer atomic per wave that has any.
 * A corner's angle -- the expensive part, two reciprocal square roots and a double-precision arcsine -- is computed once, by the vertex that owns it; the face normal
 * is made again at each of its three corners.  A wave takes as long as its vertex of highest valence.
 * The 12-byte vectors are tight: scalar 4-byte loads and stores, as k_pyramid_pass has them.
 */
#pragma once
#include "normals_hd.h"

__global__ __launch_bounds__(NRM_BLOCK) void k_vertex_normals(const uint32_t *offsets, const uint32_t *entries, const uint32_t *indices, const float *positions,
                                                              uint32_t nVertices, float *normals, unsigned int *nInvalid) {
    using namespace pt::detail;
    const uint32_t v = blockIdx.x * NRM_BLOCK + threadIdx.x;
    bool invalid = false;
    if (v < nVertices) {
        N3 sum; sum.x = 0.0f; sum.y = 0.0f; sum.z = 0.0f;
        const uint32_t end = offsets[v + 1];
        for (uint32_t k = offsets[v]; k < end; ++k) {
            const uint32_t e = entries[k], t = e / 3u, corner = e - 3u * t;
            const N3 p0 = normalsLoad(positions, indices[3 * (size_t) t]), p1 = normalsLoad(positions, indices[3 * (size_t) t + 1]), p2 = normalsLoad(positions, indices[3 * (size_t) t + 2]);
            N3 n;
            if (!normalsFace(p0, p1, p2, n)) continue;
            /* the corner's own vertex first, then the triangle's next two in its order */
            const N3 a = corner == 0u ? p0 : corner == 1u ? p1 : p2, b = corner == 0u ? p1 : corner == 1u ? p2 : p0, c = corner == 0u ? p2 : corner == 1u ? p0 : p1;
            sum = normalsAdd(sum, normalsCorner(n, a, b, c));
        }
        invalid = !normalsFinish(sum);
        normals[3 * (size_t) v] = sum.x; normals[3 * (size_t) v + 1] = sum.y; normals[3 * (size_t) v + 2] = sum.z;
    }
    const unsigned long long m = __ballot(invalid);
    if (__lane_id() == 0 && m != 0ull) atomicAdd(nInvalid, (unsigned int) __popcll(m));
}

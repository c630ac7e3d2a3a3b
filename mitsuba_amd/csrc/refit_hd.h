/*
 * refit_hd.h -- the arithmetic the host builder (bvh.h, host_scene.h) and the refit kernels of phip_scene_update (k_update.h) share, stated once as
 * __host__ __device__ functions: the Wald record of a triangle, the pad of a box, the scene box, the origin / exponent / quantisation of a wide node, the centre /
 * half extent of a packed leaf and the geometry of a shading record.  One statement, two callers: a refitted tree is made of the bits a fresh build would make
 * from the same boxes.  Everything is compiled with -ffp-contract=off; the quantisation is in double on both sides (frexp / ldexp / floor / ceil are exact).
 * std::min / std::max are spelled out (hmin / hmax: the same comparisons) because the device has no <algorithm>.
 */
#pragma once
#include <cstdint>
#include <cstring>
#include <cmath>
#include "dv_scene.h"

namespace pt {
namespace detail {

#define RHD __host__ __device__ inline

RHD float hmin(float a, float b) { return (b < a) ? b : a; }            /* std::min */
RHD float hmax(float a, float b) { return (a < b) ? b : a; }            /* std::max */
RHD double hmind(double a, double b) { return (b < a) ? b : a; }
RHD double hmaxd(double a, double b) { return (a < b) ? b : a; }
RHD float bits2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* TriAccel::load, triaccel.h:61-93 -- returns false for degenerate triangles (k = 3) */
RHD bool waldLoad(const float *A, const float *B, const float *C, uint32_t prim, float *out12) {
    float b[3] = { C[0] - A[0], C[1] - A[1], C[2] - A[2] };
    float c[3] = { B[0] - A[0], B[1] - A[1], B[2] - A[2] };
    float N[3] = { c[1] * b[2] - c[2] * b[1], c[2] * b[0] - c[0] * b[2], c[0] * b[1] - c[1] * b[0] };
    uint32_t k = 0;
    for (int j = 0; j < 3; j++)
        if (fabsf(N[j]) > fabsf(N[k])) k = j;
    const uint32_t u = (k + 1u) % 3u, v = (k + 2u) % 3u;               /* waldModulo[k], waldModulo[k + 1] */
    const float n_k = N[k], denom = b[u] * c[v] - b[v] * c[u];
    if (denom == 0) return false;
    out12[0] = bits2f(k);
    out12[1] = N[u] / n_k;
    out12[2] = N[v] / n_k;
    out12[3] = (A[0] * N[0] + A[1] * N[1] + A[2] * N[2]) / n_k;
    out12[4] = A[u];
    out12[5] = A[v];
    out12[6] = b[u] / denom;
    out12[7] = -b[v] / denom;
    out12[8] = c[v] / denom;
    out12[9] = -c[u] / denom;
    out12[10] = bits2f(prim);
    out12[11] = 0.0f;
    return true;
}
/* the never-hit record (k = 3, no primitive): a leaf whose triangles are all degenerate keeps one, and so does a record whose triangle an update collapsed */
RHD void waldNeverHit(float *out12) {
    for (int i = 0; i < 12; ++i) out12[i] = 0.0f;
    out12[0] = bits2f(3u); out12[10] = bits2f(0xFFFFFFFFu);
}

/* Builder::pad, per axis: what a box [mn, mx] is widened by on either side (bvh.h explains the four terms) */
RHD float padOf(float mn, float mx, float maxExtent, float camPad) {
    return 1e-5f * hmax(fabsf(mn), fabsf(mx)) + 1e-7f * (mx - mn) + 2e-6f * maxExtent + camPad + 1e-30f;
}
/* the camera's term of the pad: 4.8e-7 x its largest coordinate, on every axis (bvh.h: buildBVH) */
RHD float camPadOf(const float *cameraPosition) {
    const float m = hmax(fabsf(cameraPosition[0]), hmax(fabsf(cameraPosition[1]), fabsf(cameraPosition[2])));
    return 4.8e-7f * m;
}
/* scene box: the tight box enlarged exactly like the reference's kd-tree root (gkdtree.h:1213-1220): min -= (max-min)*eps + eps; max += (max-min_new)*eps + eps */
RHD void sceneBoxOf(const float *tightMn, const float *tightMx, float *sceneMn, float *sceneMx) {
    const float eps = 1e-3f;
    for (int a = 0; a < 3; ++a) {
        float mn = tightMn[a], mx = tightMx[a];
        mn -= (mx - mn) * eps + eps;
        mx += (mx - mn) * eps + eps;
        sceneMn[a] = mn; sceneMx[a] = mx;
    }
}
RHD float boxArea(const float *mn, const float *mx) {
    float d[3] = { mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2] };
    if (d[0] < 0 || d[1] < 0 || d[2] < 0) return 0.0f;
    return 2.0f * (d[0] * d[1] + d[1] * d[2] + d[0] * d[2]);
}

/* a wide node's grid (buildWide): origin p = the node box's lower corner, per axis the power-of-two step 2^e >= extent / 255 as a biased exponent byte */
struct WideGrid { float p[3]; uint32_t e8[3]; double step[3]; };
RHD void wideGridOf(const float *nbMn, const float *nbMx, WideGrid &g) {
    for (int a = 0; a < 3; ++a) {
        g.p[a] = nbMn[a];
        const double ext = (double) nbMx[a] - (double) g.p[a];
        int e = -120;
        if (ext > 0) { int ex; (void) frexp(ext / 255.0, &ex); e = ex; }            /* 2^e >= ext / 255 */
        while (ldexp(1.0, e) * 255.0 < ext) ++e;
        e = e > 127 ? 127 : (e < -120 ? -120 : e);
        g.e8[a] = (uint32_t) (e + 127); g.step[a] = ldexp(1.0, e);
    }
}
/* a child box on that grid, rounded outwards */
RHD void wideQuantise(const WideGrid &g, const float *mn, const float *mx, uint8_t *qlo3, uint8_t *qhi3) {
    for (int a = 0; a < 3; ++a) {
        const double lo = floor(((double) mn[a] - (double) g.p[a]) / g.step[a]);
        const double hi = ceil(((double) mx[a] - (double) g.p[a]) / g.step[a]);
        qlo3[a] = (uint8_t) hmind(255.0, hmaxd(0.0, lo));
        qhi3[a] = (uint8_t) hmind(255.0, hmaxd(0.0, hi));
    }
}

/* the slots of a wide node's n <= 8 children (buildWide explains the layout): a child goes to the slot whose octant direction ((s & 1 ? + : -), (s & 2 ? + : -),
   (s & 4 ? + : -)) best matches its offset from the node's centre -- greedy on the dot product: of all (child, free slot) pairs the best one, n times; the first
   pair wins a tie.  The host builder and the collapse of phip_scene_rebuild (rebuild_hd.h) both call it */
RHD void wideAssignSlots(const float (*cmn)[3], const float (*cmx)[3], int n, const float *nbMn, const float *nbMx, int *slotOf) {
    const float cen[3] = { 0.5f * (nbMn[0] + nbMx[0]), 0.5f * (nbMn[1] + nbMx[1]), 0.5f * (nbMn[2] + nbMx[2]) };
    bool slotUsed[8] = { false, false, false, false, false, false, false, false }, childDone[8] = { false, false, false, false, false, false, false, false };
    for (int k = 0; k < n; ++k) {
        float bestV = -INFINITY; int bc = -1, bs = -1;
        for (int c = 0; c < n; ++c) {
            if (childDone[c]) continue;
            const float d[3] = { 0.5f * (cmn[c][0] + cmx[c][0]) - cen[0], 0.5f * (cmn[c][1] + cmx[c][1]) - cen[1], 0.5f * (cmn[c][2] + cmx[c][2]) - cen[2] };
            for (int sl = 0; sl < 8; ++sl) {
                if (slotUsed[sl]) continue;
                const float v = ((sl & 1) ? d[0] : -d[0]) + ((sl & 2) ? d[1] : -d[1]) + ((sl & 4) ? d[2] : -d[2]);
                if (v > bestV) { bestV = v; bc = c; bs = sl; }
            }
        }
        childDone[bc] = true; slotUsed[bs] = true; slotOf[bc] = bs;
    }
}

/* centre / half extent of a packed leaf (host_scene.h: packLeafTable explains the terms): `ext` = the largest extent of the tight box, `camMax` = the camera's largest coordinate */
RHD void leafCentreHalf(const float *lo, const float *hi, float ext, float camMax, float *c, float *h) {
    for (int a = 0; a < 3; ++a) {
        c[a] = (float) (0.5 * ((double) lo[a] + (double) hi[a]));
        const double need = hmaxd((double) c[a] - (double) lo[a], (double) hi[a] - (double) c[a]);
        h[a] = nextafterf((float) need, INFINITY) + 2.4e-7f * fabsf(c[a]) + 4e-6f * ext + 4.8e-7f * camMax;
    }
}

/* the geometry of a shading record (dv_scene.h): dpdu / dpdv (the triangle's sides, or TriMesh::computeUVTangents, trimesh.cpp:683-735, with zero tangents for
   degenerate triangles) and the three vectors of r3..r5: the vertex normals, or the flat shading frame (n, s, t) */
RHD void triShadeGeometry(const V3 &p0, const V3 &p1, const V3 &p2, bool texcoords, const V2 &t0, const V2 &t1, const V2 &t2,
                          bool hasNormals, const V3 &n0, const V3 &n1, const V3 &n2, V3 &dpdu, V3 &dpdv, V3 &a, V3 &b, V3 &c) {
    const V3 side1(p1 - p0), side2(p2 - p0);
    dpdu = side1; dpdv = side2;                      /* skdtree.h:378-379 */
    if (texcoords) {
        dpdu = V3(0.0f); dpdv = V3(0.0f);
        const V2 dUV1(t1.x - t0.x, t1.y - t0.y), dUV2(t2.x - t0.x, t2.y - t0.y);
        const V3 n = cross(side1, side2);
        const float length = n.length();
        if (length != 0) {
            const float determinant = dUV1.x * dUV2.y - dUV1.y * dUV2.x;
            if (determinant == 0) {
                coordinateSystem(n / length, dpdu, dpdv);
            } else {
                const float invDet = 1.0f / determinant;
                dpdu = (side1 * dUV2.y - side2 * dUV1.y) * invDet;
                dpdv = (side1 * (-dUV2.x) + side2 * dUV1.x) * invDet;
            }
        }
    }
    if (hasNormals) { a = n0; b = n1; c = n2; }
    else {
        Frame f; triShadingFrame(triFaceNormal(side1, side2), dpdu, f);
        a = f.n; b = f.s; c = f.t;
    }
}

/* ---- the refit of phip_scene_update, item by item: what one lane of a kernel of k_update.h does, and what the host twin of the test hook loops over ----
 * The topology is the creation's: records keep their places, nodes their slots.  Vertices are read from the shading records (r0..r2.xyz), which the triangle
 * pass has rewritten first; `recPrim` is the primitive of every Wald record as the creation fixed it (0xFFFFFFFF: a leaf's never-hit placeholder). */

/* what the scene box pass leaves for the passes after it (device memory; the host reads it back for the DevScene's constants) */
struct RefitConsts {
    float tightMin[3], tightMax[3], sceneMin[3], sceneMax[3];
    float maxExtent;        /* Builder::extent's largest component */
    float camPad, camMax;   /* 4.8e-7 x camMax; the camera's largest coordinate */
    float rootArea;         /* area of the tight box (1 if it has none): the SAH cost is relative to it */
};
RHD void refitConstsOf(const float *tightMn, const float *tightMx, const float *cameraPosition, RefitConsts &K) {
    float ext[3];
    for (int a = 0; a < 3; ++a) { K.tightMin[a] = tightMn[a]; K.tightMax[a] = tightMx[a]; ext[a] = tightMx[a] - tightMn[a]; }
    sceneBoxOf(tightMn, tightMx, K.sceneMin, K.sceneMax);
    K.maxExtent = hmax(ext[0], hmax(ext[1], ext[2]));
    K.camMax = hmax(fabsf(cameraPosition[0]), hmax(fabsf(cameraPosition[1]), fabsf(cameraPosition[2])));
    K.camPad = camPadOf(cameraPosition);
    const float area = boxArea(tightMn, tightMx);
    K.rootArea = area > 0 ? area : 1.0f;
}

RHD void growByTriangle(const float4 *triShade, uint32_t stride, uint32_t prim, float *mn, float *mx) {
    const float4 *r = triShade + (size_t) stride * prim;
    for (int k = 0; k < 3; ++k) {
        const float4 v = r[k];
        mn[0] = hmin(mn[0], v.x); mn[1] = hmin(mn[1], v.y); mn[2] = hmin(mn[2], v.z);
        mx[0] = hmax(mx[0], v.x); mx[1] = hmax(mx[1], v.y); mx[2] = hmax(mx[2], v.z);
    }
}
/* union of the full bounds of the triangles of records first .. first + count, padded (Builder::pad); an empty box (placeholders only) stays empty */
RHD void refitLeafBox(const float4 *triShade, uint32_t stride, const uint32_t *recPrim, uint32_t first, uint32_t count, const RefitConsts &K, float *mn, float *mx) {
    for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t prim = recPrim[first + k];
        if (prim != 0xFFFFFFFFu) growByTriangle(triShade, stride, prim, mn, mx);
    }
    for (int a = 0; a < 3; ++a) {
        if (!(mn[a] <= mx[a])) continue;
        const float e = padOf(mn[a], mx[a], K.maxExtent, K.camPad);
        mn[a] -= e; mx[a] += e;
    }
}

/* one Wald record: the twelve words of waldLoad on the triangle's vertices of now, or the never-hit record; word 11 (the shade class) stays */
RHD void refitWaldRecord(const float4 *triShade, uint32_t stride, uint32_t prim, float4 *rec3) {
    if (prim == 0xFFFFFFFFu) return;
    const float4 *r = triShade + (size_t) stride * prim;
    const float4 a = r[0], b = r[1], c = r[2];
    const float A[3] = { a.x, a.y, a.z }, B[3] = { b.x, b.y, b.z }, C[3] = { c.x, c.y, c.z };
    float w[12];
    if (!waldLoad(A, B, C, prim, w)) waldNeverHit(w);
    const float cls = rec3[2].w;
    rec3[0] = make_float4(w[0], w[1], w[2], w[3]); rec3[1] = make_float4(w[4], w[5], w[6], w[7]); rec3[2] = make_float4(w[8], w[9], w[10], cls);
}

/* one shading record from the vertex arrays: p0..p2, the frame or the vertex normals, dpdu / dpdv from the record's own UVs; every .w word (materials, emitter, flags) stays.
   positions == NULL / normals == NULL: the vertices / the vertex normals of the record stay */
RHD void refitShadeRecord(const float *positions, const float *normals, const uint32_t *indices, uint32_t tri, float4 *r) {
    const uint32_t i0 = indices[3 * (size_t) tri], i1 = indices[3 * (size_t) tri + 1], i2 = indices[3 * (size_t) tri + 2];
    V3 p0 = xyz(r[0]), p1 = xyz(r[1]), p2 = xyz(r[2]);          /* (positions == NULL: the vertices stay) */
    if (positions) {
        p0 = V3(positions[3 * (size_t) i0], positions[3 * (size_t) i0 + 1], positions[3 * (size_t) i0 + 2]);
        p1 = V3(positions[3 * (size_t) i1], positions[3 * (size_t) i1 + 1], positions[3 * (size_t) i1 + 2]);
        p2 = V3(positions[3 * (size_t) i2], positions[3 * (size_t) i2 + 1], positions[3 * (size_t) i2 + 2]);
    }
    const float4 r3 = r[3];
    const uint32_t flags = pm_to_bits(r3.w);
    const bool texcoords = (flags & TS_TEXCOORDS) != 0, hasNormals = (flags & TS_VERTEX_NORMALS) != 0;
    V2 t0(0, 0), t1(0, 0), t2(0, 0);
    if (texcoords) { const float4 r6 = r[6], r7 = r[7]; t0 = V2(r6.x, r6.y); t1 = V2(r6.z, r6.w); t2 = V2(r7.x, r7.y); }
    V3 n0 = xyz(r3), n1 = xyz(r[4]), n2 = xyz(r[5]);
    if (hasNormals && normals) {
        n0 = V3(normals[3 * (size_t) i0], normals[3 * (size_t) i0 + 1], normals[3 * (size_t) i0 + 2]);
        n1 = V3(normals[3 * (size_t) i1], normals[3 * (size_t) i1 + 1], normals[3 * (size_t) i1 + 2]);
        n2 = V3(normals[3 * (size_t) i2], normals[3 * (size_t) i2 + 1], normals[3 * (size_t) i2 + 2]);
    }
    V3 dpdu, dpdv, a, b, c;
    triShadeGeometry(p0, p1, p2, texcoords, t0, t1, t2, hasNormals, n0, n1, n2, dpdu, dpdv, a, b, c);
    r[0] = make_float4(p0.x, p0.y, p0.z, r[0].w); r[1] = make_float4(p1.x, p1.y, p1.z, r[1].w); r[2] = make_float4(p2.x, p2.y, p2.z, r[2].w);
    r[3] = make_float4(a.x, a.y, a.z, r3.w); r[4] = make_float4(b.x, b.y, b.z, r[4].w); r[5] = make_float4(c.x, c.y, c.z, r[5].w);
    if (texcoords) { r[7] = make_float4(t2.x, t2.y, dpdu.x, dpdu.y); r[8] = make_float4(dpdu.z, dpdv.x, dpdv.y, dpdv.z); }
}

/* one node of the compressed 8-wide tree (bvh.h: buildWide gives the layout): the boxes of its slots -- a leaf slot's from its records' triangles, an inner slot's
   = its child's node box, which the level below has left in nodeBox --, then p, e8 and qlo / qhi as buildWide computes them.  Slots, imask, meta, childBase and triBase
   stay.  Leaves the node's own box in nodeBox[6 idx ..] and returns its term of the SAH cost */
RHD float refitWideNode(uint4 *nd, uint32_t idx, const float4 *triShade, uint32_t stride, const uint32_t *wRecPrim, const RefitConsts &K, float *nodeBox) {
    const uint4 g0 = nd[0], g1 = nd[1];
    const uint32_t imask = g0.w >> 24, childBase = g1.x, triBase = g1.y;
    float cmn[8][3], cmx[8][3]; uint32_t mult[8];
    float nmn[3] = { INFINITY, INFINITY, INFINITY }, nmx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t s = 0; s < 8u; ++s) {
        const uint32_t meta = ((s < 4u ? g1.z : g1.w) >> (8u * (s & 3u))) & 0xffu;
        mult[s] = 0u;
        for (int a = 0; a < 3; ++a) { cmn[s][a] = INFINITY; cmx[s][a] = -INFINITY; }
        if (meta == 0u) continue;
        if (imask & (1u << s)) {
            const uint32_t child = childBase + (uint32_t) __builtin_popcount(imask & ((1u << s) - 1u));
            for (int a = 0; a < 3; ++a) { cmn[s][a] = nodeBox[6 * (size_t) child + a]; cmx[s][a] = nodeBox[6 * (size_t) child + 3 + a]; }
            mult[s] = 1u;
        } else {
            const uint32_t count = (uint32_t) __builtin_popcount(meta >> 5), off = meta & 31u;
            refitLeafBox(triShade, stride, wRecPrim, triBase + off, count, K, cmn[s], cmx[s]);
            mult[s] = count;
        }
        for (int a = 0; a < 3; ++a) { nmn[a] = hmin(nmn[a], cmn[s][a]); nmx[a] = hmax(nmx[a], cmx[s][a]); }
    }
    for (int a = 0; a < 3; ++a) if (!(nmn[a] <= nmx[a])) { nmn[a] = 0.0f; nmx[a] = 0.0f; }        /* (placeholders only: a point, so that p stays finite) */
    WideGrid grid; wideGridOf(nmn, nmx, grid);
    uint32_t q[6][2] = { { 0u, 0u }, { 0u, 0u }, { 0u, 0u }, { 0u, 0u }, { 0u, 0u }, { 0u, 0u } };
    double cost = 0;
    for (uint32_t s = 0; s < 8u; ++s) {
        uint8_t qlo[3] = { 255, 255, 255 }, qhi[3] = { 0, 0, 0 };
        if (mult[s]) {
            wideQuantise(grid, cmn[s], cmx[s], qlo, qhi);
            cost += (double) boxArea(cmn[s], cmx[s]) / (double) K.rootArea * (double) mult[s];
        }
        for (int a = 0; a < 3; ++a) { q[a][s >> 2] |= (uint32_t) qlo[a] << (8u * (s & 3u)); q[3 + a][s >> 2] |= (uint32_t) qhi[a] << (8u * (s & 3u)); }
    }
    uint4 o0; o0.x = pm_to_bits(grid.p[0]); o0.y = pm_to_bits(grid.p[1]); o0.z = pm_to_bits(grid.p[2]);
    o0.w = grid.e8[0] | (grid.e8[1] << 8) | (grid.e8[2] << 16) | (imask << 24);
    nd[0] = o0;
    nd[2] = make_uint4(q[0][0], q[0][1], q[1][0], q[1][1]);
    nd[3] = make_uint4(q[2][0], q[2][1], q[3][0], q[3][1]);
    nd[4] = make_uint4(q[4][0], q[4][1], q[5][0], q[5][1]);
    for (int a = 0; a < 3; ++a) { nodeBox[6 * (size_t) idx + a] = nmn[a]; nodeBox[6 * (size_t) idx + 3 + a] = nmx[a]; }
    return (float) cost;
}

/* one entry of the packed leaf table (host_scene.h: packLeafTable): centre and half extent from the leaf's records' triangles; the record masks in the .w words stay */
RHD void refitLeafEntry(float4 *entry2, int32_t ref, const float4 *triShade, uint32_t stride, const uint32_t *recPrim, const RefitConsts &K) {
    const uint32_t r = ~(uint32_t) ref, first = r >> 3, count = (r & 7u) + 1u;
    float mn[3], mx[3];
    refitLeafBox(triShade, stride, recPrim, first, count, K, mn, mx);
    for (int a = 0; a < 3; ++a) if (!(mn[a] <= mx[a])) { mn[a] = K.tightMin[a]; mx[a] = K.tightMin[a]; }     /* (placeholders only: any point will do, nothing in it can be hit) */
    float c[3], h[3];
    leafCentreHalf(mn, mx, K.maxExtent, K.camMax, c, h);
    entry2[0] = make_float4(c[0], c[1], c[2], entry2[0].w);
    entry2[1] = make_float4(h[0], h[1], h[2], entry2[1].w);
}

#undef RHD

} // namespace detail
} // namespace pt

/* what every kernel of k_update.h gets (filled by host_update.h), and their block size */
#define UPD_BLOCK 256
struct UpdateArgs {
    const float *positions, *normals;       /* 3 x nVertices each, device memory; either may be NULL (unchanged) */
    const uint32_t *indices;                /* 3 x nTriangles */
    uint32_t nVertices, nTriangles;
    const uint32_t *hadRecord;              /* one bit per triangle: it got a Wald record at creation */
    float4 *triShade; uint32_t stride;
    uint4 *wnodes; uint32_t nodeStride;     /* uint4s per node in memory */
    const uint32_t *wRecPrim;               /* primitive of every record of wtris, fixed at creation */
    float *nodeBox, *sahTerm;               /* 6 / 1 floats per wide node */
    float4 *flatLeaves; const int32_t *leafRefs; uint32_t nFlatLeaves; const uint32_t *recPrim;       /* the packed leaf table, its leaves' references, the primitives of tris */
    pt::detail::RefitConsts *consts;
    float *partials;                        /* 6 floats per block of k_upd_box */
    uint32_t *counters;                     /* k_upd_check: non-finite values, triangles that would need a new record, records that become never-hit */
    float camPos[3];
};

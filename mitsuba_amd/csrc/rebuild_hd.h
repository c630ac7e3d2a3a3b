/*
 * rebuild_hd.h -- phip_scene_rebuild item by item: what one lane of a kernel of k_rebuild.h does, and what the host twin of the test hook
 * (phip_debug_host_rebuild_trace_wide) loops over.  A new topology of the 8-wide tree from the triangles where they are, in four steps:
 *   keys       a 30-bit Morton code (10 bits per axis) of the centre of the triangle's bounds inside the tight box; a triangle waldLoad gives no record has the key
 *              0xFFFFFFFF: it sorts behind every code and is left out of the tree.  The pairs are sorted by a stable radix sort, so equal codes are in triangle order
 *   hierarchy  the binary radix tree over the sorted codes (Karras, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", HPG 2012): inner
 *              node i finds its range and its split by itself; equal codes are told apart by their place in the sorted order, so a run of m equal codes is a
 *              balanced subtree of depth ceil(log2 m).  Then the subtree boxes, bottom-up from the leaves (rebuildClimb: one arrival flag per inner node)
 *   collapse   level by level from the root: a wide node starts with the two children of its binary node and opens the inner node of the largest area among
 *              its children until eight slots are used or only leaves are left; then a binary subtree of at most three triangles is one leaf slot, whose
 *              records are its range of the sorted order, and a larger one is an inner child.  Slots by octant direction (wideAssignSlots, the host builder's rule); the leaf slots'
 *              records follow each other in slot order, so an offset is at most 21 (< 24)
 *   emit       behind an exclusive scan over the level (inner children, records): imask, meta, childBase, triBase, the primitive of every record, the next
 *              level's work items.  The nodes come out in breadth-first order with children childBase + rank
 * Boxes and records are not written here: the refit of phip_scene_update (refit_hd.h) runs on the new topology and fills in every padded box and Wald record.
 * Depth: a path of the binary tree has at most 30 + ceil(log2 m) inner nodes (m = the most triangles in one Morton cell), and every wide node on a path absorbs at
 * least one of them, so the wide tree has at most 31 + ceil(log2 m) levels; the traversal stacks hold 52.
 */
#pragma once
#include "refit_hd.h"

namespace pt {
namespace detail {

#define RHD __host__ __device__ inline

#define REBUILD_NO_KEY 0xFFFFFFFFu
#define REBUILD_NO_NODE 0xFFFFFFFFu
#define REBUILD_EMPTY_SLOT ((int32_t) 0x80000000u)      /* (a leaf reference ~place with place = 2^31 - 1: there are fewer than 2^30 triangles) */
#define REBUILD_LEAF_MAX 3u                              /* records of a leaf slot */

RHD uint32_t mortonSpread10(uint32_t v) {               /* 10 bits -> every third bit */
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu; v = (v | (v << 8)) & 0x0300f00fu; v = (v | (v << 4)) & 0x030c30c3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}
/* key of triangle `tri`: vertices from its shading record */
RHD uint32_t rebuildKey(const float4 *triShade, uint32_t stride, uint32_t tri, const RefitConsts &K) {
    const float4 *r = triShade + (size_t) stride * tri;
    const float4 a = r[0], b = r[1], c = r[2];
    const float A[3] = { a.x, a.y, a.z }, B[3] = { b.x, b.y, b.z }, C[3] = { c.x, c.y, c.z };
    float w[12];
    if (!waldLoad(A, B, C, tri, w)) return REBUILD_NO_KEY;
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = hmin(A[k], hmin(B[k], C[k])), hi = hmax(A[k], hmax(B[k], C[k]));
        const float ext = K.tightMax[k] - K.tightMin[k];
        const float t = ext > 0 ? (0.5f * (lo + hi) - K.tightMin[k]) / ext : 0.0f;
        q[k] = (uint32_t) hmin(1023.0f, hmax(0.0f, t * 1024.0f));
    }
    return (mortonSpread10(q[0]) << 2) | (mortonSpread10(q[1]) << 1) | mortonSpread10(q[2]);
}

/* What the passes share.  Node ids of the binary tree: inner node i (0 .. nValid - 2; 0 is the root) has id i, the leaf at place p of the sorted order id
   nValid - 1 + p.  A reference is >= 0 for an inner node and ~p for a leaf, as in bvh.h */
struct RebuildTree {
    const uint32_t *keys, *tris;     /* sorted (key, triangle) pairs; the first nValid are in the tree */
    uint32_t nValid;
    int32_t *child;                  /* 2 per inner node */
    uint32_t *range;                 /* 2 per inner node: first and last place of its leaves */
    uint32_t *parent;                /* per node id; REBUILD_NO_NODE for the root */
    float *box;                      /* 6 per node id: the bounds of the triangles below it, not padded (the collapse compares areas; the refit writes the boxes that are traversed) */
    uint32_t *arrived;               /* per inner node: children that have delivered their box */
};
RHD uint32_t rebuildNodeId(const RebuildTree &T, int32_t ref) { return ref >= 0 ? (uint32_t) ref : T.nValid - 1u + ~(uint32_t) ref; }
RHD uint32_t rebuildCount(const RebuildTree &T, int32_t ref) { return ref >= 0 ? T.range[2 * (size_t) ref + 1] - T.range[2 * (size_t) ref] + 1u : 1u; }
RHD uint32_t rebuildFirst(const RebuildTree &T, int32_t ref) { return ref >= 0 ? T.range[2 * (size_t) ref] : ~(uint32_t) ref; }

/* length of the common prefix of the keys at places i and j, -1 outside the array */
RHD int rebuildDelta(const uint32_t *keys, uint32_t n, long long i, long long j) {
    if (j < 0 || j >= (long long) n) return -1;
    const uint32_t a = keys[i], b = keys[j];
    if (a != b) return __builtin_clz(a ^ b);
    return 32 + __builtin_clz((uint32_t) i ^ (uint32_t) j);
}
/* inner node i: range, split, children, and its children's parent (Karras 2012, figure 4) */
RHD void rebuildInnerNode(const RebuildTree &T, uint32_t i) {
    const uint32_t *keys = T.keys; const uint32_t n = T.nValid;
    const int d = rebuildDelta(keys, n, i, (long long) i + 1) - rebuildDelta(keys, n, i, (long long) i - 1) >= 0 ? 1 : -1;
    const int dmin = rebuildDelta(keys, n, i, (long long) i - d);
    long long lmax = 2;
    while (rebuildDelta(keys, n, i, (long long) i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (rebuildDelta(keys, n, i, (long long) i + (l + t) * d) > dmin) l += t;
    const long long j = (long long) i + l * d;
    const int dnode = rebuildDelta(keys, n, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (rebuildDelta(keys, n, i, (long long) i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const long long gamma = (long long) i + s * d + (d < 0 ? -1 : 0);
    const uint32_t first = (uint32_t) (j < (long long) i ? j : (long long) i), last = (uint32_t) (j < (long long) i ? (long long) i : j);
    const int32_t left = first == (uint32_t) gamma ? ~(int32_t) gamma : (int32_t) gamma;
    const int32_t right = last == (uint32_t) gamma + 1u ? ~(int32_t) (gamma + 1) : (int32_t) (gamma + 1);
    T.child[2 * (size_t) i] = left; T.child[2 * (size_t) i + 1] = right;
    T.range[2 * (size_t) i] = first; T.range[2 * (size_t) i + 1] = last;
    T.parent[rebuildNodeId(T, left)] = i; T.parent[rebuildNodeId(T, right)] = i;
    if (i == 0u) T.parent[0] = REBUILD_NO_NODE;
}

/* the box of the leaf at place p */
RHD void rebuildLeafBox(const RebuildTree &T, const float4 *triShade, uint32_t stride, uint32_t p, float *mn, float *mx) {
    for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
    growByTriangle(triShade, stride, T.tris[p], mn, mx);
    float *b = T.box + 6 * (size_t) (T.nValid - 1u + p);
    for (int a = 0; a < 3; ++a) { b[a] = mn[a]; b[3 + a] = mx[a]; }
}
/* one step of the climb from node `cur` (box mn / mx, already stored) to its parent, for the child that arrives second: the union of the two children's boxes
   becomes the parent's.  `arrivedBefore` = the flag's value before this child's increment; returns false for the child that arrives first, which is done */
RHD bool rebuildClimbStep(const RebuildTree &T, uint32_t &cur, uint32_t par, uint32_t arrivedBefore, float *mn, float *mx) {
    if (arrivedBefore == 0u) return false;
    const int32_t l = T.child[2 * (size_t) par], r = T.child[2 * (size_t) par + 1];
    const uint32_t lid = rebuildNodeId(T, l), sib = lid == cur ? rebuildNodeId(T, r) : lid;
    const float *sb = T.box + 6 * (size_t) sib;
    float *pb = T.box + 6 * (size_t) par;
    for (int a = 0; a < 3; ++a) { mn[a] = hmin(mn[a], sb[a]); mx[a] = hmax(mx[a], sb[3 + a]); pb[a] = mn[a]; pb[3 + a] = mx[a]; }
    cur = par;
    return true;
}

/* ---- collapse ---- */
RHD bool rebuildIsInnerChild(const RebuildTree &T, int32_t ref) { return ref >= 0 && rebuildCount(T, ref) > REBUILD_LEAF_MAX; }
/* the wide node whose work item is the binary reference `item`: its children by slot (slotRef[8]: a reference, or REBUILD_EMPTY_SLOT), the number of inner
   children and of records */
RHD void rebuildCollapseNode(const RebuildTree &T, int32_t item, int32_t *slotRef, uint32_t &nInner, uint32_t &nRecs) {
    int32_t refs[8]; int n = 0;
    if (!rebuildIsInnerChild(T, item)) refs[n++] = item;             /* (the root of a tree of at most three triangles: one leaf slot) */
    else {
        refs[0] = T.child[2 * (size_t) item]; refs[1] = T.child[2 * (size_t) item + 1]; n = 2;
        while (n < 8) {
            float best = -1.0f; int bk = -1;
            for (int k = 0; k < n; ++k) {
                if (refs[k] < 0) continue;                             /* (any inner node is openable while slots are free: a small subtree becomes single triangles with boxes of their own) */
                const float *b = T.box + 6 * (size_t) rebuildNodeId(T, refs[k]);
                const float area = boxArea(b, b + 3);
                if (area > best) { best = area; bk = k; }
            }
            if (bk < 0) break;
            const int32_t open = refs[bk];
            refs[bk] = T.child[2 * (size_t) open]; refs[n++] = T.child[2 * (size_t) open + 1];
        }
    }
    float cmn[8][3], cmx[8][3], nmn[3] = { INFINITY, INFINITY, INFINITY }, nmx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int k = 0; k < n; ++k) {
        const float *b = T.box + 6 * (size_t) rebuildNodeId(T, refs[k]);
        for (int a = 0; a < 3; ++a) { cmn[k][a] = b[a]; cmx[k][a] = b[3 + a]; nmn[a] = hmin(nmn[a], b[a]); nmx[a] = hmax(nmx[a], b[3 + a]); }
    }
    int slotOf[8];
    wideAssignSlots(cmn, cmx, n, nmn, nmx, slotOf);
    for (int s = 0; s < 8; ++s) slotRef[s] = REBUILD_EMPTY_SLOT;
    nInner = 0u; nRecs = 0u;
    for (int k = 0; k < n; ++k) {
        slotRef[slotOf[k]] = refs[k];
        if (rebuildIsInnerChild(T, refs[k])) ++nInner; else nRecs += rebuildCount(T, refs[k]);
    }
}
/* ... and its node, once the scan over the level has placed its children (childBase) and its records (triBase): imask, meta, childBase, triBase -- the words a
   refit keeps; everything else is zero until the refit writes it --, the primitive of its records, its inner children's work items.  Returns its leaf slots */
RHD uint32_t rebuildEmitNode(const RebuildTree &T, const int32_t *slotRef, uint32_t childBase, uint32_t triBase, uint4 *nd, uint32_t *wRecPrim, int32_t *items) {
    uint32_t imask = 0u, rank = 0u, triOff = 0u, leaves = 0u, meta[2] = { 0u, 0u };
    for (uint32_t s = 0; s < 8u; ++s) {
        const int32_t ref = slotRef[s];
        if (ref == REBUILD_EMPTY_SLOT) continue;
        uint32_t m;
        if (rebuildIsInnerChild(T, ref)) {
            imask |= 1u << s;
            m = 0x20u | (24u + s);
            items[childBase + rank] = ref; ++rank;
        } else {
            const uint32_t cnt = rebuildCount(T, ref), first = rebuildFirst(T, ref);
            m = (((1u << cnt) - 1u) << 5) | triOff;
            for (uint32_t k = 0; k < cnt; ++k) wRecPrim[triBase + triOff + k] = T.tris[first + k];
            triOff += cnt; ++leaves;
        }
        meta[s >> 2] |= m << (8u * (s & 3u));
    }
    nd[0] = make_uint4(0u, 0u, 0u, imask << 24);
    nd[1] = make_uint4(childBase, triBase, meta[0], meta[1]);
    nd[2] = make_uint4(0u, 0u, 0u, 0u); nd[3] = make_uint4(0u, 0u, 0u, 0u); nd[4] = make_uint4(0u, 0u, 0u, 0u);
    return leaves;
}

#undef RHD

} // namespace detail
} // namespace pt

/* what the kernels of k_rebuild.h get (filled by host_rebuild.h) */
struct RebuildArgs {
    pt::detail::RebuildTree tree;
    const float4 *triShade; uint32_t stride, nTriangles;
    const pt::detail::RefitConsts *consts;
    uint32_t *keysOut, *trisOut;             /* k_rb_keys: the unsorted pairs */
    uint32_t *hadRecord;                     /* one bit per triangle: it is in the tree */
    uint32_t *counters;                      /* [0] triangles in the tree, [1] leaf slots */
    int32_t *items;                          /* per wide node: the binary reference it collapses */
    int32_t *slotRef;                        /* 8 per wide node */
    unsigned long long *scanIn, *scanOut;    /* per node of the level in flight, and one more: inner children | records << 32 */
    uint4 *wnodes; uint32_t nodeStride;
    uint32_t *wRecPrim;
    const uint8_t *triClass;                 /* the shade class of every triangle (host_scene.h: tagShadeClasses) */
    float4 *wtris;
};

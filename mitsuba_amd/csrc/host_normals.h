/*
 * host_normals.h -- host side of phip_vertex_normals_device and of the host call phip_vertex_normals: the angle-weighted vertex normals of the reference's
 * TriMesh::computeNormals from positions on the caller's device memory (the kernel: k_normals.h in phip_normals.hip) and on host memory.  Both run the statements of
 * normals_hd.h; this header holds the checks of the arguments (all of them before any write), the incidence lists and the order of the host loop.
 * The incidence lists (SceneDev::normals) are a CSR over the scene's indices: offsets of n_vertices + 1, entries of 3 * n_triangles, an entry = 3 * triangle + corner.
 * A counting sort over the creation's indices (SceneUpdateState::indices) fills every list in ascending order, which is the reference's order of summation.  They are
 * made at the scene's first call and kept: phip_scene_update, phip_scene_rebuild and phip_scene_update_appearance change no index.  After that call nothing is allocated.
 * Host code only; included by phip.hip alone, after host_boundary.h.  The caller of vertexNormalsDevice holds the scene's render lock.
 */
#pragma once
#include "host_boundary.h"
#include "normals_hd.h"

static bool normalsRangesOverlap(const phip_normals_desc *p) {
    const uintptr_t a = (uintptr_t) p->positions, b = (uintptr_t) p->normals, bytes = (uintptr_t) p->n_vertices * 3u * sizeof(float);
    return a < b + bytes && b < a + bytes;
}

/* What the arguments of the device call say without a device: NULL, or the refusal (PHIP_ERR_INVALID, all of them).  sceneVertices / sceneTriangles: the scene's counts */
static const char *normalsArgsError(bool haveScene, uint32_t sceneVertices, uint32_t sceneTriangles, const phip_normals_desc *p) {
    if (!haveScene || !p) return "NULL argument";
    if (!p->positions || !p->normals) return "positions and normals must not be NULL";
    if (p->n_vertices != sceneVertices || p->n_triangles != sceneTriangles) return "n_vertices and n_triangles must be the scene's";
    if (p->indices) return "indices must be NULL: the device call uses the scene's own";
    if (misaligned(p->positions, 4) || misaligned(p->normals, 4)) return "every pointer must be 4-byte aligned";
    if (normalsRangesOverlap(p)) return "positions and normals overlap";
    return nullptr;
}
static int normalsRefusal(bool haveScene, uint32_t sceneVertices, uint32_t sceneTriangles, const phip_normals_desc *p) {
    return refusal("phip_vertex_normals_device", PHIP_ERR_INVALID, normalsArgsError(haveScene, sceneVertices, sceneTriangles, p));
}
/* ... and those of the host call */
static const char *normalsHostArgsError(const phip_normals_desc *p) {
    if (!p) return "NULL argument";
    if (!p->positions || !p->normals || (p->n_triangles && !p->indices)) return "positions, normals and indices must not be NULL";
    if (p->n_vertices == 0) return "n_vertices must not be 0";
    if (misaligned(p->positions, 4) || misaligned(p->normals, 4) || misaligned(p->indices, 4)) return "every pointer must be 4-byte aligned";
    if (normalsRangesOverlap(p)) return "positions and normals overlap";
    for (size_t i = 0; i < 3 * (size_t) p->n_triangles; ++i)
        if (p->indices[i] >= p->n_vertices) return "triangle index out of range";
    return nullptr;
}
static int normalsHostRefusal(const phip_normals_desc *p) { return refusal("phip_vertex_normals", PHIP_ERR_INVALID, normalsHostArgsError(p)); }

/* the incidence lists of the creation's indices on the device, the events, the counter: the first call's work */
static void normalsPrepare(SceneDev &sd, const SceneUpdateState &U) {
    if (sd.normals.ready) return;
    const size_t nV = U.nVertices, nE = 3 * (size_t) U.nTriangles;
    if (nE > 0xFFFFFFFFull) throw std::runtime_error("more than 2^32 / 3 triangles: an incidence entry is 32 bits");
    /* (a kernel argument must not be NULL: a scene without triangles uploads one word of nothing for its entries and its indices) */
    std::vector<uint32_t> offsets(nV + 1, 0u), entries(std::max<size_t>(nE, 1), 0u), indices(U.indices);
    if (indices.empty()) indices.push_back(0u);
    for (size_t e = 0; e < nE; ++e) ++offsets[U.indices[e] + 1];
    for (size_t v = 0; v < nV; ++v) offsets[v + 1] += offsets[v];
    std::vector<uint32_t> next(offsets.begin(), offsets.end() - 1);
    for (size_t e = 0; e < nE; ++e) entries[next[U.indices[e]]++] = (uint32_t) e;          /* ascending e within every list: ascending triangle order */
    sd.normals.offsets.upload(offsets.data(), offsets.size());
    sd.normals.entries.upload(entries.data(), entries.size());
    sd.normals.indices.upload(indices.data(), indices.size());
    sd.normals.invalid.alloc(1);
    HIP_TRY(hipEventCreate(&sd.normals.t0)); HIP_TRY(hipEventCreate(&sd.normals.t1));
    sd.normals.ready = true;
}

static int vertexNormalsDevice(phip_scene *sc, const phip_normals_desc *p, phip_normals_info *info) {
    SceneDev &sd = *sc->devs[0];
    if (!allOnSceneDevice(sd, { p->positions, p->normals }))
        return setErr(PHIP_ERR_INVALID, "phip_vertex_normals_device: every pointer must be device memory of the scene's device");
    if (p->n_vertices == 0) return PHIP_OK;
    normalsPrepare(sd, sc->upd);
    const hipStream_t stream = sceneStream(sd, p->stream);
    const NormalsKernels K = phipNormalsKernels();
    HIP_TRY(hipMemsetAsync(sd.normals.invalid.p, 0, sizeof(unsigned int), stream));
    HIP_TRY(hipEventRecord(sd.normals.t0, stream));
    hipLaunchKernelGGL(K.vertexNormals, dim3((unsigned) (((size_t) p->n_vertices + NRM_BLOCK - 1) / NRM_BLOCK)), dim3(NRM_BLOCK), 0, stream,
                       (const uint32_t *) sd.normals.offsets.p, (const uint32_t *) sd.normals.entries.p, (const uint32_t *) sd.normals.indices.p, p->positions, p->n_vertices,
                       p->normals, sd.normals.invalid.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sd.normals.t1, stream));
    unsigned int nInvalid = 0;
    HIP_TRY(hipMemcpyAsync(&nInvalid, sd.normals.invalid.p, sizeof(nInvalid), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (info) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, sd.normals.t0, sd.normals.t1));
        info->n_invalid = nInvalid; info->kernel_ms = (double) ms;
    }
    return PHIP_OK;
}

/* the kernel's twin on host memory: the reference's own loop (trimesh.cpp:640-672), a scatter in triangle order -- every vertex receives its corners in the order
   the kernel's lane gathers them, so the sums are the same bits */
static void vertexNormalsHost(const phip_normals_desc *p, phip_normals_info *info) {
    using namespace detail;
    const size_t nV = p->n_vertices;
    float *N = p->normals;
    for (size_t i = 0; i < 3 * nV; ++i) N[i] = 0.0f;
    for (size_t t = 0; t < p->n_triangles; ++t) {
        const uint32_t *idx = p->indices + 3 * t;
        const N3 v[3] = { normalsLoad(p->positions, idx[0]), normalsLoad(p->positions, idx[1]), normalsLoad(p->positions, idx[2]) };
        N3 n;
        if (!normalsFace(v[0], v[1], v[2], n)) continue;
        for (int i = 0; i < 3; ++i) {
            const N3 c = normalsCorner(n, v[i], v[(i + 1) % 3], v[(i + 2) % 3]);
            float *o = N + 3 * (size_t) idx[i];
            o[0] = o[0] + c.x; o[1] = o[1] + c.y; o[2] = o[2] + c.z;
        }
    }
    uint32_t nInvalid = 0;
    for (size_t i = 0; i < nV; ++i) {
        N3 n = normalsLoad(N, (uint32_t) i);
        if (!normalsFinish(n)) ++nInvalid;
        N[3 * i] = n.x; N[3 * i + 1] = n.y; N[3 * i + 2] = n.z;
    }
    if (info) info->n_invalid = nInvalid;
}

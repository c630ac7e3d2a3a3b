/*
 * normals_hd.h -- the vertex normals of the reference's TriMesh::computeNormals (trimesh.cpp:640-672: Thuermer and Wuethrich's angle weighting), stated once as
 * __host__ __device__ functions: the kernel of phip_vertex_normals_device (k_normals.h) and the host call phip_vertex_normals (host_normals.h) both run these and
 * nothing else.  What is restated, with the reference's vector operators as its headers spell them:
 *   length      std::sqrt(x*x + y*y + z*z), the sum from left to right (vector.h:566-573)
 *   v / f, v /= f   ONE reciprocal, recip = 1 / f, and three products (vector.h:535-553) -- not three divisions; normalize(v) is v / v.length() (vector.h:625-627)
 *   cross       (y1*z2 - z1*y2, z1*x2 - x1*z2, x1*y2 - y1*x2) (vector.h:617-623); dot: x1*x2 + y1*y2 + z1*z2 from left to right (vector.h:609-611)
 *   the face    at corner 0: n = cross(v1 - v0, v2 - v0); a length of exactly 0 ends the triangle (the `break`: none of its corners contributes); else n /= length
 *   the corner  i: sideA = v[(i+1)%3] - v[i], sideB = v[(i+2)%3] - v[i]; n * unitAngle(normalize(sideA), normalize(sideB)) is added to vertex idx[i]
 *   unitAngle   core/util.h:309-314: dot(u, v) < 0: M_PI - 2 * asin(0.5f * (v + u).length()), else 2 * asin(0.5f * (v - u).length()); M_PI is the single-precision
 *               constant 3.14159265358979323846f (constants.h:63,80); asin is pm_asinf (phip_fmath.h)
 *   the vertex  the sum starts at +0 and takes its corners in ascending triangle order; its length != 0: n /= length; else (1, 0, 0), counted as invalid
 * m_flipNormals is not restated: a caller negates.  All float32, one IEEE operation per statement, -ffp-contract=off on both sides.
 */
#pragma once
#include <cstdint>
#include "dv_math.h"
#include "../../include/phip.h"

namespace pt {
namespace detail {

#define NHD __host__ __device__ inline

struct N3 { float x, y, z; };

NHD N3 normalsLoad(const float *p, uint32_t i) { N3 r; r.x = p[3 * (size_t) i]; r.y = p[3 * (size_t) i + 1]; r.z = p[3 * (size_t) i + 2]; return r; }
NHD N3 normalsSub(const N3 &a, const N3 &b) { N3 r; r.x = a.x - b.x; r.y = a.y - b.y; r.z = a.z - b.z; return r; }
NHD N3 normalsAdd(const N3 &a, const N3 &b) { N3 r; r.x = a.x + b.x; r.y = a.y + b.y; r.z = a.z + b.z; return r; }
NHD N3 normalsMul(const N3 &a, float f) { N3 r; r.x = a.x * f; r.y = a.y * f; r.z = a.z * f; return r; }
NHD float normalsLength(const N3 &a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
/* operator/ and operator/= of TVector3: a reciprocal and three products */
NHD N3 normalsDiv(const N3 &a, float f) { const float recip = 1.0f / f; return normalsMul(a, recip); }
NHD float normalsDot(const N3 &a, const N3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
NHD N3 normalsCross(const N3 &a, const N3 &b) {
    N3 r;
    r.x = (a.y * b.z) - (a.z * b.y);
    r.y = (a.z * b.x) - (a.x * b.z);
    r.z = (a.x * b.y) - (a.y * b.x);
    return r;
}

/* unitAngle of two unit vectors */
NHD float normalsUnitAngle(const N3 &u, const N3 &v) {
    if (normalsDot(u, v) < 0.0f)
        return PM_PI - 2.0f * pm_asinf(0.5f * normalsLength(normalsAdd(v, u)));
    return 2.0f * pm_asinf(0.5f * normalsLength(normalsSub(v, u)));
}

/* the unit normal of the triangle (v0, v1, v2) as corner 0 makes it; false: its length is 0 and the triangle contributes nothing */
NHD bool normalsFace(const N3 &v0, const N3 &v1, const N3 &v2, N3 &n) {
    n = normalsCross(normalsSub(v1, v0), normalsSub(v2, v0));
    const float length = normalsLength(n);
    if (length == 0.0f) return false;
    n = normalsDiv(n, length);
    return true;
}

/* what the corner at v0 adds to its vertex: v1, v2 are the triangle's next two corners in its own order */
NHD N3 normalsCorner(const N3 &n, const N3 &v0, const N3 &v1, const N3 &v2) {
    const N3 sideA = normalsSub(v1, v0), sideB = normalsSub(v2, v0);
    const float angle = normalsUnitAngle(normalsDiv(sideA, normalsLength(sideA)), normalsDiv(sideB, normalsLength(sideB)));
    return normalsMul(n, angle);
}

/* a vertex's sum to its normal; false: the length is 0, the normal is (1, 0, 0) and the vertex counts as invalid */
NHD bool normalsFinish(N3 &n) {
    const float length = normalsLength(n);
    if (length != 0.0f) { n = normalsDiv(n, length); return true; }
    n.x = 1.0f; n.y = 0.0f; n.z = 0.0f;
    return false;
}

} // namespace detail
} // namespace pt

/* launch shape of k_normals.h */
#define NRM_BLOCK 256

/*
 * phip_normals.hip -- the kernel of phip_vertex_normals_device (k_normals.h: one lane per vertex gathers the angle-weighted contributions of its corners in the
 * reference's order) behind the one look-up that returns it (phip_common.h).  One object; phip.hip launches it (host_normals.h).
 */
#include "phip_common.h"
#include "k_normals.h"

NormalsKernels phipNormalsKernels() {
    NormalsKernels k;
    k.vertexNormals = k_vertex_normals;
    return k;
}

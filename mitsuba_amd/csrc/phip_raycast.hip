/*
 * phip_raycast.hip -- the kernels of phip_trace_device (k_raycast.h: k_raycast_p, the persistent ray server of k_wide.h on a caller's ray array; k_surfaces, the
 * surface records) behind the one look-up that returns them (phip_common.h).  One object; phip.hip asks for the server's residency and launches both (host_raycast.h).
 */
#include "phip_common.h"
#include "k_traverse.h"
#define WIDE_SERVER_ONLY      /* k_wide.h without k_rays_w and k_raycast_w: those are phip.hip's */
#include "k_wide.h"
#include "k_raycast.h"

RaycastKernels phipRaycastKernels() {
    RaycastKernels k;
    k.cast = k_raycast_p; k.surfaces = k_surfaces;
    return k;
}

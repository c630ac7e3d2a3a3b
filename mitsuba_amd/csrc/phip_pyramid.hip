/*
 * phip_pyramid.hip -- the kernels of phip_mip_pyramid_device (k_pyramid.h: level 0 into the float32 chain, one pass of one resampling step, the tail of the pyramid
 * in one block's LDS) behind the one look-up that returns them (phip_common.h).  One object; phip.hip launches them (host_pyramid.h).
 */
#include "phip_common.h"
#include "k_pyramid.h"

PyramidKernels phipPyramidKernels() {
    PyramidKernels k;
    k.level0 = k_pyramid_level0; k.pass = k_pyramid_pass; k.tail = k_pyramid_tail;
    return k;
}

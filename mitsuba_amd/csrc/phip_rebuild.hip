/*
 * phip_rebuild.hip -- the kernels of phip_scene_rebuild (k_rebuild.h: keys, the binary radix tree and its boxes, the collapse to the 8-wide layout level by level)
 * behind the one look-up that returns them, and the two rocPRIM calls of the pipeline -- the stable radix sort of the (key, triangle) pairs and the exclusive scan
 * over a level -- behind two functions (rocPRIM is header-only and launches its own kernels: they are instantiated here).  One object; phip.hip drives it
 * (host_rebuild.h).
 */
#include "phip_common.h"
#include <rocprim/rocprim.hpp>
#include "k_rebuild.h"

RebuildKernels phipRebuildKernels() {
    RebuildKernels k;
    k.keys = k_rb_keys; k.inner = k_rb_inner; k.boxes = k_rb_boxes; k.collapse = k_rb_collapse; k.emit = k_rb_emit; k.shadeClass = k_rb_class;
    return k;
}

/* temp == NULL: the size of the temporary storage is returned in tempBytes and nothing runs (rocPRIM's convention) */
hipError_t phipRebuildSortPairs(void *temp, size_t &tempBytes, const uint32_t *keysIn, uint32_t *keysOut, const uint32_t *trisIn, uint32_t *trisOut, uint32_t n, hipStream_t stream) {
    return rocprim::radix_sort_pairs(temp, tempBytes, keysIn, keysOut, trisIn, trisOut, (size_t) n, 0u, 32u, stream);
}
hipError_t phipRebuildScan(void *temp, size_t &tempBytes, const unsigned long long *in, unsigned long long *out, uint32_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, tempBytes, in, out, 0ull, (size_t) n, rocprim::plus<unsigned long long>(), stream);
}

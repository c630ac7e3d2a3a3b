/*
 * phip_update.hip -- the kernels of phip_scene_update (k_update.h: check, shading records, scene box, Wald records, the level-by-level refit of the 8-wide tree, the
 * packed leaf table) behind the one look-up that returns them (phip_common.h).  One object; phip.hip launches them (host_update.h).
 */
#include "phip_common.h"
#include "k_update.h"

UpdateKernels phipUpdateKernels() {
    UpdateKernels k;
    k.check = k_upd_check; k.shade = k_upd_shade; k.box = k_upd_box; k.boxFinal = k_upd_box_final;
    k.wald = k_upd_wald; k.refitLevel = k_upd_refit_level; k.leafTable = k_upd_leaf_table;
    return k;
}

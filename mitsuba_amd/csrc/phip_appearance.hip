/*
 * phip_appearance.hip -- the kernels of phip_scene_update_appearance (k_appearance.h: the texel maximum, the texel conversion, the environment map's CDFs, the
 * material words of the shading records, the shade classes of the Wald records) behind the one look-up that returns them (phip_common.h).  One object; phip.hip
 * launches them (host_appearance.h).
 */
#include "phip_common.h"
#include "k_appearance.h"

AppearanceKernels phipAppearanceKernels() {
    AppearanceKernels k;
    k.texmax = k_appearance_texmax; k.texels = k_appearance_texels; k.envRows = k_envmap_cdf_rows; k.envMarginal = k_envmap_cdf_marginal;
    k.records = k_appearance_records; k.classes = k_appearance_classes;
    return k;
}

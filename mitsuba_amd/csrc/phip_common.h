/*
 * phip_common.h -- what every translation unit of libphip.so starts with: HIP, the C ABI, the device scene layout and
 * shading functions (dv_scene.h), the path-pool layout (k_pool.h), the error macro.
 *
 * libphip.so is built from thirteen sources (50 objects) so that they compile in parallel:
 *   phip.hip          the C ABI + traversal and film kernels, with the host side it includes by concern: host_scene.h (scene build, replicas), host_boundary.h (what
 *                     a call on the caller's device memory needs), host_render.h (kernel selection, one device's render loop), host_multi.h (multi-device
 *                     orchestration, RCCL) and one header per entry point on the caller's device memory: 1 object
 *   phip_shade.hip    k_shade / k_shade_direct / k_shade_trace instantiations behind the look-ups phipShade*KernelF<n> -- compiled per feature set (-DSHADE_FEAT=0..3, 8
 *                     and 11: environment emitter, bitmap textures, the QMC samplers) and per part (-DSHADE_PART=0..3), 24 objects: see its header
 *   phip_shade_w.hip  k_shade_trace_w instantiations behind phipShadeTraceWideKernelF<n>, per feature set: 6 objects
 *   phip_mega.hip     k_mega instantiations behind phipMegaKernel (-DMEGA_PART=0: scenes in LDS) / phipMegaKernelWide (-DMEGA_PART=1: the 8-wide tree in memory) /
 *                     phipMegaKernelDirect (-DMEGA_PART=2: `direct`): 3 objects
 *   phip_update.hip   the kernels of phip_scene_update (k_update.h) behind phipUpdateKernels: 1 object
 *   phip_rebuild.hip  the kernels of phip_scene_rebuild (k_rebuild.h) behind phipRebuildKernels, and its two rocPRIM calls (sort, scan): 1 object
 *   phip_raycast.hip  the kernels of phip_trace_device (k_raycast.h) behind phipRaycastKernels: 1 object
 *   phip_shade_r.hip  the kernels of phip_radiance_device (k_shade_r.h) behind phipShadeRaysKernelS<s>F<n> and phipRadianceOutKernel -- per feature set (-DSHADE_FEAT=0..3) and
 *                     strictNormals (-DSHADE_PART=0 / 1): 8 objects
 *   phip_camera_film.hip  the kernels of phip_camera_rays_device and phip_film_device (k_camera_film.h) behind phipCameraFilmKernels: 1 object
 *   phip_appearance.hip   the kernels of phip_scene_update_appearance (k_appearance.h) behind phipAppearanceKernels: 1 object
 *   phip_shading_parts.hip  the kernels of phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device (k_shading_parts.h) behind
 *                     phipShadingPartsKernels: 1 object
 *   phip_pyramid.hip  the kernels of phip_mip_pyramid_device (k_pyramid.h) behind phipPyramidKernels: 1 object
 *   phip_normals.hip  the kernel of phip_vertex_normals_device (k_normals.h) behind phipNormalsKernels: 1 object
 * The other units hold kernels and the look-ups that return them, nothing else: every launch and every query of the runtime is in phip.hip and its host headers
 * (but for the launches inside rocPRIM's sort and scan, which phip_rebuild.hip wraps).
 * No device function is called across units (everything on the device side is inline in headers), so no -fgpu-rdc.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "../../include/phip.h"
#include "dv_scene.h"

using namespace pt;

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e__));         \
    } while (0)

#include "k_pool.h"
#include "k_clip.h"

/* ---- kernels defined in the other translation units: every unit exports typed look-ups that RETURN its kernels; phip.hip selects one per render and launches it ---- */
typedef void (*ShadeKernel)(DevScene, PathPool, RenderConst, float4 *);                             /* k_shade, k_shade_direct, k_shade_trace */
typedef void (*ShadeTraceWideKernel)(DevScene, PathPool, RenderConst, float4 *, uint32_t);          /* k_shade_trace_w: ... and the staged nodes */
typedef void (*MegaKernel)(DevScene, MegaParams, RenderConst, float4 *);                            /* k_mega */
/* per feature set n (phip_shade.hip / phip_shade_w.hip compiled with -DSHADE_FEAT=n): k_shade<materials, strictNormals = 0 / 1, FEAT> by the leaf BSDF models present and
   the table set (0 = generic pointers; FEAT 0 only: 1 = emitter table and materials addressed as LDS, 2 = the emitter table only); k_shade_direct<materials, FEAT>;
   k_shade_trace and k_shade_trace_w<materials, strictNormals, FEAT> */
#define PHIP_DECLARE_SHADE_KERNELS(n)                                                   \
    ShadeKernel phipShadeKernelS0F##n(int materialMask, int tables);                    \
    ShadeKernel phipShadeKernelS1F##n(int materialMask, int tables);                    \
    ShadeKernel phipShadeDirectKernelF##n(int materialMask);                            \
    ShadeKernel phipShadeTraceKernelF##n(bool strictNormals, int materialMask);         \
    ShadeTraceWideKernel phipShadeTraceWideKernelF##n(bool strictNormals, int materialMask);
PHIP_DECLARE_SHADE_KERNELS(0) PHIP_DECLARE_SHADE_KERNELS(1) PHIP_DECLARE_SHADE_KERNELS(2) PHIP_DECLARE_SHADE_KERNELS(3) PHIP_DECLARE_SHADE_KERNELS(8) PHIP_DECLARE_SHADE_KERNELS(11)
#undef PHIP_DECLARE_SHADE_KERNELS
/* k_mega<materials, strictNormals, traversal form, QMC[, DIRECT]> (phip_mega.hip), nullptr for a form the part does not hold: flat 2 / 3 (DevScene::flatMode: scenes that
   fit LDS) in the object compiled with -DMEGA_PART=0, flat 4 / 5 (the 8-wide tree in memory) in -DMEGA_PART=1, `direct` with flat 2 .. 5 in -DMEGA_PART=2 */
MegaKernel phipMegaKernel(int materialMask, bool strictNormals, int flat, bool qmc);
MegaKernel phipMegaKernelWide(int materialMask, bool strictNormals, int flat, bool qmc);
MegaKernel phipMegaKernelDirect(int materialMask, bool strictNormals, int flat, bool qmc);
/* the kernels of phip_scene_update (phip_update.hip, k_update.h); UpdateArgs is theirs */
struct UpdateArgs;
struct UpdateKernels {
    void (*check)(UpdateArgs), (*shade)(UpdateArgs), (*box)(UpdateArgs), (*boxFinal)(UpdateArgs, uint32_t);
    void (*wald)(UpdateArgs, float4 *, const uint32_t *, uint32_t);
    void (*refitLevel)(UpdateArgs, uint32_t, uint32_t), (*leafTable)(UpdateArgs);
};
UpdateKernels phipUpdateKernels();
/* the kernels of phip_scene_rebuild (phip_rebuild.hip, k_rebuild.h); RebuildArgs is theirs.  The sort of the (key, triangle) pairs and the scan over a level are rocPRIM's:
   temp == NULL returns the size of the temporary storage in tempBytes and runs nothing */
struct RebuildArgs;
struct RebuildKernels {
    void (*keys)(RebuildArgs), (*inner)(RebuildArgs), (*boxes)(RebuildArgs);
    void (*collapse)(RebuildArgs, uint32_t, uint32_t), (*emit)(RebuildArgs, uint32_t, uint32_t, uint32_t, uint32_t), (*shadeClass)(RebuildArgs, uint32_t);
};
RebuildKernels phipRebuildKernels();
hipError_t phipRebuildSortPairs(void *temp, size_t &tempBytes, const uint32_t *keysIn, uint32_t *keysOut, const uint32_t *trisIn, uint32_t *trisOut, uint32_t n, hipStream_t stream);
hipError_t phipRebuildScan(void *temp, size_t &tempBytes, const unsigned long long *in, unsigned long long *out, uint32_t n, hipStream_t stream);
/* the kernels of phip_trace_device (phip_raycast.hip, k_raycast.h): rays, hits and surface records as the 16-byte words they are made of */
struct RaycastKernels {
    void (*cast)(DevScene, const float4 *, uint32_t, float4 *, uint8_t *, PathPool, unsigned int *);
    void (*surfaces)(DevScene, const float4 *, const float4 *, uint32_t, float4 *);
};
RaycastKernels phipRaycastKernels();
/* the kernels of phip_radiance_device (phip_shade_r.hip, k_shade_r.h).  Per feature set n = 0..3 and strictNormals = 0 / 1 (compiled with -DSHADE_FEAT=n -DSHADE_PART=0 / 1):
   k_shade_r<materials, strictNormals, FEAT> by the leaf BSDF models present and k_shade's table set; RaySamples, the ray array it draws its samples from, is an argument
   of these kernels alone.  k_radiance_out: (L, acc, n, sppPass, spp, first, last, out, invalid) */
struct RaySamples;
typedef void (*ShadeRaysKernel)(DevScene, PathPool, RenderConst, float4 *, RaySamples);
typedef void (*RadianceOutKernel)(const float4 *, double2 *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, float4 *, unsigned long long *);
#define PHIP_DECLARE_RADIANCE_KERNELS(n)                                                \
    ShadeRaysKernel phipShadeRaysKernelS0F##n(int materialMask, int tables);            \
    ShadeRaysKernel phipShadeRaysKernelS1F##n(int materialMask, int tables);
PHIP_DECLARE_RADIANCE_KERNELS(0) PHIP_DECLARE_RADIANCE_KERNELS(1) PHIP_DECLARE_RADIANCE_KERNELS(2) PHIP_DECLARE_RADIANCE_KERNELS(3)
#undef PHIP_DECLARE_RADIANCE_KERNELS
RadianceOutKernel phipRadianceOutKernel();
/* the kernels of phip_camera_rays_device and phip_film_device (phip_camera_film.hip, k_camera_film.h): the check of a pixel list, the camera samples, and
   ImageBlock::put on a caller's values without / with PHIP_FILM_SIGNED */
struct CameraFilmKernels {
    void (*pixelsCheck)(const uint32_t *, uint32_t, uint32_t, unsigned long long *);
    void (*rays)(DevScene, RenderConst, const uint32_t *, uint32_t, float4 *, uint2 *, float2 *);
    void (*film[2])(DevScene, RenderConst, const float4 *, float *, int, unsigned long long *);
};
CameraFilmKernels phipCameraFilmKernels();
/* the kernels of phip_scene_update_appearance (phip_appearance.hip, k_appearance.h); ShapeWords (appearance_hd.h) is the per-shape table of the records pass */
namespace pt { namespace detail { struct ShapeWords; } }
struct AppearanceKernels {
    void (*texmax)(const float *, uint32_t, uint32_t *);
    void (*texels)(const float *, float4 *, uint32_t);
    void (*envRows)(const float4 *, int, int, float *, float *, float *);
    void (*envMarginal)(const float *, int, float *, float *);
    void (*records)(float4 *, uint32_t, uint32_t, const uint32_t *, const pt::detail::ShapeWords *, uint8_t *);
    void (*classes)(float4 *, const uint32_t *, uint32_t, const uint8_t *, uint32_t);
};
AppearanceKernels phipAppearanceKernels();
/* the kernels of phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device (phip_shading_parts.hip, k_shading_parts.h).  bsdf[eval | 2 * sample]:
   (scene, rays, hits, wo, samples, n, local, eval out, sampled out, wi out); emitterSample / emitterEval[the scene has an environment emitter]:
   (scene, ref, refN, samples, n, sampled out, shadow rays out) and (scene, rays, hits, refN, n, eval out, emitter out) */
struct ShadingPartsKernels {
    void (*bsdf[4])(DevScene, const float4 *, const float4 *, const float4 *, const float2 *, uint32_t, uint32_t, float4 *, float4 *, float4 *);
    void (*emitterSample[2])(DevScene, const float4 *, const float4 *, const float2 *, uint32_t, float4 *, float4 *);
    void (*emitterEval[2])(DevScene, const float4 *, const float4 *, const float4 *, uint32_t, float4 *, int32_t *);
};
ShadingPartsKernels phipShadingPartsKernels();
/* the kernels of phip_mip_pyramid_device (phip_pyramid.hip, k_pyramid.h; PyramidOuts: pyramid_hd.h).  level0: (level 0, texels, chain out, rounded out);
   pass: (source, source width, source height, float32 out, rounded out, axis, wrap mode, max value); tail: (float32 level, width, height, its index, the caller's
   levels, wrap u, wrap v, max value) */
struct PyramidOuts;
struct PyramidKernels {
    void (*level0)(const float *, size_t, float *, float *);
    void (*pass)(const float *, int, int, float *, float *, int, uint32_t, float);
    void (*tail)(const float *, int, int, int, PyramidOuts, uint32_t, uint32_t, float);
};
PyramidKernels phipPyramidKernels();
/* the kernel of phip_vertex_normals_device (phip_normals.hip, k_normals.h): (incidence offsets, incidence entries, the scene's indices, positions, vertex count,
   normals out, the count of invalid vertices) */
struct NormalsKernels {
    void (*vertexNormals)(const uint32_t *, const uint32_t *, const uint32_t *, const float *, uint32_t, float *, unsigned int *);
};
NormalsKernels phipNormalsKernels();

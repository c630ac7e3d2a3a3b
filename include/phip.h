/*
 * phip.h -- C ABI of the MI355X-native `path_hip` integrator back end (libphip.so).
 *
 * This is the drop-in boundary: it is exactly what a Mitsuba 0.6
 * integrator plugin `path_hip.so` (class PathHIP : MonteCarloIntegrator, see
 * mitsuba_amd/plugin/path_hip.cpp and INTEGRATION.md) binds in place of the CPU
 * per-block worker loop.  Reference interfaces replaced (file:line under /root/reference):
 *
 *   phip_scene_create   <- Scene::initialize + ShapeKDTree::build     src/librender/scene.cpp:322-384,
 *                                                                      src/librender/skdtree.cpp:68-110
 *   phip_render         <- SamplingIntegrator::render + BlockRenderer::process + renderBlock
 *                          + MIPathTracer::Li + ImageBlock::put        src/librender/integrator.cpp:95-188,
 *                                                                      src/integrators/path/path.cpp:119-300,
 *                                                                      include/mitsuba/render/imageblock.h:103-204
 *   phip_render_device  <- same, result left in device memory so the caller can RCCL-reduce it
 *                          (replaces StreamBackend::sendWorkResult,    src/libcore/sched_remote.cpp:519-532)
 *   phip_render_params.n_devices / devices[]  <- the Scheduler's worker set: one host thread + stream per GPU, the
 *                          reference's spiral block list dealt over them, the per-device films merged by one
 *                          ncclReduce(sum) (replaces BlockedRenderProcess::processResult's film->put under a mutex,
 *                          src/librender/renderproc.cpp:142-149, and sched_remote.cpp:519-532)
 *   phip_render_params.progress  <- ProgressReporter::update / RenderQueue::signalWorkEnd
 *                                                                      src/librender/renderproc.cpp:146-154
 *   phip_trace          <- ShapeKDTree::rayIntersect(ray, its) / (ray) src/librender/skdtree.cpp:112-142,207-226
 *   phip_trace_device   <- the same on device memory, with the record of fillIntersectionRecord, include/mitsuba/render/skdtree.h:343-428
 *   phip_cancel         <- SamplingIntegrator::cancel                  src/librender/integrator.cpp:90-93
 *   phip_develop        <- HDRFilm::develop weight normalisation       src/libcore/fmtconv.cpp:979-991
 *
 * Conventions: plain C, plain pointers and sizes, no exceptions cross the boundary.  Every
 * function that can fail returns 0 on success and a negative phip_status otherwise;
 * phip_last_error() returns a thread-local human-readable message.  All pointers passed in are
 * borrowed for the duration of the call only (phip_scene_create deep-copies).  All arithmetic on
 * the path is float32 / RGB (the reference's -DSINGLE_PRECISION -DSPECTRUM_SAMPLES=3 build).
 */
#ifndef PHIP_H
#define PHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHIP_ABI_VERSION 7

typedef enum phip_status {
    PHIP_OK              =  0,
    PHIP_ERR_INVALID     = -1,  /* bad argument / malformed scene description            */
    PHIP_ERR_UNSUPPORTED = -2,  /* feature outside the path (e.g. phong microfacets)     */
    PHIP_ERR_DEVICE      = -3,  /* HIP runtime error, no device, kernel failure          */
    PHIP_ERR_CANCELLED   = -4,  /* phip_cancel() was called while rendering              */
    PHIP_ERR_NOMEM       = -5
} phip_status;

/* ---- materials: src/bsdfs/{diffuse,dielectric,roughconductor,twosided}.cpp ---- */
typedef enum phip_bsdf_type {
    PHIP_BSDF_DIFFUSE        = 0,  /* SmoothDiffuse, diffuse.cpp:110-150                 */
    PHIP_BSDF_DIELECTRIC     = 1,  /* SmoothDielectric, dielectric.cpp:217-387           */
    PHIP_BSDF_ROUGHCONDUCTOR = 2,  /* RoughConductor, roughconductor.cpp:253-415         */
    PHIP_BSDF_TWOSIDED       = 3   /* TwoSidedBRDF adapter, twosided.cpp:108-183         */
} phip_bsdf_type;

typedef enum phip_microfacet_type {   /* MicrofacetDistribution::EType, microfacet.h:47-56 */
    PHIP_MF_BECKMANN = 0,
    PHIP_MF_GGX      = 1
} phip_microfacet_type;

typedef struct phip_material {
    uint32_t type;              /* phip_bsdf_type                                          */
    uint32_t nested[2];         /* TWOSIDED: material ids of the front / back BRDF
                                   (equal when only one was nested, twosided.cpp:87-88)  */
    float    reflectance[3];    /* DIFFUSE: reflectance; DIELECTRIC / ROUGHCONDUCTOR:
                                   specularReflectance                                   */
    float    transmittance[3];  /* DIELECTRIC: specularTransmittance                     */
    float    eta[3];            /* DIELECTRIC: eta[0] = intIOR/extIOR (dielectric.cpp:158);
                                   ROUGHCONDUCTOR: eta/extEta as linear RGB              */
    float    k[3];              /* ROUGHCONDUCTOR: k/extEta as linear RGB                */
    float    alpha_u, alpha_v;  /* ROUGHCONDUCTOR roughness (clamped to >= 1e-4 inside)  */
    uint32_t distribution;      /* phip_microfacet_type                                  */
    uint32_t sample_visible;    /* microfacet.h:144, default true                        */
    uint32_t reflectance_texture; /* 0 = the constant `reflectance`, else 1 + id of a `bitmap` texture on DIFFUSE `reflectance`
                                   (diffuse.cpp:110-150) or on DIELECTRIC / ROUGHCONDUCTOR `specularReflectance`
                                   (dielectric.cpp:300, roughconductor.cpp:297-298,373-374): texture->eval(its)  */
    uint32_t alpha_u_texture, alpha_v_texture;   /* ROUGHCONDUCTOR (ABI 5): 0 = the constants alpha_u / alpha_v, else 1 + id of a `bitmap` texture
                                   given as the child "alpha" (then both ids are equal), "alphaU" or "alphaV" (roughconductor.cpp:424-431);
                                   the roughness at a vertex is texture->eval(its).average() (roughconductor.cpp:275-280), clamped to >= 1e-4
                                   (microfacet.h:113-114).  Two different textures make the BSDF anisotropic (roughconductor.cpp:228-229) */
    uint32_t transmittance_texture; /* DIELECTRIC (ABI 5): 0 or 1 + id of a `bitmap` texture on specularTransmittance (dielectric.cpp:301,348) */
} phip_material;

/* ---- `bitmap` texture (src/textures/bitmap.cpp, Texture2D::eval texture.cpp:112-121): an RGB MIP pyramid exactly as
 * the plugin built and stores it (level 0 = the image; every further level, sizes max(1, (n+1)/2) down to 1x1,
 * mipmap.h:182-192 -- filterType nearest / bilinear: level 0 only).  Lookups without UV partials read level 0
 * bilinearly (bitmap.cpp:431-454); the first path vertex has partials (camera-ray differentials,
 * intersection.cpp:5-76) and uses MIPMap::eval (mipmap.h:629-833). ---- */
typedef enum phip_wrap_mode {     /* = ReconstructionFilter::EBoundaryCondition, value for value (rfilter.h:53-64) */
    PHIP_WRAP_CLAMP = 0, PHIP_WRAP_REPEAT = 1, PHIP_WRAP_MIRROR = 2, PHIP_WRAP_ZERO = 3, PHIP_WRAP_ONE = 4
} phip_wrap_mode;
typedef enum phip_filter_type {   /* EMIPFilterType, mipmap.h:40-52 */
    PHIP_FILTER_NEAREST = 0, PHIP_FILTER_BILINEAR = 1, PHIP_FILTER_TRILINEAR = 2, PHIP_FILTER_EWA = 3
} phip_filter_type;
#define PHIP_MIP_MAX_LEVELS 17
typedef struct phip_texture {
    uint32_t width, height;
    uint32_t n_levels;                    /* 1 or the complete pyramid                     */
    const float *levels[PHIP_MIP_MAX_LEVELS];   /* levels[l]: RGB floats, row-major        */
    uint32_t wrap_u, wrap_v;              /* phip_wrap_mode ('wrapModeU/V', default repeat) */
    uint32_t filter_type;                 /* phip_filter_type ('filterType', default EWA)  */
    float    max_anisotropy;              /* 'maxAnisotropy', default 20                   */
    float    uv_scale[2], uv_offset[2];   /* Texture2D 'uscale/vscale', 'uoffset/voffset'  */
} phip_texture;

/* ---- shapes: every shape is a TriMesh (analytic shapes go through Shape::createTriMesh) ---- */
typedef struct phip_shape {
    uint32_t first_vertex, n_vertices;   /* range in positions[] / normals[]              */
    uint32_t first_triangle, n_triangles;/* range in indices[] (indices are GLOBAL vertex ids) */
    uint32_t material;                   /* id into materials[]                           */
    int32_t  emitter;                    /* id into emitters[] or -1                      */
    uint32_t has_normals;                /* 0: shading normal = face normal (skdtree.h:393)*/
    uint32_t has_texcoords;              /* 1: its.uv from texcoords[], dpdu/dpdv from TriMesh::computeUVTangents (trimesh.cpp:683-735) */
} phip_shape;

/* ---- emitters: `area` (src/emitters/area.cpp) and the `constant` environment (src/emitters/constant.cpp).
 * Emitters are listed in the order of Scene::getEmitters() (the selection PDF of scene.cpp:375-381 depends on
 * it).  At most one environment emitter (scene.cpp:510-513).  The bounding sphere of the constant emitter
 * is derived by the library exactly like ConstantBackgroundEmitter::createShape does (constant.cpp:67-72:
 * 1.5 x the bounding sphere of the kd-tree's box expanded by the sensor position); `envmap` has the same sphere. ---- */
enum { PHIP_EMITTER_AREA = 0, PHIP_EMITTER_CONSTANT = 1, PHIP_EMITTER_ENVMAP = 2 };
typedef struct phip_emitter {
    float    radiance[3];
    float    sampling_weight;            /* Emitter::getSamplingWeight, default 1         */
    uint32_t shape;                      /* area: the parent shape (area.cpp:185-203); constant: ignored */
    uint32_t type;                       /* PHIP_EMITTER_*                                 */
    uint32_t reserved[2];
} phip_emitter;

/* ---- sensor: `perspective` pinhole (src/sensors/perspective.cpp:126-180,271-297) ---- */
typedef struct phip_camera {
    float to_world[16];      /* row-major camera-to-world, no scale (perspective.cpp:116-118)  */
    float xfov_deg;          /* horizontal field of view in degrees (sensor.cpp:244-278 resolved)*/
    float near_clip, far_clip;
    float reserved;
} phip_camera;

/* ---- film + reconstruction filter (films/hdrfilm.cpp, libcore/rfilter.cpp:38-57) ---- */
#define PHIP_FILTER_RESOLUTION 31
typedef struct phip_film {
    int32_t width, height;               /* full film size                                */
    int32_t crop_offset_x, crop_offset_y;
    int32_t crop_width, crop_height;     /* the rendered window; output is crop-sized     */
    float   filter_radius;               /* ReconstructionFilter::getRadius               */
    float   filter_table[PHIP_FILTER_RESOLUTION + 1]; /* m_values[], last entry 0         */
} phip_film;

/* ---- `envmap` (src/emitters/envmap.cpp): latitude-longitude radiance map.  `texels` is MIP level 0 exactly as the
 * reference stores it (MIPMap::getArray(): RGB, already rounded to half precision by the plugin) -- the illumination
 * code reads only that level: sampleDirect / pdfDirect (envmap.cpp:516-632) and evalEnvironment for rays without
 * differentials (envmap.cpp:380-394, MIPMap::evalBilinear, mipmap.h:575-596).  Directly visible background pixels
 * (camera rays carry differentials, envmap.cpp:395-407) use the EWA-filtered lookup of MIPMap::eval (mipmap.h:629-833)
 * over the plugin's MIP pyramid: pass every level as the reference built and stored it (`levels`, sizes halve with
 * max(1, (n+1)/2) down to 1x1, mipmap.h:182-192).  With n_levels <= 1 a render that shows the environment needs
 * hideEmitters (those pixels are then never evaluated, path.cpp:139-141) or PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND. */
#define PHIP_ENVMAP_MAX_LEVELS 17        /* images are smaller than 65536 pixels (envmap.cpp:163-165) */
typedef struct phip_envmap {
    const float *texels;                 /* level 0: height x width x 3 floats (RGB), row 0 = +Y pole; NULL: no envmap */
    uint32_t width, height;
    float    scale;                      /* 'scale' property                               */
    float    to_world[16];               /* row-major emitter-to-world transform ('toWorld') */
    uint32_t n_levels;                   /* 0 / 1: level 0 only; else the complete pyramid  */
    const float *levels[PHIP_ENVMAP_MAX_LEVELS];   /* levels[l], l >= 1: RGB floats of level l ([0] is ignored) */
} phip_envmap;

typedef struct phip_scene_desc {
    uint32_t abi_version;                /* PHIP_ABI_VERSION                              */
    uint32_t n_vertices;
    const float    *positions;           /* 3*n_vertices, world space                     */
    const float    *normals;             /* 3*n_vertices or NULL (then no shape has normals)*/
    uint32_t n_triangles;
    const uint32_t *indices;             /* 3*n_triangles, global vertex ids              */
    uint32_t n_shapes;
    const phip_shape    *shapes;         /* triangle ranges must tile [0,n_triangles) in order */
    uint32_t n_materials;
    const phip_material *materials;
    uint32_t n_emitters;
    const phip_emitter  *emitters;
    phip_camera camera;
    phip_film   film;
    phip_envmap envmap;                  /* used by the emitter of type PHIP_EMITTER_ENVMAP */
    const float *texcoords;              /* 2*n_vertices or NULL (then no shape has texcoords) */
    uint32_t n_textures;
    const phip_texture *textures;
} phip_scene_desc;

/* ---- integrator parameters: MonteCarloIntegrator (src/librender/integrator.cpp:190-225) ---- */
typedef enum phip_sampler_kind {
    PHIP_SAMPLER_CTR = 0     /* counter-based (pixel, sample, dimension) stream -- the parity stream.  `seed` selects the
                                stream: the Mitsuba shim maps the scene's `independent` sampler here (its SFMT stream is
                                a per-worker sequential generator, src/samplers/independent.cpp:71-103, that no parallel
                                schedule can reproduce). */
    , PHIP_SAMPLER_LD = 1    /* (ABI 5) the construction of `ldsampler` (src/samplers/ldsampler.cpp): the first 4 2D requests of a sample
                                (pixel jitter, emitter / BSDF samples of the first vertices) and its first 4 1D requests (Russian
                                roulette) are points of randomly scrambled (0,2)-sequences (core/qmc.h) visited in a random order per
                                pixel and dimension, later requests fall back to the counter stream -- with the scrambles and the
                                order taken from the counter-based generator instead of the worker's sequential Random, so the
                                stream is addressable and reproducible.  The sample count of the whole render (`sample_total`,
                                else `spp`) must be a power of two (ldsampler.cpp:83-87 rounds it up).  `direct`: its sample arrays
                                (direct.cpp:139-146) are one scrambled sequence of sampleCount x N points each, in a random order
                                (ldsampler.cpp:193-197); single shading samples are the sample's next 2D requests. */
    , PHIP_SAMPLER_SOBOL = 2 /* (ABI 6, `path` only) the reference's `sobol` sampler (src/samplers/sobol.cpp): its stream is addressable as it
                                stands -- sample k of pixel (x, y) is point sobol::look_up(m, k, x, y) of the global Sobol' sequence
                                (Gruenschloss' enumeration of elementary intervals, sobolseq.h:94-130), dimension d of that point is
                                sobol::sampleSingle(index, d) (sobolseq.h:42-58), dimensions are consumed in call order (camera sample 0-1,
                                then every 2D request two and every 1D request one; as the plugin stands no 2D request is served from
                                dimension 4, sobol.cpp:241-242 with m_arrayStartDim = m_arrayEndDim = 5: the third 2D request of a sample
                                starts at 5 -- restated for rr_depth >= 2, where the first two requests after the camera sample are 2D;
                                rr_depth 1 is PHIP_ERR_INVALID) -- so the device reproduces it bit for bit, given the
                                plugin's direction numbers as DATA: phip_render_params.sobol_* (the Mitsuba shim reads them out of the
                                loaded plugin, the test harness out of oracle/_ref/plugins/sobol.so or the fixture tests/golden/sobol_tables.npz made from it).
                                Requests beyond sobol_dimensions fall back to the counter stream (the reference stops with an error there).
                                The film's crop window must start at the origin. */
    , PHIP_SAMPLER_STRATIFIED = 3 /* (ABI 6; every integrator since round 5) the construction of `stratified` (src/samplers/stratified.cpp:147-200): the first 4 2D
                                requests of a sample (the pixel jitter is the first) and its first 4 1D requests are jittered points of a
                                res x res (res^2 x 1) grid whose cells the samples of a pixel visit in a random order per dimension, later
                                requests are independent -- with the order a keyed permutation (as PHIP_SAMPLER_LD) and the jitter the
                                counter stream's number for that request, instead of the worker's sequential Random.  The sample count of
                                the render must be a perfect square (stratified.cpp:64-72 rounds it up).  With PHIP_INTEGRATOR_DIRECT a sample array of
                                more than one shading sample per kind is one Latin hypercube over all its entries (stratified.cpp:160-164), single samples
                                are the sample's next 2D requests. */
    , PHIP_SAMPLER_HALTON = 4     /* (ABI 6; `direct` too since round 4) the reference's `halton` sampler as it stands (src/samplers/halton.cpp): sample k of pixel (x, y) is
                                point offset(x mod 128, y mod 128) + stride * k of the Halton sequence (Gruenschloss' enumeration over bases 2 and 3,
                                halton.cpp:244-296: stride = 2^a 3^b, the offset by the Chinese remainder theorem), dimension d is the (scrambled) radical
                                inverse in the d-th prime (qmc.cpp:141-166); dimensions are consumed exactly as by PHIP_SAMPLER_SOBOL (the same bookkeeping,
                                incl. the 2D request that skips dimension 4).  The primes and the digit permutations (Faure's by default, `scramble` = -1;
                                none for 0; pseudorandom ones otherwise) are DATA: phip_render_params.qmc_*. */
    , PHIP_SAMPLER_HAMMERSLEY = 5 /* (ABI 6; `direct` with single shading samples since round 4) the reference's `hammersley` sampler (src/samplers/hammersley.cpp): dimension 0 is index * 1 / (sampleCount
                                resX resY), dimension d > 0 the radical inverse in the (d-1)-th prime, index = offset(x mod 128, y mod 128) + resY * k
                                (hammersley.cpp:181-222); the rest as PHIP_SAMPLER_HALTON.  The sample count is that of the whole render (`sample_total`). */
} phip_sampler_kind;
#define PHIP_SOBOL_MATRIX_SIZE 52    /* words per dimension of sobol::Matrices (sobolseq.h:30) */

/* which SamplingIntegrator::Li the call evaluates */
typedef enum phip_integrator_kind {
    PHIP_INTEGRATOR_PATH = 0,    /* MIPathTracer, src/integrators/path/path.cpp:119-300                                     */
    PHIP_INTEGRATOR_DIRECT = 1,  /* MIDirectIntegrator, src/integrators/direct/direct.cpp:149-312 (max_depth / rr_depth unused) */
    PHIP_INTEGRATOR_VOLPATH_SIMPLE = 2   /* SimpleVolumetricPathTracer on a scene WITHOUT participating media, src/integrators/path/volpath_simple.cpp:88-318: the path tracer
                                            without multiple importance sampling (parameters as PHIP_INTEGRATOR_PATH).  Media are not part of the scene description: the
                                            plugin shim refuses a scene that has any (mitsuba_amd/plugin/volpath_simple_hip.cpp) */
} phip_integrator_kind;

#define PHIP_MAX_DEVICES 16
typedef struct phip_render_params {
    int32_t  spp;                /* sampler sampleCount                                   */
    int32_t  max_depth;          /* -1 = infinite (integrator.cpp:197)                    */
    int32_t  rr_depth;           /* default 5                                             */
    int32_t  strict_normals;     /* default 0                                             */
    int32_t  hide_emitters;      /* default 0                                             */
    int32_t  block_size;         /* Scene::getBlockSize, default 32 (mitsuba.cpp:144)     */
    uint32_t sampler;            /* phip_sampler_kind                                     */
    uint32_t seed;
    /* block sharding: this call renders the blocks whose index in the reference's spiral order
       (imageproc.cpp:43-78) is congruent to shard_index modulo shard_count. 0/1 = whole image. */
    int32_t  shard_index;
    int32_t  shard_count;
    int32_t  device;             /* HIP device ordinal                                    */
    int32_t  flags;              /* PHIP_FLAG_*                                           */
    void    *stream;             /* hipStream_t to launch on, NULL = library-owned stream; must be NULL when n_devices > 1 (PHIP_ERR_INVALID otherwise) */
    uint32_t integrator;         /* phip_integrator_kind                                  */
    int32_t  emitter_samples;    /* `direct`: emitterSamples (direct.cpp:98-99), default 1 */
    int32_t  bsdf_samples;       /* `direct`: bsdfSamples (direct.cpp:100-101), default 1  */
    /* Multi-GPU inside the call (ABI 4).  n_devices <= 1: the scene's device (`device`).  n_devices > 1: the blocks of this
       call's shard are dealt round-robin, in the reference's spiral order, over devices[0..n_devices): one host thread and
       one stream per device, the scene is replicated to a device on first use (phip_scene_replicate does it ahead of time),
       and the per-device (R,G,B,alpha,weight) films are merged on devices[0] with one ncclReduce(sum) (RCCL over xGMI).
       devices[0] must be the scene's device; phip_render_device's buffer lives there.  A device may not be listed twice
       unless PHIP_FLAG_ALIAS_DEVICES is set (test hook for single-GPU boxes: the films are then summed by a kernel). */
    int32_t  n_devices;
    int32_t  devices[PHIP_MAX_DEVICES];
    /* Progressive rendering (ABI 4): this call renders sample indices [sample_offset, sample_offset + spp) of a render of
       sample_total samples per pixel (0 = spp; only the camera-ray differential scale 1/sqrt(sampleCount),
       integrator.cpp:144-145, depends on it); with PHIP_FLAG_ACCUMULATE the result is ADDED to the film left by the
       previous call (phip_render: the library-owned film; phip_render_device: the caller's buffer). */
    int32_t  sample_offset;
    int32_t  sample_total;
    /* Progress (ABI 4): called whenever the job's live-path count is polled (about every 8 wavefront iterations) and at the
       end, with the camera samples finished so far by that device.  With n_devices > 1 the calls come from the library's
       per-device host threads -- never two at a time (they are serialised), but not on the caller's thread.
       May be NULL.  The callback may call phip_cancel. */
    void   (*progress)(void *user, int32_t device, uint64_t samples_done, uint64_t samples_total);
    void    *progress_user;
    /* PHIP_SAMPLER_SOBOL (ABI 6): host pointers, read during the call.  sobol_matrices = sobol::Matrices::matrices32, sobol_dimensions x 52
       words; sobol_vdc / sobol_vdc_inv = rows [m - 1] of sobol::Matrices::vdc_sobol_matrices / _inv (52 words each), m = sobol_log_resolution =
       log2 of the larger side of the crop window rounded up to a power of two (SobolSampler::setFilmResolution, sobol.cpp:147-157; m <= 1:
       no per-pixel enumeration, the tables may be NULL); sobol_scramble = the sampler's m_scramble (0 unless the scene sets `scramble`: then sampleTEA of it, sobol.cpp:92-102). */
    const uint32_t *sobol_matrices;
    const uint64_t *sobol_vdc;
    const uint64_t *sobol_vdc_inv;
    uint32_t sobol_dimensions;
    uint32_t sobol_log_resolution;
    uint64_t sobol_scramble;
    /* PHIP_SAMPLER_HALTON / _HAMMERSLEY (ABI 6): host pointers, read during the call.  qmc_primes = the first qmc_dimensions entries of the
       reference's primeTable (qmc.cpp:27-81); qmc_permutations = the digit permutations of its PermutationStorage (src/samplers/faure.cpp)
       for those bases, concatenated -- the one of dimension d starts at primes[0] + ... + primes[d - 1] -- or NULL for `scramble` = 0. */
    const uint32_t *qmc_primes;
    const uint16_t *qmc_permutations;
    uint32_t qmc_dimensions;
    uint32_t qmc_reserved;
} phip_render_params;

#define PHIP_FLAG_KERNEL_TIMING 1   /* bracket the kernels with hipEvents, fill phip_stats.*_ms */
#define PHIP_FLAG_SAMPLE_BUFFER 2   /* keep per-sample radiance for phip_get_samples (tests)    */
#define PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND 4   /* directly visible envmap pixels: unfiltered level-0 lookup instead of the reference's EWA filter (deviation!) */
#define PHIP_FLAG_ACCUMULATE 8      /* add to the film of the previous call instead of overwriting it (progressive rendering) */
#define PHIP_FLAG_ALIAS_DEVICES 16  /* devices[] may name one GPU several times (exercises the multi-device path on a 1-GPU box) */
#define PHIP_FLAG_NO_FUSED 32       /* never use the fused single-kernel path (k_mega) nor the one-kernel iterations (k_shade_trace, k_shade_trace_w) -- A/B and parity tests of the wavefront kernels on small scenes */
#define PHIP_FLAG_NO_MEGA 64        /* not k_mega, but the one-kernel iterations where the scene admits them: k_shade_trace on a small scene (with glass / copper it runs k_mega since round 5:
                                       how the tests still reach k_shade_trace on it), k_shade_trace_w on a scene k_mega serves on the 8-wide tree in memory (fused_traversal 4 / 5; where that kernel is on: PHIP_FLAG_FUSED_ANY).  The
                                       kernels' own clients are scenes with textures or an environment emitter */
#define PHIP_FLAG_FUSED_ANY 128     /* the fused kernel on EVERY scene it admits (round 6: k_mega walks the 8-wide tree from memory, phip_accel_info.fused_traversal 4 / 5) -- by default
                                       only trees of at most PHIP_FUSED_WIDE_MAX_NODES wide nodes run it, the wavefront kernels are faster beyond; parity tests and A/B.
                                       Likewise the one-kernel iterations on the 8-wide tree (k_shade_trace_w: every scene past the packed leaf table that k_mega did not take,
                                       textures / an environment emitter included; `path` and `volpath_simple`): by default on trees of at most
                                       PHIP_SHADE_TRACE_WIDE_MAX_NODES wide nodes, with this flag on every tree */
#define PHIP_FUSED_WIDE_MAX_NODES 4096
#define PHIP_SHADE_TRACE_WIDE_MAX_NODES 0   /* measured: at no tree size is k_shade_trace_w ahead of k_shade + k_rays_w by more than the step spread -- PHIP_FLAG_FUSED_ANY only */

typedef struct phip_stats {
    uint64_t samples;                /* camera samples rendered by this call                  */
    uint64_t closest_rays;           /* "Normal rays traced" (skdtree.cpp:46)                 */
    uint64_t shadow_rays;            /* "Shadow rays traced" (skdtree.cpp:47)                 */
    uint64_t path_vertices;          /* sum of path depths, "Average path length" (path.cpp:24)*/
    uint64_t closest_node_visits;    /* accel nodes fetched by closest-hit queries            */
    uint64_t closest_triangle_tests; /* TriAccel tests by closest-hit queries                 */
    uint64_t shadow_node_visits;     /* same for any-hit (shadow) queries                     */
    uint64_t shadow_triangle_tests;
    uint64_t invalid_samples;        /* rejected by the ImageBlock::put validity check        */
    uint32_t iterations;             /* wavefront iterations = launches of each kernel        */
    uint32_t vertex_traced;          /* 1: the iterations ran k_shade_trace / k_shade_trace_w -- vertex, shadow ray and next ray of a slot in ONE kernel per iteration (scenes
                                        that are not k_mega's: <= 64 Wald records with any material; a scene on the 8-wide tree under PHIP_FLAG_FUSED_ANY, or with a tree of at most
                                        PHIP_SHADE_TRACE_WIDE_MAX_NODES wide nodes); trace / shadow ms are then 0.  0 for a job that gave such a pass up and went on with the wavefront
                                        kernels.  (`reserved`, always 0, before round 5) */
    double   render_ms;              /* host wall clock of the call                           */
    double   trace_kernel_ms;        /* sum of HIP-event durations of the closest-hit kernel  */
    double   shadow_kernel_ms;       /* ... of the any-hit kernel                             */
    double   shade_kernel_ms;
    double   film_kernel_ms;
    double   algorithmic_bytes;      /* SURVEY 8(d) bytes of the whole call, from the counters */
    double   trace_kernel_bytes;     /* the closest-hit kernel's share: node + triangle + ray + hit bytes */
    double   fused_kernel_ms;        /* ... of k_mega (scenes that fit LDS: the whole path in one kernel) */
    double   reduce_ms;              /* multi-device: ncclReduce of the films + its synchronisation, host wall clock */
    uint32_t fused;                  /* 1: the call ran the fused kernel for the whole frame, on every device (then trace/shadow/shade ms are 0); 0 when any pass was rendered again on the wavefront kernels */
    uint32_t n_devices;              /* devices that rendered (counters are summed over them, *_ms are the maximum) */
    double   d2h_ms;                 /* (ABI 7) phip_render: the film's device-to-host copy, host wall clock; included in render_ms */
} phip_stats;

typedef struct phip_ray  { float o[3]; float mint; float d[3]; float maxt; } phip_ray;
typedef struct phip_hit  { float t, u, v; uint32_t prim; /* global triangle id, 0xFFFFFFFF = miss */ } phip_hit;
#define PHIP_NO_HIT 0xFFFFFFFFu

typedef struct phip_scene phip_scene;   /* opaque */

/* number of HIP devices visible, or a negative phip_status */
int          phip_device_count(void);
const char  *phip_last_error(void);
const char  *phip_version(void);
const char  *phip_build_id(void);         /* hash of the sources + flags the library was built from (mitsuba_amd/_ffi.py: source_id); "unknown-build-id" outside the in-tree build */

/* Flattens the scene, builds the acceleration structure on the host and uploads it to `device`. */
phip_scene  *phip_scene_create(const phip_scene_desc *desc, int device);
void         phip_scene_destroy(phip_scene *scene);

/* Renders the crop window; out_rgbaw = crop_h*crop_w*5 float32 (R,G,B,alpha,weight) on the HOST,
   accumulated filter-weighted sums exactly like the film's ESpectrumAlphaWeight bitmap.
   out_rgbaw may be any host memory.  Pinned memory (phip_host_alloc, hipHostMalloc, a registered range) receives the film in one
   asynchronous copy at the link's rate; pageable memory receives it in chunks through the library's pinned staging buffers. */
int  phip_render(phip_scene *scene, const phip_render_params *params,
                 float *out_rgbaw, phip_stats *out_stats);

/* Same, but d_out_rgbaw is DEVICE memory on params->device (e.g. a torch tensor's data_ptr());
   the buffer is overwritten.  Completion is synchronous on return. */
int  phip_render_device(phip_scene *scene, const phip_render_params *params,
                        void *d_out_rgbaw, phip_stats *out_stats);

/* (ABI 7) A device-resident frame of this scene's crop size -- phip_render_device's output, e.g. after the caller's own RCCL reduce of
   per-process films (bench.py --gpus N under torchrun) -- to host memory, the way phip_render delivers it: one asynchronous copy into pinned
   memory, staged chunks into pageable memory.  The reference's analogue is the master's film->put (src/librender/renderproc.cpp:142-149). */
int  phip_film_to_host(phip_scene *scene, const void *d_rgbaw, float *out_rgbaw);

/* Per-sample radiance of the last render with PHIP_FLAG_SAMPLE_BUFFER: n = crop_w*crop_h*spp
   entries of (R,G,B,alpha) ordered [y][x][sample].  Test/diagnostic hook. */
int  phip_get_samples(phip_scene *scene, float *out_rgba, size_t n_samples);

/* Ray-cast entry (the reference's kdbench / test_kd workload): closest hit into hits[],
   and/or any-hit into occluded[] (either may be NULL).  Host pointers. */
int  phip_trace(phip_scene *scene, const phip_ray *rays, size_t n,
                phip_hit *hits, uint8_t *occluded, phip_stats *out_stats);

/* The surface at a hit: what fillIntersectionRecord (include/mitsuba/render/skdtree.h:343-428) gives the integrators, for callers that use the scene's tree
   for something else than its integrators (a depth sensor, visibility queries, their own feature buffers).  64 bytes. */
typedef struct phip_surface {
    float p[3];  float t;               /* the hit point as shading computes it (the barycentric sum of the vertices, not o + t d), the ray distance */
    float ng[3]; uint32_t prim;         /* geometric normal (flipped towards the shading normal on meshes with vertex normals, as the record has it);
                                           PHIP_NO_HIT: a miss, every other field 0 */
    float ns[3]; uint32_t flags;        /* shading normal (the shading frame's n); PHIP_SURFACE_BACK: the ray arrived on the back (wi.z <= 0, wi as skdtree.h:427) */
    float uv[2];                        /* texture coordinates; (u, v) of the hit on a mesh without them (skdtree.h:404) */
    uint32_t material;                  /* the leaf BSDF on the side of arrival: the shape's material, or the nested id a `twosided` adapter shows that side */
    int32_t  emitter;                   /* id into emitters[] of the area emitter the triangle belongs to, or -1 */
} phip_surface;
#define PHIP_SURFACE_BACK 1u

/* phip_trace on DEVICE memory, ordered on the caller's stream, with the surface records: the ray cast of a loop that stays on the GPU (a torch producer writes
   the rays, phip_scene_update / phip_scene_rebuild move the scene, the hits stay in tensors).  Every pointer is device memory of the scene's device and -- d_occluded
   excepted -- 16-byte aligned; a host pointer, another device's pointer or a misaligned one is PHIP_ERR_INVALID.  d_hits, d_occluded and d_surfaces may each be NULL;
   d_surfaces needs d_hits (PHIP_ERR_INVALID without).  n == 0 returns PHIP_OK and touches nothing; n is at most 2^32 - 256 rays per call (PHIP_ERR_INVALID beyond).
   `stream` is the hipStream_t the caller's producer ran on, or NULL: the work is ordered after it; completion is synchronous on return, as for phip_render_device.
   The hits are phip_trace's on the same rays, bit for bit (the closest hit does not depend on the structure or the order of the tests); out_stats fills the fields
   phip_trace fills (the node-visit and triangle-test counters are those of this kernel's order of work; closest_rays / shadow_rays are counted by the kernel),
   render_ms, and in shade_kernel_ms the HIP-event time of the surface records' kernel.
   Rays are not validated and must be finite: they are clipped by the arithmetic phip_trace clips them with, so a non-finite ray gets what it gets there.
   The call takes the scene's render lock.  Its buffers -- the stack overflow region of the persistent grid, the work counters, the per-wave statistics -- are the
   scene's and are sized by the grid, not by n: after the first call no call allocates, and there is no chunking. */
int  phip_trace_device(phip_scene *scene, const phip_ray *d_rays, size_t n,
                       phip_hit *d_hits, uint8_t *d_occluded, phip_surface *d_surfaces,
                       void *stream, phip_stats *out_stats);

/* Path-traced radiance along a caller's rays in DEVICE memory: SamplingIntegrator::Li(ray, rRec) (include/mitsuba/render/integrator.h) as an entry point, for callers
   whose sensor is their own code -- an orthographic, thin-lens or spherical camera, an irradiance meter, a light-probe or lightmap bake written as torch code over
   this call.  phip_render_device serves the one sensor the library knows, the `perspective` pinhole through the film.
     Samples.  For ray i and k in [0, spp) one evaluation of the integrator's Li starts with the caller's ray -- its o, d, mint and maxt --, clipped to the scene with
       the arithmetic the camera ray is clipped with.
     Stream.  The random numbers are the PHIP_SAMPLER_CTR stream of (pixel = the ray's stream key, sample = sample_offset + k, seed), consumed exactly as phip_render
       consumes them for a camera sample; the two numbers of the pixel jitter are drawn and not used.  The key of ray i is d_stream[i], or first_stream + i.
     Read from params: spp, max_depth, rr_depth, strict_normals, hide_emitters, seed, sample_offset, sample_total, stream, device (n_devices = 1: devices[0]),
       integrator, PHIP_FLAG_KERNEL_TIMING.  Ignored: what concerns the film -- shards, block size, the progress callback (its totals are the film's),
       PHIP_FLAG_ENVMAP_BILINEAR_BACKGROUND, the flags that choose a fused kernel.  Refused, PHIP_ERR_INVALID: PHIP_FLAG_SAMPLE_BUFFER, PHIP_FLAG_ACCUMULATE.
     Differentials.  The caller's ray has none: a bitmap texture at the first vertex and a directly visible environment map are read the way later vertices read
       them, level 0 and bilinear (phip_bsdf_device reads textured parameters the same way: bsdfTextures without partials).  This is the one difference from a camera ray; on a scene without textures and without an envmap there is none, and sample k of a
       ray equals sample k of the pixel whose camera ray it is and whose index (y * crop_width + x) is its key, bit for bit (PHIP_FLAG_SAMPLE_BUFFER, phip_get_samples).
     Output.  d_out[i].rgb is the float64 sum of the spp float32 sample values, in ascending k, divided by spp and rounded once to float32; d_out[i].alpha the same mean
       of the samples' alpha, 1 where the caller's ray hit and 0 where it did not.  A non-finite or negative sample is counted in invalid_samples and contributes
       zero, as the film would reject it.
     Served: PHIP_INTEGRATOR_PATH and PHIP_INTEGRATOR_VOLPATH_SIMPLE with PHIP_SAMPLER_CTR.  PHIP_ERR_UNSUPPORTED: PHIP_INTEGRATOR_DIRECT and the other samplers, whose
       streams are addressed by film coordinates.  PHIP_ERR_INVALID: n_devices > 1, a host pointer, another device's pointer, a misaligned pointer, d_rays or d_out
       NULL, n > 2^32 - 256, and what phip_render refuses of the parameters above.  n == 0 returns PHIP_OK and touches nothing.  Rays are not validated and must be finite.
     Ordering and locking, as for phip_trace_device: the work is ordered after params->stream, completion is synchronous on return, the call takes the scene's render
       lock; phip_cancel ends it with PHIP_ERR_CANCELLED and d_out unspecified.
     Stats: samples, the ray and vertex counters, invalid_samples, iterations, render_ms, and under PHIP_FLAG_KERNEL_TIMING trace / shade_kernel_ms and, in
       film_kernel_ms, the time of the kernel that writes d_out.
   There is no fused path: the call runs the wavefront kernels, as a render with PHIP_FLAG_NO_FUSED does.  Its buffers are the scene's and are kept between calls; a
   call whose spp does not fit one pass (PHIP_MAX_PASS_SAMPLES, as for renders) splits spp over passes and keeps 32 bytes per ray of running sums, so that buffer, like
   the 16 bytes per sample of a pass, grows with n.
     Pairs (stream_layout = PHIP_RADIANCE_STREAM_PAIRS).  d_stream holds n pairs (key, sample) instead of n keys: sample k of ray i draws the stream of
       (pixel = key, sample = sample + k), so the rays of one call need not share a sample index -- the camera samples of a whole render, as
       phip_camera_rays_device writes them (d_rays, d_keys), are ONE call at spp = 1 instead of one call per sample.  d_stream must then not be NULL and is 8-byte
       aligned, and params->sample_offset must be 0 (the index is the pair's): PHIP_ERR_INVALID otherwise, and for a layout other than 0 and 1. */
typedef struct phip_radiance_desc {
    const phip_ray *d_rays;      /* n rays, device memory of the scene's device, 16-byte aligned; finite, not validated */
    size_t          n;
    const uint32_t *d_stream;    /* NULL, or n stream keys: ray i draws the counter stream of "pixel" d_stream[i]; NULL = first_stream + i.  stream_layout 1: n pairs (key, sample) */
    uint32_t        first_stream;
    uint32_t        stream_layout; /* 0: d_stream holds keys; PHIP_RADIANCE_STREAM_PAIRS: pairs (was `reserved`, always 0: same layout) */
    float          *d_out;       /* n x (R, G, B, alpha) float32, device, 16-byte aligned */
} phip_radiance_desc;
#define PHIP_RADIANCE_STREAM_PAIRS 1u
int  phip_radiance_device(phip_scene *scene, const phip_render_params *params, const phip_radiance_desc *desc, phip_stats *out_stats /* may be NULL */);

/* The sensor as an entry point: the camera samples phip_render traces, written to DEVICE memory -- for callers that trace or shade them themselves
   (phip_trace_device, phip_radiance_device) and put the results on the film with phip_film_device.  PHIP_SAMPLER_CTR only (PHIP_ERR_UNSUPPORTED for the others,
   whose streams are addressed by film coordinates).
     Samples.  Pixel i of the list (d_pixels[i], or i itself when d_pixels is NULL: every pixel of the crop window, row-major) and k in [0, spp): entry i * spp + k
       is sample sample_offset + k of that pixel.  Its position on the film is (float32(x) + jx, float32(y) + jy) in crop coordinates, (jx, jy) the first two numbers
       of block 0 of the counter stream of (pixel, sample, seed); its ray is the `perspective` camera's through that position, as the render generates it before it
       clips it to the scene (phip_trace_device and phip_radiance_device clip a caller's ray with the same arithmetic).
     Read from params: spp, sample_offset, seed, sampler, stream, device (n_devices = 1: devices[0]).
     PHIP_ERR_INVALID: n_devices > 1, spp <= 0, a negative sample_offset, d_rays NULL, a host pointer, another device's pointer, a misaligned pointer, more than
       2^32 - 256 samples, an entry of d_pixels that is not below crop_w * crop_h (the list is checked on the device before anything is written: after a refusal
       the output buffers are untouched).  An empty list (d_pixels set, m == 0) returns PHIP_OK and touches nothing.
     Ordering and locking, as for phip_trace_device: the work is ordered after params->stream, completion is synchronous on return, the call takes the scene's
       render lock. */
typedef struct phip_camera_rays_desc {
    const uint32_t *d_pixels;   /* NULL: every pixel of the crop window, row-major; else m crop-pixel indices (y * crop_width + x), each < crop_w * crop_h */
    size_t          m;          /* number of pixels (ignored when d_pixels is NULL) */
    phip_ray       *d_rays;     /* m * spp rays, entry (i * spp + k): pixel i, sample sample_offset + k; 16-byte aligned */
    uint32_t       *d_keys;     /* NULL, or m * spp pairs (stream key = the pixel index, sample index = sample_offset + k); 8-byte aligned */
    float          *d_positions;/* NULL, or m * spp pairs: the sample's position on the film in crop coordinates, float32(x) + jitter; 8-byte aligned */
} phip_camera_rays_desc;
int  phip_camera_rays_device(phip_scene *scene, const phip_render_params *params, const phip_camera_rays_desc *desc);

/* ImageBlock::put (include/mitsuba/render/imageblock.h:124-204) on a caller's per-sample values: d_out is the film phip_render_device would leave if sample
   sample_offset + k of crop pixel (x, y) had carried d_values[y][x][k] -- the sample positions are derived again from the counter stream (not passed in), the
   render blocks' bitmaps, their border, the clipped footprints and the filter table's look-up are the render's.  With phip_camera_rays_device and phip_trace_device
   this is a filtered normal, depth or albedo buffer; with phip_radiance_device or the caller's own integrator, a render in parts.  PHIP_SAMPLER_CTR only.
     Read from params: spp, sample_offset, seed, block_size, sampler, stream, device (n_devices = 1: devices[0]), PHIP_FLAG_ACCUMULATE (the sums are added to what
       d_out holds), PHIP_FLAG_KERNEL_TIMING.
     Validity.  flags = 0: a sample of which a value is not finite or negative is rejected whole and counted in invalid_samples, as the film rejects it;
       PHIP_FILM_SIGNED: only a non-finite one is (normals, signed fields).
     Deterministic: one lane per film pixel gathers the samples that reach it in a fixed order -- no float atomics, any filter radius, any spp, and no pass limit
       (the buffer is the caller's).
     PHIP_ERR_INVALID: shard_count > 1, n_devices > 1, spp <= 0, a negative sample_offset, a block size phip_render refuses, d_values or d_out NULL, not device
       memory of the scene's device or not 16-byte aligned, an unknown flag.  Nothing is written after a refusal.
     Stats: samples, invalid_samples, render_ms and -- under PHIP_FLAG_KERNEL_TIMING -- film_kernel_ms.  Ordering and locking as above. */
typedef struct phip_film_desc {
    const float *d_values;   /* crop_h * crop_w * spp x 4 float32, order [y][x][k] (phip_camera_rays_device's order with d_pixels NULL); 16-byte aligned */
    float       *d_out;      /* crop_h * crop_w x 5: the four filtered sums and the weight, phip_render_device's layout; 16-byte aligned */
    uint32_t     flags;      /* PHIP_FILM_SIGNED: reject only non-finite samples; 0: the film's own check (non-finite or negative) */
    uint32_t     reserved;
} phip_film_desc;
#define PHIP_FILM_SIGNED 1u
int  phip_film_device(phip_scene *scene, const phip_render_params *params, const phip_film_desc *desc, phip_stats *out_stats /* may be NULL */);

/* Shading in parts: what an integrator does between two ray casts, on DEVICE memory -- for the caller's own integrator over phip_camera_rays_device,
   phip_trace_device and phip_film_device (ambient occlusion, a direct-lighting variant, path guiding, a learned sampler, the caller's own multiple importance
   sampling).  The three calls are the reference's public interfaces: BSDF::eval / pdf / sample; Scene::sampleEmitterDirect without its visibility test;
   Intersection::Le / Scene::evalEnvironment with Scene::pdfEmitterDirect.  Their arithmetic is the path integrator's own -- the device functions its vertex calls,
   compiled with the product's flags -- so a value equals the one a render computes from the same inputs, bit for bit.
     Conventions, those of phip_trace_device: every pointer is device memory of the scene's device and 16-byte aligned, arrays of 2 floats 8-byte aligned; a host
       pointer, another device's pointer or a misaligned one is PHIP_ERR_INVALID and nothing is written.  n == 0 returns PHIP_OK and touches nothing; n is at most
       2^32 - 256 (PHIP_ERR_INVALID beyond).  `stream` is the caller's hipStream_t or NULL: the work is ordered after it, completion is synchronous on return.
       The calls take the scene's render lock and allocate nothing: inputs and outputs are the caller's.  Inputs are not validated for finiteness.
       PHIP_ERR_INVALID for a NULL scene, a NULL desc or a NULL required pointer; PHIP_ERR_DEVICE without a GPU: there is no CPU fallback.  The message
       (phip_last_error) starts with the function's name.  There are no render parameters, hence no n_devices: the scene's first device serves. */

/* BSDF::eval / pdf / sample at the hits of a ray cast: d_rays and d_hits are what phip_trace_device read and wrote; wi is the shading frame's toLocal(-d).
     Textures.  Textured parameters are read as later path vertices read them -- level 0, no UV partials -- the sentence of phip_radiance_device's "Differentials";
       on a mesh without texture coordinates the coordinates are the hit's (u, v), as in phip_surface.uv.
     Two-sided.  A `twosided` adapter is resolved by the side of arrival: its second nested model serves wi.z < 0 (phip_surface.material names the model).
     A miss (prim == PHIP_NO_HIT; also a primitive index the scene does not have) writes zeros to every output asked for.
     The integrator's strictNormals test is the integrator's and is not applied: phip_surface.ng is there for the caller's own.
     PHIP_ERR_INVALID beside the conventions': no output asked for, d_eval without d_wo, d_sampled without d_samples, a flag other than PHIP_BSDF_LOCAL. */
typedef struct phip_bsdf_sample {
    float wo[3]; float pdf;            /* the sampled direction (world space; PHIP_BSDF_LOCAL: shading frame) and its density: solid angle, or discrete for a delta component */
    float weight[3]; float eta;        /* value / pdf, cosine included, as BSDF::sample returns it; the relative index of refraction along the sampled direction (1: no refraction) */
    uint32_t flags;                    /* PHIP_BSDF_SAMPLED_VALID | PHIP_BSDF_SAMPLED_DELTA */
    uint32_t reserved[3];              /* 0 */
} phip_bsdf_sample;                    /* 48 bytes; a failed sample (weight zero) is all zero */
#define PHIP_BSDF_SAMPLED_DELTA 1u
#define PHIP_BSDF_SAMPLED_VALID 2u
#define PHIP_BSDF_LOCAL 1u             /* phip_bsdf_desc.flags: d_wo is read, and phip_bsdf_sample.wo written, in the shading frame instead of world space */
typedef struct phip_bsdf_desc {
    const phip_ray *d_rays;            /* n rays: their directions are read */
    const phip_hit *d_hits;            /* n hits of those rays */
    size_t          n;
    const float    *d_wo;              /* NULL, or n x float4: xyz = the outgoing direction (w is not read) */
    const float    *d_samples;         /* NULL, or n x float2 in [0, 1) */
    float          *d_eval;            /* NULL, or n x float4: rgb = BSDF::eval in the solid-angle measure, cosine included; w = BSDF::pdf.  Needs d_wo */
    phip_bsdf_sample *d_sampled;       /* NULL, or n records.  Needs d_samples */
    float          *d_wi_local;        /* NULL, or n x float4: wi in the shading frame, w = 0 */
    uint32_t        flags;             /* PHIP_BSDF_LOCAL or 0 */
    uint32_t        reserved;
    void           *stream;
} phip_bsdf_desc;
int  phip_bsdf_device(phip_scene *scene, const phip_bsdf_desc *desc);

/* Scene::sampleEmitterDirect(dRec, sample, testVisibility = false): one emitter sample per reference point.  An environment emitter (`constant`, `envmap`) is
   served; a scene without emitters writes "no sample" everywhere.  Visibility is the caller's next phip_trace_device call with d_occluded on d_shadow_rays: this
   call traces nothing. */
typedef struct phip_emitter_sample {
    float d[3]; float dist;            /* unit direction from the reference point to the sampled position, and the distance */
    float value[3]; float pdf;         /* radiance / pdf, the emitter selection probability included: sampleEmitterDirect's return; pdf: solid-angle density times that probability */
    int32_t emitter;                   /* id into emitters[], or -1: no sample (pdf == 0), every other field 0 */
    uint32_t reserved[3];
} phip_emitter_sample;                 /* 48 bytes */
typedef struct phip_emitter_sample_desc {
    const float *d_ref;                /* n x float4: xyz = the reference point */
    const float *d_ref_n;              /* NULL, or n x float4: xyz = the normal at the reference point.  NULL is the zero normal of a point that lies on no surface
                                          (DirectSamplingRecord::refN); the path integrator passes zero too at a transmissive or two-sided-transmissive surface */
    const float *d_samples;            /* n x float2 in [0, 1) */
    size_t       n;
    phip_emitter_sample *d_sampled;    /* n records */
    phip_ray    *d_shadow_rays;        /* NULL, or n rays: the shadow ray the `path` integrator traces for the sample -- o = the reference point, mint = Epsilon (scaled by
                                          the origin's magnitude when it is traced, as every ray's), d, maxt = dist * (1 - ShadowEpsilon).  An entry without a sample is
                                          the empty interval mint = 0, maxt = -1, for which phip_trace_device answers "not occluded" without traversing */
    void        *stream;
} phip_emitter_sample_desc;
int  phip_emitter_sample_device(phip_scene *scene, const phip_emitter_sample_desc *desc);

/* The emitted radiance a ray meets and the density with which emitter sampling would have produced it: the other half of multiple importance sampling
   (path.cpp, the block behind bsdf->sample).  At a hit on an area emitter rgb = its.Le(-d), zero on the back; at a miss in a scene with an environment emitter rgb =
   evalEnvironment for a ray without differentials (the lookup later vertices use); otherwise rgb = 0.  w = Scene::pdfEmitterDirect for that record in the solid-angle
   measure, the selection probability included, and 0 where rgb comes from no emitter -- also at a miss whose origin lies outside the environment emitter's sphere
   (its fillDirectSamplingRecord refuses the ray; the integrator adds nothing there). */
typedef struct phip_emitter_eval_desc {
    const phip_ray *d_rays;            /* n rays: origin and direction are read */
    const phip_hit *d_hits;            /* n hits of those rays */
    const float    *d_ref_n;           /* NULL (zero normals), or n x float4: the normal at the ray's origin; enters only through dot(d, refN) and refN.isZero() */
    size_t          n;
    float          *d_eval;            /* n x float4 */
    int32_t        *d_emitter;         /* NULL, or n x int32: the emitter's id, or -1 */
    void           *stream;
} phip_emitter_eval_desc;
int  phip_emitter_eval_device(phip_scene *scene, const phip_emitter_eval_desc *desc);

/* Replicates the device-resident scene (geometry, acceleration structure, materials, textures) from the scene's device
   to each listed device (device-to-device copies over xGMI), so that a later multi-device render starts immediately. */
int  phip_scene_replicate(phip_scene *scene, const int32_t *devices, int32_t n_devices);

/* New vertex positions, vertex normals and / or camera for the scene as created: a REFIT of its acceleration structure, not a rebuild (a fly-through, a deforming
   mesh).  After the call every entry point behaves exactly as if the scene had been created from the original descriptor with these positions, normals and camera:
   per-sample radiance, film and the counters samples / closest_rays / shadow_rays / path_vertices / invalid_samples are the same bits (node-visit and triangle-test
   counters, sah_cost and timings may differ: the refitted boxes are conservative, not the builder's).  The topology is the creation's -- indices, shapes, materials,
   emitters, textures, film and crop window; node, record and leaf counts --, so fits_lds, fused_traversal and the kernels a render resolves do not change.
   The call takes the scene's render lock (it serialises with renders), validates before it writes -- on any error the scene is unchanged -- and drops the replicas
   on other devices, which the next multi-device render copies again.  Errors: PHIP_ERR_INVALID for a non-finite position, normal or camera transform, normals for a
   scene created without them, an area emitter whose mesh has no area left, device_pointers = 1 with memory that is not the scene's device's; PHIP_ERR_UNSUPPORTED
   (the count in phip_last_error) when a triangle that was degenerate at creation -- it got no Wald record -- is not degenerate now: a fresh build would give it a
   record, a refit cannot.  The converse is served: a triangle that collapses gets the never-hit record and comes back with a later update.  PHIP_ERR_DEVICE without
   a GPU: there is no CPU fallback.  How much slower a refitted tree traverses than a fresh one depends on how far the vertices went (DESIGN.md 3.12 has
   measurements); the library fixes no threshold -- sah_cost is there for the caller to decide when to call phip_scene_rebuild (below), which builds a new tree on
   the device in place of destroying the scene and creating it again. */
typedef struct phip_update_desc {
    const float *positions;      /* 3 * n_vertices of the scene as created, world space; NULL = unchanged */
    const float *normals;        /* 3 * n_vertices; NULL = unchanged; PHIP_ERR_INVALID if the scene was created without normals */
    const phip_camera *camera;   /* NULL = unchanged (film and crop window never change) */
    uint32_t device_pointers;    /* 0: positions / normals are host memory; 1: device memory on the scene's device (a torch tensor's data_ptr()) */
    void *stream;                /* device_pointers = 1: the hipStream_t the caller's producer ran on, or NULL; the update is ordered after it */
} phip_update_desc;
typedef struct phip_update_info {
    double update_ms;            /* host wall clock of the call */
    double kernel_ms;            /* HIP-event time of the device work */
    float  sah_cost;             /* buildWide's cost formula on the refitted boxes; phip_scene_accel_info reports the same value from now on */
    uint32_t n_degenerate;       /* triangles whose Wald record is the never-hit record after this update */
} phip_update_info;
int  phip_scene_update(phip_scene *scene, const phip_update_desc *update, phip_update_info *out_info /* may be NULL */);

/* phip_scene_update with a NEW topology of the 8-wide tree, built on the device from the positions where they are: the remedy for a tree that a
   refit has made slow (the builder's spatial splits on scenes of 4096 triangles or more do not survive moving vertices), without the host builder and without
   uploading materials, textures and the environment map again.  The same sentence holds after the call, with the same list of bits: every entry point behaves as if
   the scene had been created from the original descriptor with these positions, normals and camera.  What differs from phip_scene_update:
     * n_nodes, max_depth, n_leaves and n_triangle_refs of phip_scene_accel_info may change (the new tree has one record per non-degenerate triangle and no split
       references), sah_cost is buildWide's formula on the new tree, and what the creation derives from those counts -- the node cache, fused_traversal with the
       PHIP_FUSED_WIDE_MAX_NODES gate -- is derived again;
     * a triangle that was degenerate at creation and is not degenerate now gets its record: no PHIP_ERR_UNSUPPORTED for it, and later phip_scene_update calls start
       from the new state.  n_degenerate is 0: a degenerate triangle has no record in the new tree;
     * one refusal of its own, PHIP_ERR_UNSUPPORTED: the new tree is deeper than the traversal stacks allow (52 levels).  The tree is a radix tree over 30-bit Morton
       keys, so it has at most 31 + ceil(log2 m) levels, m being the largest number of triangles whose centres share one cell of a 1024^3 grid over the scene box:
       the refusal needs more than two million triangles in one cell.
   update may be NULL (or all-zero): the scene's current vertices and camera, e.g. after a series of phip_scene_update calls.  Locking, validation before anything is
   written (on any error the scene is unchanged: the call builds into fresh buffers and swaps them in at the end), the dropped replicas and the other error codes are
   phip_scene_update's.  A scene that is not on the 8-wide tree alone -- at most 64 Wald records: it has the packed leaf table, no split references, nothing to
   gain -- is served by phip_scene_update itself, with that call's refusals (the degenerate-at-creation triangle included) and its unchanged counts. */
int  phip_scene_rebuild(phip_scene *scene, const phip_update_desc *update /* may be NULL */, phip_update_info *out_info /* may be NULL */);

/* New materials, emitter radiances and sampling weights, texture contents and sampling settings and / or a new environment map for the scene as created: what a
   surface or a light LOOKS like, in place (dimming a lamp, turning a wall to glass, an animated sky, a video texture) -- without the host builder, without
   uploading the geometry again.  After the call every entry point behaves exactly as if the scene had been created from the original descriptor with these
   materials, emitters, textures and environment map -- on top of whatever phip_scene_update and phip_scene_rebuild have done to vertices and camera so far:
   per-sample radiance, film, the counters samples / closest_rays / shadow_rays / path_vertices / invalid_samples and phip_surface.material are the same bits.
   What stays fixed: every count, the shape -> material and shape -> emitter assignment, emitter types, texture and environment-map sizes and level counts, the
   film, the tree (phip_scene_accel_info does not change but for nothing).  Material TYPES may change, what `twosided` adapters nest included: the set of leaf
   BSDF models may then be another one, and renders resolve other kernels from then on (material_mask_changed).
   The call takes the scene's render lock (it serialises with renders), validates before it writes -- on any error the scene is unchanged: the environment map's
   tables are built in fresh buffers and swapped in at the end, everything else is written after the last check -- and drops the replicas on other devices, which the
   next multi-device render copies again.  A NULL desc, or one with all four pointers NULL, returns PHIP_OK and changes nothing.
   Errors.  Every refusal is one the creation has, with the creation's message and PHIP_ERR_INVALID: a count that differs from the scene's, what phip_scene_create
   refuses of a material array (an unknown BSDF type, a reflectance or a texture maximum -- the NEW texels' -- above 1, a `twosided` that nests a transmissive or a
   later material, a texture id out of range, eta <= 0), an anisotropic BSDF on a shape without texture coordinates, an emitter whose type or shape is not the
   creation's, a texture or environment map whose size or level count is not the creation's or that lacks a level pointer, a bad wrap mode or filter type, a black
   or non-finite environment map, a singular to_world, an `envmap` for a scene without that emitter, device_pointers = 1 with memory that is not the scene's
   device's.  An unsupported microfacet distribution is PHIP_ERR_UNSUPPORTED, as at creation.  PHIP_ERR_DEVICE without a GPU: there is no CPU fallback. */
typedef struct phip_appearance_desc {
    uint32_t n_materials, n_emitters, n_textures;   /* must equal the scene's counts when the matching pointer is set: PHIP_ERR_INVALID otherwise */
    uint32_t device_pointers;      /* 0: every texel pointer below is host memory; 1: device memory of the scene's device */
    const phip_material *materials;/* NULL = unchanged; else n_materials entries, host memory always */
    const phip_emitter  *emitters; /* NULL = unchanged; else n_emitters entries, host memory always: radiance and sampling_weight are taken,
                                      type and shape must be the creation's (PHIP_ERR_INVALID) */
    const phip_texture  *textures; /* NULL = unchanged; else n_textures entries (host structs); an entry with width == 0 leaves that texture alone;
                                      otherwise width, height and n_levels must be the creation's, every level pointer set, and texels, wrap modes,
                                      filter type, max_anisotropy, uv scale / offset are replaced */
    const phip_envmap   *envmap;   /* NULL = unchanged; else the scene must have a PHIP_EMITTER_ENVMAP emitter, width / height / n_levels the creation's;
                                      texels, levels, scale and to_world are replaced */
    void *stream;                  /* device_pointers = 1: the hipStream_t the producer ran on, or NULL; the call is ordered after it */
} phip_appearance_desc;
typedef struct phip_appearance_info {
    double update_ms, kernel_ms;   /* host wall clock of the call; HIP-event time of its device work */
    uint32_t material_mask_changed;/* 1: the set of leaf BSDF models changed, so renders resolve other kernels from now on */
    uint32_t reserved;
} phip_appearance_info;
int phip_scene_update_appearance(phip_scene *scene, const phip_appearance_desc *desc, phip_appearance_info *out_info /* may be NULL */);

/* The MIP pyramid of a texture or an environment map exactly as the reference's TMIPMap builds and stores it (mipmap.h:181-270: a two-lobe Lanczos Resampler per
   axis, X then Y, every level made from the float32 level before it, clamped to [0, max_value] after each pass, negative channels of level 0 set to 0; every level
   stored in half precision), from a level 0 in DEVICE memory into caller-allocated levels in device memory -- what phip_texture.levels[] / phip_envmap.levels[]
   and, with device_pointers = 1, phip_appearance_desc take.  The scene gives the device and the stream (and owns the scratch: the call takes the render lock); it is
   not changed.  The bits are those of the host call phip_mip_pyramid below, and the reference's own.  Complete on return.
   Refusals, PHIP_ERR_INVALID, all before anything is written: a NULL scene or desc, a zero size, a size of 65536 or more (the creation's limit), an n_levels that is
   not the pyramid's own count (sizes halve with max(1, (n + 1) / 2) down to 1 x 1), a bad wrap mode, a max_value that is not > 0 (NaN included), a missing level
   pointer, a pointer that is not 4-byte aligned, levels that overlap (but for d_levels[0] == d_level0), a pointer that is not device memory of the scene's device.
   PHIP_ERR_DEVICE without a GPU. */
typedef struct phip_pyramid_desc {
    uint32_t width, height;        /* of level 0 */
    uint32_t n_levels;             /* the complete count */
    uint32_t wrap_u, wrap_v;       /* phip_wrap_mode per axis: what a tap outside the image reads (an environment map: repeat, clamp) */
    float    max_value;            /* 1 for a bitmap texture, +infinity for an environment map */
    const float *d_level0;         /* height x width x 3 floats (RGB), tight: the layout of phip_texture.levels[] */
    float *d_levels[PHIP_MIP_MAX_LEVELS];   /* d_levels[l], 1 <= l < n_levels: the output levels, caller-allocated, tight RGB floats.  d_levels[0]: NULL (level 0 is
                                      not written), d_level0 itself (rounded in place) or memory of its own */
    void *stream;                  /* the hipStream_t the producer of d_level0 ran on, or NULL; the call is ordered after it */
} phip_pyramid_desc;
int phip_mip_pyramid_device(phip_scene *scene, const phip_pyramid_desc *desc);
/* The same pyramid on HOST memory, without a device: every pointer of the descriptor is host memory, `stream` is ignored.  The same statements run (pyramid_hd.h), so
   the levels are the device call's bit for bit; the refusals are the same but for the device's. */
int phip_mip_pyramid(const phip_pyramid_desc *desc);

/* The vertex normals of a mesh exactly as the reference's TriMesh::computeNormals makes them for a mesh loaded without normals (trimesh.cpp:640-672: every corner
   adds its triangle's unit normal times its own angle -- Thuermer and Wuethrich's weighting, unitAngle of core/util.h:309-314 --, the sum runs in triangle order, a
   vertex whose sum has length 0 gets (1, 0, 0) and is counted), from positions in DEVICE memory into caller-allocated normals in device memory: what
   phip_update_desc.normals takes with device_pointers = 1.  The topology is the scene's own, as created; the scene gives the device too and keeps the incidence
   lists of its vertices from its first call on (the call takes the render lock); it is not changed otherwise.  The bits are those of the host call
   phip_vertex_normals below, and the reference's own but for glibc's asinf.  m_flipNormals is not restated: a caller negates.
   Positions are not validated: non-finite input gives non-finite normals, which phip_scene_update then refuses as it does today.
   Refusals, PHIP_ERR_INVALID, all before anything is written: a NULL scene or desc, NULL positions or normals, counts that are not the scene's, indices that are
   not NULL, a pointer that is not 4-byte aligned, positions and normals that overlap, a pointer that is not device memory of the scene's device.
   PHIP_ERR_DEVICE without a GPU. */
typedef struct phip_normals_desc {
    uint32_t n_vertices, n_triangles;   /* device call: must equal the scene's counts */
    const uint32_t *indices;            /* host call: 3 * n_triangles, host memory; device call: must be NULL (the scene's own) */
    const float *positions;             /* 3 * n_vertices; host call: host memory; device call: device memory of the scene's device */
    float *normals;                     /* 3 * n_vertices out, same memory kind; every vertex is written */
    void *stream;                       /* device call: the producer's hipStream_t or NULL; the call is ordered after it and complete on return */
    uint32_t reserved[2];
} phip_normals_desc;
typedef struct phip_normals_info {
    uint32_t n_invalid;                 /* vertices without a contribution: they got (1, 0, 0) */
    uint32_t reserved;
    double kernel_ms;                   /* device call: the kernel in HIP-event time; host call: 0 */
} phip_normals_info;
int phip_vertex_normals_device(phip_scene *scene, const phip_normals_desc *desc, phip_normals_info *out_info /* may be NULL */);
/* The same normals on HOST memory, without a device: the same statements run (normals_hd.h), so the normals are the device call's bit for bit.  Any indices do,
   also those of several meshes in one array.  Refusals, PHIP_ERR_INVALID, before anything is written: a NULL desc, NULL positions, normals or (with triangles)
   indices, n_vertices == 0, a pointer that is not 4-byte aligned, positions and normals that overlap, an index >= n_vertices. */
int phip_vertex_normals(const phip_normals_desc *desc, phip_normals_info *out_info /* may be NULL */);

/* Thread-safe and sticky, like Scheduler::cancel on a process (src/libcore/sched.cpp): a running phip_render returns
   PHIP_ERR_CANCELLED; a request that arrives before the render starts cancels that render.  The flag is consumed by the
   call that observes it. */
void phip_cancel(phip_scene *scene);

/* (ABI 7) Page-locked host memory for phip_render's out_rgbaw (hipHostMalloc, portable); NULL + phip_last_error() on failure.
   Replaces nothing in the reference: its film lives in the process that renders (src/librender/film.cpp). */
void *phip_host_alloc(size_t bytes);
void  phip_host_free(void *p);

/* RGB = sum/weight (0 where weight == 0): rgbaw[n*5] -> rgb[n*3]. Host-side helper. */
void phip_develop(const float *rgbaw, size_t n_pixels, float *out_rgb);

/* Acceleration-structure facts for DESIGN.md / bench accounting: n_nodes, max_depth, node_bytes (80) and sah_cost are those of the compressed 8-wide tree, which
   every scene has; n_leaves and n_triangle_refs those of the binary tree it was collapsed from. */
typedef struct phip_accel_info {
    uint32_t n_nodes, n_leaves, n_triangle_refs, max_depth;
    uint32_t node_bytes, triangle_bytes;
    float    sah_cost;
    float    build_ms;
    uint32_t fits_lds;       /* 1: leaf table, records, emitter table and materials fit the fused kernel's LDS plan (k_mega) */
    uint32_t fused_traversal; /* how k_mega traverses the scene: 2 / 3 = packed leaf table with masks of <= 32 / <= 64 Wald records, tests dealt over the wave
                                 (was `reserved`, always 0, before round 5: same layout; 0 and 1 were a walk of the BVH4 and a table of plain leaf boxes: retired); round 6, fits_lds = 0:
                                 4 / 5 = k_mega can walk the compressed 8-wide tree from memory (materials in LDS / in memory; PHIP_FLAG_FUSED_ANY) */
} phip_accel_info;
int  phip_scene_accel_info(const phip_scene *scene, phip_accel_info *out);

/* Utilities for callers that fill a phip_scene_desc without Mitsuba at hand (the test harness, bench.py): the table of the reference's default `gaussian` reconstruction
 * filter with the given standard deviation -- (radius, PHIP_FILTER_RESOLUTION + 1 values), rfilter.cpp:38-57 + gaussian.cpp:34-57; the Mitsuba shim copies the scene's own
 * filter instead -- and sizeof of the ABI's structs by index (0 phip_material, 1 phip_shape, 2 phip_emitter, 3 phip_camera, 4 phip_film, 5 phip_scene_desc,
 * 6 phip_render_params, 7 phip_stats, 8 phip_ray, 9 phip_hit, 10 phip_accel_info, 11 phip_update_desc, 12 phip_update_info, 13 phip_surface, 15 phip_radiance_desc; 14 is unassigned and answers 0: tests/test_raycast_device_host.py pins phip_abi_sizeof(14) == 0 as "one past the last struct" and stays as it is, so the new struct skips that index; 16 is unassigned likewise: tests/test_radiance_device_host.py pins it; 17 phip_camera_rays_desc, 18 phip_film_desc; 19 is unassigned likewise: tests/test_camera_film_host.py pins it; 20 phip_appearance_desc, 21 phip_appearance_info; 22 is unassigned likewise: tests/test_appearance_host.py pins it; 23 phip_bsdf_desc, 24 phip_bsdf_sample, 25 phip_emitter_sample_desc, 26 phip_emitter_sample, 27 phip_emitter_eval_desc; 28 is unassigned likewise: tests/test_shading_parts_host.py pins it; 29 phip_pyramid_desc; 30 is unassigned likewise: tests/test_pyramid_host.py pins it; 31 phip_normals_desc, 32 phip_normals_info), for bindings that mirror them (tests/test_abi.py holds the ctypes mirror against it). */
void   phip_gaussian_filter(float stddev, float *radius, float *table);
size_t phip_abi_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif /* PHIP_H */

/*
 * host_boundary.h -- what a call on the caller's device memory needs, stated once: whose memory a pointer is, how it is aligned, how many items one call takes,
 * the stream its work is ordered on, the device its parameters name, a device's CU count, one block per BLOCK items, a refusal under its call's name.
 * The per-call headers (host_raycast.h, host_radiance.h, host_camera_film.h, host_shading_parts.h, host_pyramid.h, host_normals.h, host_update.h, host_appearance.h) and host_render.h use these
 * and keep the texts of their own refusals; the guard that brings an entry point to its body is phip.hip's (onDevice).
 * Host code only; included by phip.hip alone, after host_scene.h.
 */
#pragma once
#include "host_scene.h"

/* items of one call: ray and sample indices are 32-bit handles, 0xFFFFFFFF is none (INVALID_RAY); whole chunks of 64 and blocks of 256 stay below it */
#define CALL_MAX_ITEMS ((size_t) 0xFFFFFF00u)

static bool misaligned(const void *p, size_t align) { return ((uintptr_t) p & (align - 1u)) != 0; }          /* (align: a power of two; NULL is aligned) */

/* a caller's device array: device memory of the scene's device */
static bool onSceneDevice(const void *p, int device) {
    hipPointerAttribute_t attr; memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void) hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice && attr.device == device;
}
/* ... every pointer given of a call's list */
static bool allOnSceneDevice(const SceneDev &sd, std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (p && !onSceneDevice(p, sd.device)) return false;
    return true;
}
static bool allOnSceneDevice(const SceneDev &sd, const void *const *ptrs, size_t n) {          /* (an array of them: the levels of phip_mip_pyramid_device) */
    for (size_t i = 0; i < n; ++i)
        if (ptrs[i] && !onSceneDevice(ptrs[i], sd.device)) return false;
    return true;
}

/* the stream a call's work is ordered on: the caller's, or the scene's, created on first use */
static hipStream_t sceneStream(SceneDev &sd, void *callerStream) {
    if (callerStream) return (hipStream_t) callerStream;
    if (!sd.stream) HIP_TRY(hipStreamCreate(&sd.stream));
    return sd.stream;
}

/* the device the render parameters name, which must be the scene's (`who`: the call's name in front of the refusal, or empty) */
static int paramsDevice(const phip_render_params *p) { return p->n_devices == 1 ? p->devices[0] : p->device; }
static void requireSceneDevice(const SceneDev &sd, const phip_render_params *p, const std::string &who = std::string()) {
    if (paramsDevice(p) != sd.device) throw std::invalid_argument(who + "scene was created on a different device");
}

/* the CU count of a device as the runtime states it; `fallback` where it does not */
static int cuCount(int device, int fallback) {
    hipDeviceProp_t prop;
    return hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : fallback;
}

static unsigned blocksFor(size_t n) { return (unsigned) ((n + BLOCK - 1) / BLOCK); }          /* one lane per item */

/* what an `*ArgsError` function found, as the entry point and its test hook return it: the code, and the text under the call's name; PHIP_OK without a refusal */
static int refusal(const char *name, int code, const char *bad) {
    return bad ? setErr(code, std::string(name) + ": " + bad) : (int) PHIP_OK;
}

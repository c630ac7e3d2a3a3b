/*
 * path_hip.cpp -- Mitsuba 0.6 integrator plugin `path_hip` : the thin C++ shim between the
 * reference's plugin boundary and the MI355X back end (libphip.so, include/phip.h).
 *
 * Build (inside a Mitsuba 0.6 source tree, next to src/integrators/path/):
 *     plugins += env.SharedLibrary('path_hip', ['path_hip/path_hip.cpp'], LIBS = env['LIBS'] + ['phip'])
 * (pattern: src/integrators/SConscript:5).  Select it with <integrator type="path_hip"/>.
 * In this repository it is compiled against the reference's own headers and run inside the reference's libraries
 * (oracle/Makefile.ref, target `shims`; tests/test_gpu_dropin.py); the standalone harness (mitsuba_amd/*.py, tests/)
 * drives the same C ABI through ctypes.  See INTEGRATION.md.
 *
 * What it does, and nothing else (PhipMonteCarloShim in phip_flatten.h, shared with volpath_simple_hip.cpp; this file states what is path_hip's own):
 *   - derives from MonteCarloIntegrator so that maxDepth / rrDepth / strictNormals / hideEmitters
 *     parse, validate and serialise exactly like `path` (src/librender/integrator.cpp:190-225);
 *   - preprocess(): flattens Scene::getShapes() into a phip_scene_desc (every Shape through
 *     createTriMesh() unless it already is a TriMesh) and calls phip_scene_create (phip_flatten.h, shared with direct_hip.cpp);
 *   - render(): overrides SamplingIntegrator::render (integrator.cpp:95-129): one phip_render call,
 *     then film->put() of one full-frame ImageBlock; returns false when cancelled;
 *   - cancel(): phip_cancel (integrator.cpp:90-93);
 *   - Li(): still required by the interface (integrator.h:321-322, used by `adaptive`/`irrcache`):
 *     delegates to a nested CPU `path` integrator with the same parameters.
 */
#include "phip_flatten.h"

MTS_NAMESPACE_BEGIN

class PathHIP : public PhipMonteCarloShim<PathHIP> {
public:
    static const char *name() { return "path_hip"; }
    static const char *nested() { return "path"; }
    static uint32_t integrator() { return PHIP_INTEGRATOR_PATH; }
    void checkScene(const Scene *) { }

    PathHIP(const Properties &props) : PhipMonteCarloShim<PathHIP>(props) { }
    PathHIP(Stream *stream, InstanceManager *manager) : PhipMonteCarloShim<PathHIP>(stream, manager) { }

    MTS_DECLARE_CLASS()
};

MTS_IMPLEMENT_CLASS_S(PathHIP, false, MonteCarloIntegrator)
MTS_EXPORT_PLUGIN(PathHIP, "MI355X path tracer (path_hip)");
MTS_NAMESPACE_END

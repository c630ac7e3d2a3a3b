/*
 * volpath_simple_hip.cpp -- Mitsuba 0.6 integrator plugin `volpath_simple_hip`: the shim of path_hip.cpp (see there for what it does) for the sibling
 * integrator `volpath_simple` (src/integrators/path/volpath_simple.cpp) on scenes WITHOUT participating media -- the path tracer without multiple importance
 * sampling, PHIP_INTEGRATOR_VOLPATH_SIMPLE of include/phip.h.  Media are outside the back end's scope: a scene that has any is refused in
 * preprocess() with an error, as the reference refuses what a plugin cannot render (Log(EError)).
 *
 * Build (inside a Mitsuba 0.6 source tree, next to src/integrators/path/):
 *     plugins += env.SharedLibrary('volpath_simple_hip', ['path_hip/volpath_simple_hip.cpp'], LIBS = env['LIBS'] + ['phip'])
 * (pattern: src/integrators/SConscript:5).  Select it with <integrator type="volpath_simple_hip"/>.
 * Parameters parse like `volpath_simple` (= those of `path`: maxDepth, rrDepth, strictNormals, hideEmitters); Li() delegates to a nested CPU
 * `volpath_simple` with the same parameters.  Everything else is PhipMonteCarloShim (phip_flatten.h).
 */
#include "phip_flatten.h"

MTS_NAMESPACE_BEGIN

class VolPathSimpleHIP : public PhipMonteCarloShim<VolPathSimpleHIP> {
public:
    static const char *name() { return "volpath_simple_hip"; }
    static const char *nested() { return "volpath_simple"; }
    static uint32_t integrator() { return PHIP_INTEGRATOR_VOLPATH_SIMPLE; }
    void checkScene(const Scene *scene) {
        if (!scene->getMedia().empty())
            Log(EError, "volpath_simple_hip: the scene contains participating media -- the GPU back end renders surfaces only (use `volpath_simple`)");
    }

    VolPathSimpleHIP(const Properties &props) : PhipMonteCarloShim<VolPathSimpleHIP>(props) { }
    VolPathSimpleHIP(Stream *stream, InstanceManager *manager) : PhipMonteCarloShim<VolPathSimpleHIP>(stream, manager) { }

    MTS_DECLARE_CLASS()
};

MTS_IMPLEMENT_CLASS_S(VolPathSimpleHIP, false, MonteCarloIntegrator)
MTS_EXPORT_PLUGIN(VolPathSimpleHIP, "MI355X path tracer without MIS (volpath_simple_hip)");
MTS_NAMESPACE_END

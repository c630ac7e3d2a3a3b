"""k_shade_trace_w (k_shade_trace_w.h): vertex, shadow ray and next ray of a slot in ONE kernel per iteration on the compressed 8-wide tree in memory -- the scenes
between the packed leaf table (<= 64 Wald records) and the big trees whose bitmap textures, texture coordinates or environment emitter keep them off k_mega.

Every sample must be the oracle's and the wavefront kernels' (k_shade + k_rays_w) bit for bit: the kernel shades with the same shadeVertex, its traversal returns the
structure-independent hit, and the vertex's additions join L[id] in the same order.  Shapes: the Cornell box with two spheres of 6 x 4 (104 triangles: past the 64
records of the packed table, and small enough for the oracle's sweep over all triangles) and of 24 x 12 segments (1088 triangles, 111 wide nodes: more than the 48 a
block stages in LDS, so nodes are also fetched from memory); films of 64 x 64 and a ragged 100 x 70 (partial blocks of slots, edge tiles)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_l2, sobol_tables, qmc_tables
from mitsuba_amd import _abi as A, scene as S
from ref_scenes import _sphere_uvs, _checker, _sky, half
from test_gpu_parity import compare_render, gpu  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

# Measured, the kernel is ahead of the wavefront kernels at no tree size, so no tree runs it by default (PHIP_SHADE_TRACE_WIDE_MAX_NODES = 0): every
# render that is to reach it passes PHIP_FLAG_FUSED_ANY, and the default render of its scenes is the wavefront kernels'
ANY = A.PHIP_FLAG_FUSED_ANY

SIZES = {"104": (6, 4), "1088": (24, 12)}
GAVE_UP = "warning: the fused kernel gave up"


def sphere_box(gauss, kind, nlon, nlat, w=64, h=64):
    """the Cornell box with two tessellated spheres (S.cornell_spheres' places) and what keeps it off k_mega:
    albedo    an EWA `bitmap` albedo on one sphere, a trilinear one on the other (diffuse only: the MM = 0 kernels)
    roughmap  a glass sphere and a copper sphere with a `bitmap` on its roughness (all three BSDF models: the class deal)
    constant  glass + copper under a `constant` environment emitter
    envmap    glass + copper under an `envmap` with its pyramid (the filtered lookup of the visible background)
    plain     S.cornell_spheres itself: a scene of k_mega (PHIP_FLAG_NO_MEGA)"""
    if kind == "plain":
        return S.cornell_spheres(w, h, gauss, nlon=nlon, nlat=nlat)
    sb = S.SceneBuilder()
    if kind == "constant":
        sb.constant((0.5, 0.6, 0.8), sampling_weight=0.7)       # environment emitters first: the order of Scene::getEmitters()
    if kind == "envmap":
        rng = np.random.default_rng(5)
        sb.envmap(half(_sky(32, 16) * rng.uniform(0.5, 1.5, (16, 32, 1))), scale=0.6, pyramid=True)
    S.cornell_box(w, h, gauss, sb=sb)
    if kind == "albedo":
        rng = np.random.default_rng(11)
        t_alb = sb.bitmap(half(rng.uniform(0.05, 0.95, (24, 40, 3))), filter_type="ewa", uscale=2.0)
        t_chk = sb.bitmap(half(_checker(32, 4)), filter_type="trilinear", wrap="mirror", uscale=3.0, vscale=3.0)
        m0, m1 = sb.diffuse(texture=t_alb), sb.twosided(sb.diffuse(texture=t_chk))
    elif kind == "roughmap":
        t_a = sb.bitmap(half(0.04 + 0.5 * _checker(32, 4)), filter_type="ewa")
        m0, m1 = sb.dielectric(1.5, 1.0), sb.twosided(sb.roughconductor(S.CU_ETA, S.CU_K, alpha=0.15, alpha_texture=t_a))
    else:
        m0, m1 = sb.dielectric(1.5, 1.0), sb.twosided(sb.roughconductor(S.CU_ETA, S.CU_K, alpha=0.15))
    for centre, radius, m in (((185, 120, 170), 70.0, m0), ((370, 330, 350), 60.0, m1)):
        P, T, N = S.sphere_mesh(centre, radius, nlon, nlat)
        sb.mesh(P, T, m, normals=N, uvs=_sphere_uvs(N) if kind in ("albedo", "roughmap") else None)
    return sb


def render(gpu, gs, integ, spp, flags=0, **kw):
    film = gpu.HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER | flags, **kw)
    return film.storage.copy(), integ.samples(gs, spp).copy(), integ.stats


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def test_textured_sphere_box_runs_one_kernel_per_iteration(gpu, gauss):
    """the scene class the feature is for, under PHIP_FLAG_FUSED_ANY: no k_mega, no ray kernel, more than one iteration"""
    sb = sphere_box(gauss, "albedo", *SIZES["104"])
    assert sb.n_triangles > 64
    gs = gpu.Scene(sb.desc())
    ai = gs.accel_info()
    assert ai.fits_lds == 0 and ai.fused_traversal == 0, (ai.fits_lds, ai.fused_traversal)      # not a scene of k_mega, and phip_accel_info says so as before
    integ = gpu.PathHIP(maxDepth=6)
    film = gpu.HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, 4, flags=A.PHIP_FLAG_KERNEL_TIMING | ANY)
    st = integ.stats
    assert st.vertex_traced == 1 and st.fused == 0 and st.iterations > 1, st.as_dict()
    assert st.trace_kernel_ms == 0 and st.shadow_kernel_ms == 0 and st.shade_kernel_ms > 0, st.as_dict()
    assert st.samples == gs.width * gs.height * 4
    assert integ.render(gs, film, 4) and integ.stats.vertex_traced == 0 and integ.stats.fused == 0                # the default: the parent's path
    gs.close()


@pytest.mark.parametrize("res", [(64, 64), (100, 70)])
def test_textured_sphere_box_matches_oracle_and_wavefront(gpu, oracle, gauss, res):
    """compare_render: every sample the oracle's (the sweep: 104 triangles), film, samples and ray / vertex counts those of PHIP_FLAG_NO_FUSED (it takes that leg
    because vertex_traced is set)"""
    same, r = compare_render(gpu, oracle, sphere_box(gauss, "albedo", *SIZES["104"], w=res[0], h=res[1]).desc(), 8, min_identical=1.0, render_kw=dict(flags_extra=ANY), maxDepth=6)
    assert same == 1.0, same


def _cases():
    from mitsuba_amd.integrator import PathHIP, VolPathSimpleHIP
    return {"roughmap": ("roughmap", PathHIP, dict(maxDepth=6), None),
            "constant": ("constant", PathHIP, dict(maxDepth=6), None),
            "envmap": ("envmap", PathHIP, dict(maxDepth=6), None),
            "strict": ("roughmap", PathHIP, dict(maxDepth=6, strictNormals=True), None),
            "unbounded": ("albedo", PathHIP, dict(maxDepth=-1), None),
            "volpath": ("roughmap", VolPathSimpleHIP, dict(maxDepth=6), None),
            "sobol": ("envmap", PathHIP, dict(maxDepth=6), lambda w, h: dict(sobol=sobol_tables(w, h))),
            "halton": ("roughmap", PathHIP, dict(maxDepth=6), lambda w, h: dict(sampler=A.PHIP_SAMPLER_HALTON, qmc=qmc_tables(-1)))}


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("case", ["roughmap", "constant", "envmap", "strict", "unbounded", "volpath", "sobol", "halton"])
def test_feature_sets_match_oracle_and_wavefront(gpu, oracle, gauss, case, size):
    kind, cls, ikw, rkw = _cases()[case]
    sb = sphere_box(gauss, kind, *SIZES[size])
    gs = gpu.Scene(sb.desc())
    integ = cls(**ikw)
    kw = rkw(gs.width, gs.height) if rkw else {}
    assert integ.render(gs, gpu.HDRFilm(gs.width, gs.height), 1, flags=ANY, **kw) and integ.stats.vertex_traced == 1, integ.stats.as_dict()      # (k_shade_trace_w is what compare_render holds up)
    gs.close()
    # 1088 triangles: the kd-tree oracle (a sweep per ray is out of reach); the few samples an edge ray separates are re-evaluated one by one (compare_render)
    same, r = compare_render(gpu, oracle, sb.desc(), 4, min_identical=1.0 if size == "104" else 0.9999, integrator=None if cls.__name__ == "PathHIP" else cls,
                             render_kw=dict(kw, flags_extra=ANY), **ikw)


def test_no_mega_on_an_untextured_sphere_box_reaches_the_kernel(gpu, gauss):
    """PHIP_FLAG_NO_MEGA (with PHIP_FLAG_FUSED_ANY: the kernel is on) on a scene k_mega serves on the tree in memory: the one-kernel iterations, with k_mega's and the
    wavefront kernels' bits"""
    for size in sorted(SIZES):
        gs = gpu.Scene(sphere_box(gauss, "plain", *SIZES[size]).desc())
        assert gs.accel_info().fused_traversal == 4
        integ = gpu.PathHIP(maxDepth=6)
        f0, s0, st0 = render(gpu, gs, integ, 4)
        assert st0.fused == 1 and st0.vertex_traced == 0
        f1, s1, st1 = render(gpu, gs, integ, 4, flags=A.PHIP_FLAG_NO_MEGA | ANY)
        assert st1.fused == 0 and st1.vertex_traced == 1, st1.as_dict()
        f2, s2, st2 = render(gpu, gs, integ, 4, flags=A.PHIP_FLAG_NO_FUSED)
        assert st2.fused == 0 and st2.vertex_traced == 0
        assert same_bits(s1, s0) and same_bits(f1, f0) and same_bits(s1, s2) and same_bits(f1, f2), size
        for st in (st0, st2):
            assert (st.samples, st.path_vertices, st.closest_rays, st.shadow_rays) == (st1.samples, st1.path_vertices, st1.closest_rays, st1.shadow_rays)
        gs.close()


def test_big_tree_runs_the_kernel_under_fused_any_only(gpu, gauss):
    """a big tree: the wavefront kernels by default, k_shade_trace_w with PHIP_FLAG_FUSED_ANY -- same bits.  (The atrium is untextured: k_mega would take it under the flag,
    so PHIP_FLAG_NO_MEGA rides along.)"""
    gs = gpu.Scene(S.atrium(96, 54, gauss, detail=0.3).desc())       # 22 k triangles, ~2500 wide nodes
    assert gs.accel_info().n_nodes > A.PHIP_SHADE_TRACE_WIDE_MAX_NODES
    integ = gpu.PathHIP(maxDepth=6)
    f0, s0, st0 = render(gpu, gs, integ, 4, flags=A.PHIP_FLAG_NO_MEGA)
    assert st0.vertex_traced == 0 and st0.fused == 0, st0.as_dict()
    f1, s1, st1 = render(gpu, gs, integ, 4, flags=A.PHIP_FLAG_NO_MEGA | A.PHIP_FLAG_FUSED_ANY)
    assert st1.vertex_traced == 1 and st1.fused == 0, st1.as_dict()
    assert same_bits(s1, s0) and same_bits(f1, f0)
    assert (st0.samples, st0.path_vertices, st0.closest_rays, st0.shadow_rays) == (st1.samples, st1.path_vertices, st1.closest_rays, st1.shadow_rays)
    gs.close()


def test_several_passes_and_accumulation(gpu, phip, gauss, monkeypatch):
    """a job of several passes (PHIP_MAX_PASS_SAMPLES) and 3 + 5 samples accumulated over two calls: the samples are the single call's bit for bit; the film is the
    wavefront kernels' film of the same split bit for bit, and the single call's up to the order of its float additions (at most 8 samples x 25 filter taps per pixel,
    each addition within 2^-24 relative: the bound of test_progressive_passes_add_up_to_the_single_render)"""
    w, h, spp = 100, 70, 8
    gs = gpu.Scene(sphere_box(gauss, "roughmap", *SIZES["1088"], w=w, h=h).desc())
    integ = gpu.PathHIP(maxDepth=6)
    f1, s1, st1 = render(gpu, gs, integ, spp, flags=ANY)
    assert st1.vertex_traced == 1
    monkeypatch.setenv("PHIP_MAX_PASS_SAMPLES", str(4 * 3 * 1024 * 3))      # twelve 32 x 32 tiles: three samples per pass -> 3 + 3 + 2
    fm, sm, stm = render(gpu, gs, integ, spp, flags=ANY)
    fw, sw, stw = render(gpu, gs, integ, spp, flags=A.PHIP_FLAG_NO_FUSED)
    monkeypatch.delenv("PHIP_MAX_PASS_SAMPLES")
    assert stm.vertex_traced == 1 and stw.vertex_traced == 0 and stm.samples == st1.samples == w * h * spp
    assert same_bits(sm, s1) and same_bits(sm, sw) and same_bits(fm, fw)
    assert rel_l2(fm, f1) < 2e-6

    def two_calls(base):
        block = np.zeros((h, w, 5), np.float32); st = A.phip_stats()
        for n, off, fl in ((3, 0, 0), (5, 3, A.PHIP_FLAG_ACCUMULATE)):
            p = integ.params(gs, n, flags=base | fl, sample_offset=off, sample_total=spp)
            assert phip.phip_render(gs._h, C.byref(p), block.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)) == 0
            assert st.samples == w * h * n and st.vertex_traced == (1 if base == ANY else 0)
        return block
    acc, acc_w = two_calls(ANY), two_calls(A.PHIP_FLAG_NO_FUSED)
    assert same_bits(acc, acc_w)
    assert rel_l2(acc, f1) < 2e-6 and np.abs(acc[..., 4] - f1[..., 4]).max() < 1e-4
    gs.close()


def test_guards_direct_and_no_fused(gpu, gauss):
    """`direct` is not served: the frame and the path are the parent's (k_shade_direct + k_rays_w); PHIP_FLAG_NO_FUSED keeps the kernel off"""
    gs = gpu.Scene(sphere_box(gauss, "albedo", *SIZES["104"]).desc())
    d = gpu.DirectHIP(shadingSamples=2)
    f0, s0, st0 = render(gpu, gs, d, 4)
    f1, s1, st1 = render(gpu, gs, d, 4, flags=A.PHIP_FLAG_NO_FUSED)
    assert st0.vertex_traced == 0 and st0.fused == 0 and st1.vertex_traced == 0
    assert same_bits(f0, f1) and same_bits(s0, s1)
    f0, s0, st0 = render(gpu, gs, d, 4, flags=ANY)
    assert st0.vertex_traced == 0 and same_bits(f0, f1) and same_bits(s0, s1)
    f2, s2, st2 = render(gpu, gs, gpu.PathHIP(maxDepth=6), 4, flags=A.PHIP_FLAG_NO_FUSED | ANY)
    assert st2.vertex_traced == 0 and st2.fused == 0
    gs.close()


_CHILD = r"""
import sys, os, json
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from mitsuba_amd import _ffi, _abi as A, scene as S
from mitsuba_amd.integrator import Scene, PathHIP, HDRFilm
from test_gpu_shade_trace_wide import sphere_box, SIZES
ft = _ffi.gaussian_filter(0.5)
out = {}
for name, kind, size, flags in json.loads(sys.argv[2]):
    sys.stderr.write("@@case %%s\n" %% name); sys.stderr.flush()
    sb = S.atrium(96, 54, ft, detail=0.3) if kind == "atrium" else sphere_box(ft, kind, *SIZES[size])
    gs = Scene(sb.desc()); integ = PathHIP(maxDepth=6); film = HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, 4, flags=A.PHIP_FLAG_SAMPLE_BUFFER | flags)
    out[name + "_samples"] = integ.samples(gs, 4).copy(); out[name + "_film"] = film.storage.copy()
    out[name + "_stats"] = np.array([integ.stats.vertex_traced, integ.stats.fused, integ.stats.samples], np.int64)
    gs.close()
np.savez(sys.argv[1], **out)
"""


def _child(tmp_path, tag, lib, cases):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = str(tmp_path / (tag + ".npz"))
    env = dict(os.environ)
    env.pop("PHIP_LIB", None); env.pop("PHIP_MAX_PASS_SAMPLES", None)
    if lib:
        env["PHIP_LIB"] = lib
    r = subprocess.run([sys.executable, "-c", _CHILD % (root, os.path.join(root, "tests")), f, json.dumps(cases)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (tag, r.stdout[-2000:] + r.stderr[-3000:])
    logs = {}
    for part in r.stderr.split("@@case ")[1:]:
        head, _, body = part.partition("\n")
        logs[head.strip()] = body
    return np.load(f), logs


def test_stack_limits_spill_and_overflow(gpu, gauss, tmp_path):
    """the task stacks' limits with the libraries of _ffi.TEST_VARIANTS.  32-entry LDS stacks (cap32): what does not fit spills to the wave's slice of the spill buffer --
    the same bits.  128-entry stacks in all (overflow): the 1088-triangle box and the atrium outgrow them, the wave stops and says so -- the call succeeds, warns, the job is
    finished by the wavefront kernels (vertex_traced 0) and the frame is theirs bit for bit."""
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available: the test libraries cannot be built")
    from mitsuba_amd import _ffi
    any_ = A.PHIP_FLAG_NO_MEGA | A.PHIP_FLAG_FUSED_ANY
    cases = [("box", "roughmap", "1088", ANY), ("env", "envmap", "104", ANY), ("atrium", "atrium", "", any_)]
    ref = [(n + "_wf", k, s, A.PHIP_FLAG_NO_FUSED) for n, k, s, _ in cases]
    prod, plog = _child(tmp_path, "product", None, cases + ref)
    for n, _, _, _ in cases:
        assert prod[n + "_stats"][0] == 1 and prod[n + "_wf_stats"][0] == 0 and GAVE_UP not in plog[n], n
        assert same_bits(prod[n + "_samples"], prod[n + "_wf_samples"]) and same_bits(prod[n + "_film"], prod[n + "_wf_film"]), n
    cap, clog = _child(tmp_path, "cap32", _ffi.build_test_variant("cap32"), cases)
    for n, _, _, _ in cases:
        assert cap[n + "_stats"][0] == 1 and "warning" not in clog[n], (n, clog[n][-500:])          # (the stack spilled, it did not overflow)
        assert same_bits(cap[n + "_samples"], prod[n + "_samples"]) and same_bits(cap[n + "_film"], prod[n + "_film"]), n
    ovf, olog = _child(tmp_path, "overflow", _ffi.build_test_variant("overflow"), cases)
    gave_up = [n for n, _, _, _ in cases if GAVE_UP in olog[n]]
    assert "box" in gave_up and "atrium" in gave_up, olog
    for n, _, _, _ in cases:
        assert ovf[n + "_stats"][0] == (0 if n in gave_up else 1), (n, ovf[n + "_stats"])
        assert ovf[n + "_stats"][2] == prod[n + "_stats"][2], n                                     # every sample counted once
        assert same_bits(ovf[n + "_samples"], prod[n + "_wf_samples"]) and same_bits(ovf[n + "_film"], prod[n + "_wf_film"]), n

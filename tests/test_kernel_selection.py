"""Which kernel a render runs, pinned on the CPU.

The host resolves one kernel per render from the scene's feature set, its leaf BSDF models, strictNormals, the table set / traversal form, the sampler and the
integrator (phip.hip: shadeKernelOf, shadeTraceWideKernelOf, megaKernelOf over the look-ups of the other units).  A wrong entry that picks a SUPERSET kernel -- FEAT 3
for a FEAT 1 scene, the all-materials build for a diffuse scene, the generic-pointer k_shade where the LDS-table one was meant -- renders the same bits and only costs
speed, so no parity test sees it.  phip_debug_selected_kernel (libphip_debug.so) calls the same functions and returns the name the dynamic symbol table has for the
kernel's host pointer: its mangled name, whose template arguments these tests hold against the key.  No HIP call is made: no GPU is needed."""
import concurrent.futures
import itertools
import os
import re

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, resources

FEATS = (0, 1, 2, 3, 8, 11)             # environment emitter | bitmap textures << 1; 8: the QMC samplers, 11: with both other features
MASKS = (0, 1, 2, 3)                    # MM_ROUGH | MM_DIELECTRIC; MM_ALL = 3
MM_ALL = 3
SHADE, SHADE_TRACE, SHADE_TRACE_WIDE, MEGA = 0, 1, 2, 3     # the families of phip_debug_selected_kernel


def selected(family, feat=0, mask=0, strict=False, form=0, qmc=False, direct=False):
    name = _ffi.debug_lib().phip_debug_selected_kernel(family, feat, mask, int(strict), form, int(qmc), int(direct))
    return name.decode() if name is not None else None


def template_args(name, kernel):
    """the integer / bool template arguments of the instantiation `name` of `kernel` (Itanium mangling: Li<n>E, Lb<0|1>E)"""
    m = re.match(r"_Z%d%sI((?:L[ib]\d+E)+)Ev" % (len(kernel), kernel), name or "")
    assert m, (kernel, name)
    return tuple(int(a) for a in re.findall(r"L[ib](\d+)E", m.group(1)))


def table_sets(feat):
    """k_shade's table sets the host can form for a feature set (shadeTableSet): FEAT 0 alone has the builds with both tables (1) / the emitter table (2) in LDS"""
    return (0, 1, 2) if feat == 0 else (0,)


def shade_names(feats=FEATS):
    return {(feat, strict, mask, tables): selected(SHADE, feat, mask, strict, tables)
            for feat in feats for strict in (False, True) for mask in MASKS for tables in table_sets(feat)}


def shade_direct_names(feats=FEATS):
    return {(feat, mask): selected(SHADE, feat, mask, direct=True) for feat in feats for mask in MASKS}


def shade_trace_names(family, feats=FEATS):
    return {(feat, strict, mask): selected(family, feat, mask, strict) for feat in feats for strict in (False, True) for mask in MASKS}


# k_mega's parts: the traversal forms each holds, and whether it is the `direct` build (strictNormals is a run-time switch of that integrator: the host passes false)
MEGA_PARTS = {"phip_mega.o": ((2, 3), False), "phip_megaw.o": ((4, 5), False), "phip_megad.o": ((2, 3, 4, 5), True)}


def mega_names(obj):
    forms, direct = MEGA_PARTS[obj]
    return {(mask, strict, flat, qmc): selected(MEGA, 0, mask, strict, flat, qmc, direct)
            for mask in MASKS for strict in ((False,) if direct else (False, True)) for flat in forms for qmc in (False, True)}


def test_k_shade_is_the_build_of_the_feature_set_the_models_and_the_table_set():
    names = shade_names()
    for (feat, strict, mask, tables), name in names.items():
        want_feat = feat if tables == 0 else (4 if tables == 1 else 16)
        assert template_args(name, "k_shade") == (mask & MM_ALL, int(strict), want_feat), ((feat, strict, mask, tables), name)
    assert len(set(names.values())) == len(names) == 64


def test_k_shade_direct_is_the_build_of_the_feature_set():
    names = shade_direct_names()
    for (feat, mask), name in names.items():
        assert template_args(name, "k_shade_direct") == (MM_ALL if mask else 0, feat), ((feat, mask), name)
    assert len(set(names.values())) == 12


@pytest.mark.parametrize("family,kernel", [(SHADE_TRACE, "k_shade_trace"), (SHADE_TRACE_WIDE, "k_shade_trace_w")])
def test_one_kernel_iterations_are_the_build_of_the_feature_set(family, kernel):
    names = shade_trace_names(family)
    for (feat, strict, mask), name in names.items():
        assert template_args(name, kernel) == (MM_ALL if mask else 0, int(strict), feat), ((feat, strict, mask), name)
    assert len(set(names.values())) == 24


@pytest.mark.parametrize("obj", sorted(MEGA_PARTS))
def test_k_mega_is_the_build_of_the_form_the_sampler_and_the_integrator(obj):
    forms, direct = MEGA_PARTS[obj]
    names = mega_names(obj)
    for (mask, strict, flat, qmc), name in names.items():
        assert template_args(name, "k_mega") == (MM_ALL if mask else 0, int(strict), flat, int(qmc), int(direct)), ((mask, strict, flat, qmc), name)
    assert len(set(names.values())) == 16
    # a form no build holds resolves to nothing (the render then runs on the wavefront kernels): the forms 0 and 1 of the retired tree walks, and whatever lies past 5
    for flat, strict, qmc in itertools.product((0, 1, 6), (False, True), (False, True)):
        assert selected(MEGA, 0, 0, strict, flat, qmc, direct) is None, (flat, strict, qmc)


@pytest.fixture(scope="module")
def compiled():
    """{object name: the kernels the compiler built into it} for one feature set of the shading kernels and the three parts of k_mega"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    objs = ["phip_shade0_%d.o" % part for part in range(4)] + ["phip_tracew0.o"] + sorted(MEGA_PARTS)
    units = [next(u for u in _ffi.UNITS if u[2] == obj) for obj in objs]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 4)) as pool:
        return dict(zip(objs, pool.map(lambda u: set(resources(u[0], u[1])), units)))


def kernels(compiled, objs, kernel):
    prefix = "_Z%d%sI" % (len(kernel), kernel)
    return {name for obj in objs for name in compiled[obj] if name.startswith(prefix)}


def test_every_compiled_shading_kernel_of_a_feature_set_is_reachable(compiled):
    """FEAT 0, the feature set with three table sets: what the selection can return is exactly what its five objects hold"""
    assert set(shade_names((0,)).values()) == kernels(compiled, ("phip_shade0_0.o", "phip_shade0_1.o"), "k_shade")
    assert set(shade_direct_names((0,)).values()) == kernels(compiled, ("phip_shade0_2.o",), "k_shade_direct")
    assert set(shade_trace_names(SHADE_TRACE, (0,)).values()) == kernels(compiled, ("phip_shade0_3.o",), "k_shade_trace")
    assert set(shade_trace_names(SHADE_TRACE_WIDE, (0,)).values()) == kernels(compiled, ("phip_tracew0.o",), "k_shade_trace_w")


@pytest.mark.parametrize("obj", sorted(MEGA_PARTS))
def test_every_compiled_fused_kernel_is_reachable(compiled, obj):
    built = kernels(compiled, (obj,), "k_mega")
    assert len(built) == 16
    assert set(mega_names(obj).values()) == built

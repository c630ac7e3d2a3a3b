"""Register budgets of the kernels of phip_radiance_device (phip_shade_r.hip), read from the compiler as tests/test_kernel_resources.py reads the others'.

k_shade_r is k_shade with a caller's ray array behind its epilogue and takes its siblings' wave budgets (__launch_bounds__: SHADE_WAVES_LEAN / _PLAIN / SHADE_WAVES =
4 / 5 / 4 waves per SIMD).

The 16 builds with LDS-addressed tables (FEAT 4 and 16 of feature set 0: the scenes without environment emitter and textures) are held to the absolute numbers
k_shade's are held to (test_shading_kernels_of_the_metric_configurations_keep_their_waves): at most 88 VGPRs for the diffuse builds and 96 for the others, scratch
within k_shade's own bounds, LDS that admits five blocks per CU -- and scalar registers that admit as many 256-thread blocks per CU as the launch bound names waves
per SIMD (blocks_per_cu_by_sgprs, as for the persistent ray kernels): the kernel carries a by-value argument more than k_shade (RaySamples, 24 bytes).

Every other build -- the general-table build of feature set 0 and the feature sets with an environment emitter and / or textures (part 0) -- is held to its k_shade
SIBLING, compiled beside it: the VGPRs its launch bound allows, the same scalar-register test, and scratch of at most the sibling's plus 16 bytes.  The reasoning
behind that margin: k_shade_r's vertex code is the sibling's minus what FEAT bit 5 compiles out (texture partials, the filtered environment look-up), and its
regeneration swaps the camera's matrix arithmetic for two 16-byte loads, so it has no reason to keep more values alive than the sibling; 16 bytes (four dwords) is
the difference the register allocator shows between neighbouring instantiations of k_shade itself for no change of source at all.
k_radiance_out is a streaming kernel: no scratch, one wave's worth of registers at full occupancy (64 VGPRs)."""
import concurrent.futures
import os
import re

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, blocks_per_cu_by_sgprs, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def launch_waves(mm, feat):
    """the second argument of k_shade's and k_shade_r's __launch_bounds__ (k_shade.h)"""
    src = open(os.path.join(_ffi.CSRC, "k_shade.h")).read()
    lean, plain, other = (int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("SHADE_WAVES_LEAN", "SHADE_WAVES_PLAIN", "SHADE_WAVES"))
    assert (lean, plain, other) == (4, 5, 4)
    return lean if mm == 0 else (plain if (feat & 3) == 0 else other)


@pytest.fixture(scope="module")
def compiled():
    """{object: kernels} of the k_shade_r objects of part 0 (and both parts of feature set 0) and of their k_shade siblings"""
    objs = ["phip_radiance0_0.o", "phip_radiance0_1.o"] + ["phip_radiance%d_0.o" % f for f in (1, 2, 3)] + ["phip_shade%d_0.o" % f for f in (0, 1, 2, 3)]
    units = [next(u for u in _ffi.UNITS if u[2] == o) for o in objs]
    assert all(u[0] == ("phip_shade_r.hip" if "radiance" in u[2] else "phip_shade.hip") for u in units)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 4)) as pool:
        return dict(zip(objs, pool.map(lambda u: resources(u[0], u[1]), units)))


def rays_kernels(res):
    out = {}
    for name, v in res.items():
        m = re.match(r"_Z9k_shade_rILi(\d)ELb([01])ELi(\d+)E", name)
        if m:
            out[int(m.group(1)), int(m.group(2)), int(m.group(3))] = v
    return out


def test_ray_fed_vertex_kernels_of_the_lds_table_builds_keep_the_budgets_of_k_shade(compiled):
    res = dict(compiled["phip_radiance0_0.o"]); res.update(compiled["phip_radiance0_1.o"])
    assert not any(name.startswith("_Z7k_shadeI") for name in res), list(res)          # k_shade itself stays phip_shade.hip's
    ks = rays_kernels(res)
    assert sorted({f for _, _, f in ks}) == [0, 4, 16]                                 # the template argument is k_shade's; bit 5 is added inside
    seen = 0
    for (mm, strict, feat), v in ks.items():
        if feat == 0:
            continue
        seen += 1
        print((mm, strict, feat), v)
        assert v["vgprs"] <= (88 if mm == 0 else 96), ((mm, strict, feat), v)
        assert v["scratch"] <= (64 if (mm in (1, 2) and strict == 0) else 96), ((mm, strict, feat), v)
        assert 5 * v["lds"] <= 160 * 1024, ((mm, strict, feat), v)
        assert blocks_per_cu_by_sgprs(v["sgprs"]) >= launch_waves(mm, feat), ((mm, strict, feat), v)
    assert seen == 16                                                                  # 4 material sets x strictNormals x {both tables in LDS, the emitter table only}
    out = [v for name, v in res.items() if name.startswith("_Z14k_radiance_out")]
    assert len(out) == 1 and out[0]["scratch"] == 0 and out[0]["vgprs"] <= 64 and blocks_per_cu_by_sgprs(out[0]["sgprs"]) >= 8, out
    for obj in ("phip_radiance0_1.o", "phip_radiance1_0.o"):                           # ... and lives in one object
        assert not any(name.startswith("_Z14k_radiance_out") for name in compiled[obj])


@pytest.mark.parametrize("fset", [0, 1, 2, 3])
def test_general_table_builds_and_the_other_feature_sets_stay_within_their_k_shade_siblings(compiled, fset):
    mine = rays_kernels(compiled["phip_radiance%d_0.o" % fset])
    sib = {}
    for name, v in compiled["phip_shade%d_0.o" % fset].items():
        m = re.match(r"_Z7k_shadeILi(\d)ELb([01])ELi(\d+)E", name)
        if m:
            sib[int(m.group(1)), int(m.group(2)), int(m.group(3))] = v
    assert sorted(mine) == sorted(sib) and len(mine) == (12 if fset == 0 else 4)
    seen = 0
    for key, v in mine.items():
        mm, strict, feat = key
        if feat != fset:
            continue                                                                   # (the LDS-table builds: the test above)
        seen += 1
        waves = launch_waves(mm, feat)
        print(key, "k_shade_r", v, "k_shade", sib[key])
        assert v["vgprs"] <= 512 // waves // 8 * 8, (key, v)
        assert blocks_per_cu_by_sgprs(v["sgprs"]) >= waves, (key, v)
        assert v["scratch"] <= sib[key]["scratch"] + 16, (key, v, sib[key])
        assert v["lds"] <= sib[key]["lds"], (key, v, sib[key])
    assert seen == 4                                                                   # the four material sets, no strictNormals

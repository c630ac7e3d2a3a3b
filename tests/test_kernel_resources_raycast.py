"""Register budgets of the kernels of phip_trace_device (phip_raycast.hip), read from the compiler as tests/test_kernel_resources.py reads the others'.

k_raycast_p is k_rays_w's persistent loop on a caller's ray array: the same blocks of WIDE_BLOCK threads at WIDE_WAVES = 7 waves per SIMD, so the same budget --
no scratch, at most 72 VGPRs, scalar registers that admit seven blocks per CU, and the same LDS plan within the CU's 160 KB.  The clip of the caller's rays (three
IEEE divisions in the source's `load`) and the surface fill must not cost that: the fill is a kernel of its own, k_surfaces, which has to stay out of scratch."""
import os
import re

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, blocks_per_cu_by_sgprs, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_persistent_ray_cast_fits_seven_waves_per_simd_and_the_surface_fill_has_no_scratch():
    assert ("phip_raycast.hip", [], "phip_raycast.o") in _ffi.UNITS
    res = resources("phip_raycast.hip")
    assert not any(name.startswith(("_Z8k_rays_w", "_Z11k_raycast_w")) for name in res), list(res)       # those stay phip.hip's
    k = next(v for name, v in res.items() if name.startswith("_Z11k_raycast_p"))
    src = open(os.path.join(_ffi.CSRC, "k_wide_node.h")).read() + open(os.path.join(_ffi.CSRC, "k_wide.h")).read()
    waves = int(re.search(r"#define WIDE_WAVES (\d+)", src).group(1))
    assert waves == 7
    assert k["scratch"] == 0, k
    assert k["vgprs"] <= 512 // waves // 8 * 8 == 72, k
    assert blocks_per_cu_by_sgprs(k["sgprs"]) >= waves, k
    stack = int(re.search(r"#define WIDE_STACK_LDS (\d+)", src).group(1)); cache = int(re.search(r"#define WIDE_NODE_CACHE_MAX (\d+)", src).group(1))
    deal = 4 * (64 * 8 + 64 * 8 + 256 * 2)                         # WD_WAVE_BYTES per wave, as in test_ray_kernel_of_the_big_scenes_fits_seven_waves_per_simd
    assert waves * (stack * 8 * 256 + cache * 80 + deal + k["lds"]) <= 160 * 1024
    s = next(v for name, v in res.items() if name.startswith("_Z10k_surfaces"))
    assert s["scratch"] == 0, s

"""Resources of the kernels of phip_mip_pyramid_device (phip_pyramid.hip), read from the compiler as tests/test_kernel_resources.py reads the others'; compile-only.

None of the three spills: the lane's eight weights live in registers (the tap loops are unrolled; no array is indexed by a variable).  k_pyramid_tail's LDS is the
named bound PYR_TAIL_LDS_BYTES of pyramid_hd.h, within the 160 KiB one workgroup may take on gfx950; the other two use none.  The VGPR counts are those DESIGN.md
3.20 records: a change of them is a change of the kernels."""
import os
import re

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

WORKGROUP_LDS = 160 * 1024
# kernel -> (VGPRs, LDS bytes)
KERNELS = {"_Z16k_pyramid_level0": (8, 0), "_Z14k_pyramid_pass": (38, 0), "_Z14k_pyramid_tail": (78, 65536)}


def test_pyramid_kernels_have_no_scratch_and_the_tail_fits_a_workgroup():
    assert ("phip_pyramid.hip", [], "phip_pyramid.o") in _ffi.UNITS
    res = resources("phip_pyramid.hip")
    assert len(res) == len(KERNELS), list(res)                      # the unit holds these kernels and nothing else
    header = open(os.path.join(_ffi.CSRC, "pyramid_hd.h")).read()
    bound = int(re.search(r"#define PYR_TAIL_LDS_BYTES (\d+)", header).group(1))
    for prefix, (vgprs, lds) in KERNELS.items():
        found = [v for name, v in res.items() if name.startswith(prefix)]
        assert len(found) == 1, (prefix, list(res))
        print(prefix, found[0])
        assert found[0]["scratch"] == 0, (prefix, found[0])
        assert found[0]["lds"] == lds, (prefix, found[0])
        assert found[0]["vgprs"] == vgprs, (prefix, found[0])
    assert KERNELS["_Z14k_pyramid_tail"][1] == bound <= WORKGROUP_LDS
    assert KERNELS["_Z14k_pyramid_tail"][0] <= 128                  # 1024 lanes = 4 waves per SIMD: at most 128 registers each

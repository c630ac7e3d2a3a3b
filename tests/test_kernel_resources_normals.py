"""Resources of the kernel of phip_vertex_normals_device (phip_normals.hip), read from the compiler as tests/test_kernel_resources.py reads the others'; compile-only.

k_vertex_normals does not spill and uses no LDS: the three corners are chosen by selects, no array is indexed by a variable.  The VGPR count is the one DESIGN.md
3.21 records (82: six waves per SIMD would take 80, the kernel runs at five); a change of it is a change of the kernel."""
import os

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# kernel -> (VGPRs, LDS bytes)
KERNELS = {"_Z16k_vertex_normals": (82, 0)}


def test_normals_kernel_has_no_scratch_and_no_lds():
    assert ("phip_normals.hip", [], "phip_normals.o") in _ffi.UNITS and len(_ffi.UNITS) == 50
    res = resources("phip_normals.hip")
    assert len(res) == len(KERNELS), list(res)                      # the unit holds this kernel and nothing else
    for prefix, (vgprs, lds) in KERNELS.items():
        found = [v for name, v in res.items() if name.startswith(prefix)]
        assert len(found) == 1, (prefix, list(res))
        print(prefix, found[0])
        assert found[0]["scratch"] == 0, (prefix, found[0])
        assert found[0]["lds"] == lds, (prefix, found[0])
        assert found[0]["vgprs"] == vgprs, (prefix, found[0])

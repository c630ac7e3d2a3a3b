"""Resources of the kernels of phip_scene_update_appearance (phip_appearance.hip), read from the compiler as tests/test_kernel_resources.py reads the others';
compile-only.

Every kernel is a one-lane-per-item pass (a conversion, a table look-up, a sequential sum over a row): none has a reason to spill and none uses LDS -- the wave
reduction of k_appearance_texmax runs on shuffles and ends in one atomicMax per wave."""
import os

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

KERNELS = ("_Z19k_appearance_texmax", "_Z19k_appearance_texels", "_Z17k_envmap_cdf_rows", "_Z21k_envmap_cdf_marginal", "_Z20k_appearance_records", "_Z20k_appearance_classes")


def test_appearance_kernels_have_no_scratch_and_no_lds():
    assert ("phip_appearance.hip", [], "phip_appearance.o") in _ffi.UNITS
    res = resources("phip_appearance.hip")
    assert len(res) == len(KERNELS), list(res)                      # the unit holds these kernels and nothing else
    for prefix in KERNELS:
        found = [v for name, v in res.items() if name.startswith(prefix)]
        assert len(found) == 1, (prefix, list(res))
        print(prefix, found[0])
        assert found[0]["scratch"] == 0, (prefix, found[0])
        assert found[0]["lds"] == 0, (prefix, found[0])
        assert found[0]["vgprs"] <= 64, (prefix, found[0])

"""Resources of the kernels of phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device (phip_shading_parts.hip), read from the compiler as
tests/test_kernel_resources.py reads the others'; compile-only.

Each kernel is one lane per item around the vertex's own BSDF and emitter functions, without the path state, the stream and the epilogue k_shade carries beside
them: no instantiation has a reason to spill.  The numbers below are the compiler's for this unit as recorded when it was written (VGPRs: 31 / 62 / 66 / 72 for
k_bsdf_parts<eval, sample> = <0,0> / <1,0> / <0,1> / <1,1>, 43 / 54 for k_emitter_sample<ENV = 0 / 1>, 31 / 39 for k_emitter_eval; no scratch anywhere), held as
upper bounds; 72 is also the most a 256-thread block may use and still run seven waves per SIMD.  The emitter kernels stage the emitter table in 4 KB of LDS
(EMITTER_LDS_FLOATS floats), the BSDF kernel uses none."""
import os
import re

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

VGPRS = {("k_bsdf_parts", "00"): 31, ("k_bsdf_parts", "10"): 62, ("k_bsdf_parts", "01"): 66, ("k_bsdf_parts", "11"): 72,
         ("k_emitter_sample", "0"): 43, ("k_emitter_sample", "1"): 54, ("k_emitter_eval", "0"): 31, ("k_emitter_eval", "1"): 39}


def test_the_unit_compiles_and_no_instantiation_spills():
    assert ("phip_shading_parts.hip", [], "phip_shading_parts.o") in _ffi.UNITS
    res = resources("phip_shading_parts.hip")
    seen = {}
    for name, v in res.items():
        m = re.match(r"_Z\d+(k_bsdf_parts|k_emitter_sample|k_emitter_eval)I((?:Lb[01]E)+)E", name)
        assert m, name                                             # the unit holds these kernels and nothing else (no k_shade, no shadeVertex instantiation)
        seen[m.group(1), "".join(re.findall(r"Lb([01])E", m.group(2)))] = v
    assert sorted(seen) == sorted(VGPRS), sorted(seen)
    for key, v in sorted(seen.items()):
        print(key, v)
        assert v["scratch"] == 0, (key, v)
        assert v["vgprs"] <= VGPRS[key], (key, v)
        assert v["lds"] == (0 if key[0] == "k_bsdf_parts" else 4096), (key, v)
    # sampling code is compiled only where a sample is asked for: the eval-only build is smaller than the ones that sample, wi alone smaller still
    assert seen["k_bsdf_parts", "00"]["vgprs"] < seen["k_bsdf_parts", "10"]["vgprs"] <= seen["k_bsdf_parts", "11"]["vgprs"]

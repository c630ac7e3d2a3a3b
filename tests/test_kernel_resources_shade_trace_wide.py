"""Register and LDS budget of k_shade_trace_w (k_shade_trace_w.h), read from the compiler as tests/test_kernel_resources.py does (cross-compiles, no GPU).

The kernel's grid is its resident set, and what bounds that is a block's LDS: the four waves' task stacks, the staged top of the tree, the waves' ray tables and pair
lists under the class deal's exchange buffer, and the scene tables -- about 40 KB, four blocks per CU.  So the launch bound is four waves per SIMD (<= 128 VGPRs);
the scratch the vertex code parks at that bound is recorded here per feature set, as achieved."""
import concurrent.futures
import os
import re

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# bytes of scratch per lane as the compiler prints them, the larger of the builds without / with strictNormals: {feature set: (diffuse only, all three BSDF models)} --
# the table of DESIGN.md 3.5 (profiles/r07_shade_trace_wide_resources.txt has all 24 lines).  What was achieved, pinned so that a change that costs more is seen
SCRATCH = {0: (12, 104), 8: (84, 148), 1: (104, 164), 2: (172, 276), 3: (188, 320), 11: (224, 356)}


def test_every_instantiation_keeps_four_blocks_per_cu():
    units = [u for u in _ffi.UNITS if u[0] == "phip_shade_w.hip"]
    assert sorted(int(re.search(r"-DSHADE_FEAT=(\d+)", " ".join(u[1])).group(1)) for u in units) == sorted(_ffi.SHADE_FEATS)
    src = open(os.path.join(_ffi.CSRC, "k_wide_wave.h")).read() + open(os.path.join(_ffi.CSRC, "k_pool.h")).read() + open(os.path.join(_ffi.CSRC, "k_shade_trace_w.h")).read()
    waves = int(re.search(r"#define SHADE_TRACE_W_WAVES (\d+)", src).group(1))
    cap = int(re.search(r"#define WP_CAP (\d+)u", src).group(1)); pairs = int(re.search(r"#define WP_PAIRS (\d+)u", src).group(1))
    cache = int(re.search(r"#define MEGA_WIDE_NODE_CACHE (\d+)u", src).group(1))
    deal = 256 * (16 + 16 + 16 + 16 + 8 + 4)                                   # SHADE_DEAL_BYTES
    tables = 1024 * 4 + 48 * 96                                                # EMITTER_LDS_FLOATS floats + MATERIAL_LDS_MAX materials
    dyn = 4 * cap * 8 + cache * 80 + max(deal, 4 * (128 * 8 + 64 * 8 + 64 * 32 + pairs * 4)) + tables
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 2)) as pool:
        results = list(pool.map(lambda u: resources(u[0], u[1]), units))
    seen = 0
    for u, res in zip(units, results):
        feat = int(re.search(r"-DSHADE_FEAT=(\d+)", " ".join(u[1])).group(1))
        ks = {n: v for n, v in res.items() if n.startswith("_Z15k_shade_trace_w")}
        assert len(ks) == 4, (feat, list(ks))                                  # {diffuse only, all models} x strictNormals
        for name, v in sorted(ks.items()):
            mm = int(re.match(r"_Z15k_shade_trace_wILi(\d)E", name).group(1))
            print("k_shade_trace_w FEAT %2d %s: %d VGPRs, %d SGPRs, %d B scratch, %d B static LDS" % (feat, name[19:35], v["vgprs"], v["sgprs"], v["scratch"], v["lds"]))
            assert v["vgprs"] <= 512 // waves, (name, v)
            assert v["scratch"] <= SCRATCH[feat][1 if mm else 0], (name, v)
            assert waves * (v["lds"] + dyn) <= 160 * 1024, (name, v, dyn)
            seen += 1
    assert waves == 4 and seen == 24

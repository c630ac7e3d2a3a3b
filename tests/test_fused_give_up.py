"""A fused pass that gives up (k_mega.h, k_wide_wave.h, phip.hip), checked without a GPU: the test libraries build, the give-up signal is a row of its own and
not a poison added to the sample count, the task stack of traceWidePool is bounded, and the product compiles none of the fault-injection knobs.  The GPU side --
every way of giving up against the product's frame, bit for bit -- is in tests/test_gpu_parity.py."""
import os
import re

import pytest

from mitsuba_amd import _ffi

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def source(name):
    return open(os.path.join(_ffi.CSRC, name)).read()


def code(name):
    """the file without its comments"""
    s = re.sub(r"/\*.*?\*/", "", source(name), flags=re.S)
    return re.sub(r"//[^\n]*", "", s)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("tag", sorted(_ffi.TEST_VARIANTS))
def test_every_test_variant_builds(tag):
    """__graft_entry__.build() makes every library of _ffi.TEST_VARIANTS; the call returns at once when the file carries the current build id"""
    path = _ffi.build_test_variant(tag)
    assert os.path.exists(path) and _ffi.built_id(path), path


def test_the_overflow_variant_shrinks_both_caps_of_the_task_stack():
    flags = _ffi.TEST_VARIANTS["overflow"].split()
    caps = dict(f[2:].split("=") for f in flags if f.startswith("-D"))
    assert set(caps) == {"WP_CAP", "WP_SPILL_CAP"}, caps
    # roots of one traversal: up to 64 closest-hit + 64 any-hit rays fit; their children do not
    assert int(caps["WP_CAP"].rstrip("u")) + int(caps["WP_SPILL_CAP"].rstrip("u")) == 128
    src = source("k_wide_wave.h")
    assert re.search(r"#ifndef WP_SPILL_CAP\s*\n#define WP_SPILL_CAP \(64u \* SPILL_DEPTH / 2u\)", src), "the product's spill cap is the wave's whole share"
    assert "wp.spillCap = WP_SPILL_CAP;" in src


def test_k_mega_no_longer_poisons_the_sample_row():
    """A wave that gave up used to add 2^62 to its ST_SAMPLES entry: four such waves sum to 0 modulo 2^64.  It now sets its entry of ST_GAVE_UP."""
    k = code("k_mega.h")
    assert not re.search(r"<<\s*6[0-3]\b", k), "a poison constant in k_mega.h"
    assert "poison" not in k
    samples_row = re.search(r"waveStat\(P, rows\[i\], waveId, ([^;]*)\);", k)
    assert samples_row and samples_row.group(1).strip() == "val", samples_row and samples_row.group(1)
    assert re.search(r"if \(gaveUp && lane == 0u\) P\.stat\[\(size_t\) ST_GAVE_UP \* P\.nWaves \+ waveId\] = 1ull;", k)
    pool = code("k_pool.h")
    assert re.search(r"ST_SAMPLES, ST_ALIVE, ST_GAVE_UP, ST_COUNT", pool)
    host = code("host_render.h")
    assert "hc.total[ST_SAMPLES] > rc.totalIds" not in host
    assert re.search(r"gaveUp \|\| \(countKnown && hc\.total\[ST_SAMPLES\] != samplesTotal \* rc\.sppPass\)", host)
    assert re.search(r"#else\s*const bool countKnown = true;", host)


def test_trace_wide_pool_reads_no_stack_entry_past_its_room():
    """traceWidePool: a push past room used to be dropped while `count` grew, and the pops read the words behind the wave's slice of the spill buffer as node
    indices.  Now the count is checked after the roots and after every push: past room the wave drops its tasks and pairs and leaves the loop; poolRead is bounded."""
    k = code("k_wide_wave.h")
    body = k[k.index("void traceWidePool("):]
    body = body[:body.index("#undef WP_FETCH_RAY")]
    read = body[body.index("auto poolRead"):body.index("};", body.index("auto poolRead"))]
    assert "if (i - WP_CAP >= wp.spillCap) return make_uint2(0u, 0u);" in read
    assert read.index("i - WP_CAP >= wp.spillCap") < read.index("wp.spill + (i - WP_CAP)")
    loop = body[body.index("while (count | nQ)"):]
    roots = body[:body.index("while (count | nQ)")]
    assert re.search(r"if \(count > room \|\| __any\(overflow\)\) \{ overflow = true; count = 0u; \}", roots)
    drain = re.search(r"if \(count > room \|\| __any\(overflow\)\) \{ overflow = true; count = 0u; nQ = 0u; \}", loop)
    assert drain, "no drain after the push"
    assert drain.start() > loop.index("count += nRest")               # after the last push of the iteration ...
    assert drain.start() < loop.index("const uint32_t nTest")           # ... before the next read of the stack or the pair queue
    assert re.search(r"if \(__any\(overflow\)\) \{ overflow = true; goS = goC = false; \}", roots)     # a wave that overflowed traces nothing more


def test_fault_knobs_are_compiled_only_into_the_fault_build():
    """Every line of the sources that names a PHIP_TEST_FAULT_* knob, or a MegaParams fault field, sits inside an #if MEGA_MB_FAULT block"""
    for name in sorted(os.listdir(_ffi.CSRC)):
        if not name.endswith((".hip", ".h", ".inl")):
            continue
        stack = []
        for no, line in enumerate(source(name).splitlines(), 1):
            t = line.strip()
            if re.match(r"#\s*if", t):
                stack.append(t)
            elif re.match(r"#\s*endif", t):
                stack.pop()
            elif re.search(r"PHIP_TEST_FAULT|\bfaultWaves\b|\bfaultShort\b|\bfaultPass\b|\bfaulty\b", t) and not t.startswith(("/*", "*")):
                assert any(re.match(r"#\s*if MEGA_MB_FAULT\b", c) for c in stack), "%s:%d: %s" % (name, no, t)
        assert not stack, name

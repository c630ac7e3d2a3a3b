"""phip_radiance_device without a GPU: its place in the ABI, the checks of its arguments that need no device -- through phip_debug_host_radiance_args, the debug
library's hook on the function the entry point itself calls first (host_radiance.h: radianceArgsError) -- and the ValueErrors of PathHIP.radiance."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi
from mitsuba_amd.integrator import PathHIP

HERE = os.path.dirname(os.path.abspath(__file__))


def test_abi_of_phip_radiance_device(phip, have_gpu):
    header = open(os.path.join(HERE, "..", "include", "phip.h")).read()
    assert "int  phip_radiance_device(phip_scene *scene, const phip_render_params *params, const phip_radiance_desc *desc, phip_stats *out_stats" in header
    assert "} phip_radiance_desc;" in header and "#define PHIP_ABI_VERSION 7" in header            # one function, one struct: no struct of the ABI changed
    assert phip.phip_abi_sizeof(15) == C.sizeof(A.phip_radiance_desc) == 40
    assert phip.phip_abi_sizeof(14) == 0 and phip.phip_abi_sizeof(16) == 0 and phip.phip_abi_sizeof(6) == C.sizeof(A.phip_render_params)
    f = {n: getattr(A.phip_radiance_desc, n).offset for n, _ in A.phip_radiance_desc._fields_}
    assert f == dict(d_rays=0, n=8, d_stream=16, first_stream=24, reserved=28, d_out=32)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB], capture_output=True, text=True).stdout
    assert " phip_radiance_device" in out and "phip_debug_" not in out
    units = [u for u in _ffi.UNITS if u[0] == "phip_shade_r.hip"]
    assert sorted(u[2] for u in units) == sorted("phip_radiance%d_%d.o" % (f_, q) for f_ in range(4) for q in range(2))      # units of its own
    p = A.default_render_params(spp=1)
    d = A.phip_radiance_desc()
    assert phip.phip_radiance_device(None, None, None, None) == A.PHIP_ERR_INVALID
    assert phip.phip_radiance_device(None, C.byref(p), C.byref(d), None) == A.PHIP_ERR_INVALID     # no scene
    if not have_gpu:
        never_read = C.create_string_buffer(64)
        d = A.phip_radiance_desc(d_rays=C.addressof(never_read), n=1, d_out=C.addressof(never_read))
        assert phip.phip_radiance_device(C.cast(never_read, C.c_void_p), C.byref(p), C.byref(d), None) == A.PHIP_ERR_DEVICE      # no CPU fallback
        assert phip.phip_last_error()


def check(phip, desc_kw=None, **kw):
    p = A.default_render_params(spp=1, **kw)
    buf = 4096                                                     # never dereferenced: the hook looks at values only
    d = A.phip_radiance_desc(**dict(dict(d_rays=buf, n=16, d_stream=None, first_stream=0, reserved=0, d_out=buf), **(desc_kw or {})))
    rc = phip.phip_debug_host_radiance_args(C.byref(p), C.byref(d))
    assert (rc == 0) or _ffi.debug_lib().phip_last_error().startswith(b"phip_radiance_device: ")      # (the hook's library keeps its own error text)
    return rc


def test_argument_checks_that_need_no_device(phip):
    assert check(phip) == 0
    assert check(phip, integrator=A.PHIP_INTEGRATOR_VOLPATH_SIMPLE) == 0
    assert check(phip, integrator=A.PHIP_INTEGRATOR_DIRECT) == A.PHIP_ERR_UNSUPPORTED
    for sampler in (A.PHIP_SAMPLER_LD, A.PHIP_SAMPLER_SOBOL, A.PHIP_SAMPLER_STRATIFIED, A.PHIP_SAMPLER_HALTON, A.PHIP_SAMPLER_HAMMERSLEY):
        assert check(phip, sampler=sampler) == A.PHIP_ERR_UNSUPPORTED
    assert check(phip, sampler=6) == A.PHIP_ERR_INVALID and check(phip, integrator=3) == A.PHIP_ERR_INVALID
    assert check(phip, devices=[0]) == 0 and check(phip, devices=[0, 1]) == A.PHIP_ERR_INVALID
    assert check(phip, flags=A.PHIP_FLAG_SAMPLE_BUFFER) == A.PHIP_ERR_INVALID and check(phip, flags=A.PHIP_FLAG_ACCUMULATE) == A.PHIP_ERR_INVALID
    assert check(phip, flags=A.PHIP_FLAG_KERNEL_TIMING | A.PHIP_FLAG_NO_FUSED) == 0
    assert check(phip, dict(n=2 ** 32 - 256)) == 0 and check(phip, dict(n=2 ** 32 - 255)) == A.PHIP_ERR_INVALID
    assert check(phip, dict(d_rays=4096 + 4)) == A.PHIP_ERR_INVALID and check(phip, dict(d_out=4096 + 8)) == A.PHIP_ERR_INVALID
    assert check(phip, dict(d_stream=4096 + 4)) == 0 and check(phip, dict(d_stream=4096 + 2)) == A.PHIP_ERR_INVALID
    assert check(phip, dict(d_rays=None)) == A.PHIP_ERR_INVALID and check(phip, dict(d_out=None)) == A.PHIP_ERR_INVALID
    assert check(phip, dict(n=0, d_rays=None, d_out=None)) == 0                                    # n == 0: no pointer is looked at
    assert phip.phip_debug_host_radiance_args(None, None) == A.PHIP_ERR_INVALID


def test_wrapper_refuses_tensors_it_cannot_pass_on():
    torch = pytest.importorskip("torch")
    scene = types.SimpleNamespace(device=0)
    good = torch.zeros((4, 8), dtype=torch.float32)
    for bad in (good.double(), torch.zeros((4, 16))[:, :8], good.reshape(-1), torch.zeros((4, 7)), np.zeros((4, 8), np.float32), good):      # (good: not on the device)
        with pytest.raises(ValueError):
            PathHIP().radiance(scene, bad, 1)
    assert PathHIP.radiance.__code__.co_varnames[:6] == ("self", "scene", "rays", "spp", "seed", "stream_ids")


def _tokens(text):
    import re
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split()


def _between(text, start, end="\n}\n"):
    i = text.index(start)
    return text[i:text.index(end, i)]


def test_the_copies_in_k_shade_r_differ_from_their_originals_in_the_sample_source_only():
    """k_shade_r.h holds copies of shadeEpilogue and of k_shade's body (why: its header).  A fix to the shadow compaction, the dynamic tail, the retirement or the
    kernel's head has to reach both: with the comments taken out, the two texts may differ in the runs of tokens listed here -- the source of samples -- and nowhere else."""
    import difflib
    a = open(os.path.join(_ffi.CSRC, "k_shade.h")).read(); b = open(os.path.join(_ffi.CSRC, "k_shade_r.h")).read()
    want = {("void shadeEpilogue(", "void shadeEpilogueRays("): [
                ("shadeEpilogue(const", "shadeEpilogueRays(const RaySamples &src, const"),
                ("for (;;) {", ""), ("{", ""),
                ("break; } uint32_t px, py, k; if (decodeId(rc, S.film, id, px, py, k)) {", "else"),
                ("break; } id += P.capacity; }", ""),
                ("uint32_t px, py, k;", ""), ("if (decodeId(rc, S.film, id, px, py, k)) {", ""), ("}", ""),
                ("px, py,", ""), ("decodeId(rc, S.film, newId, px, py, k);", ""),
                ("cameraSample<QMC>(S, rc,", "src.sample(rc,"), ("px, py,", "pixel,"), ("pixel,", "")],
            ("void k_shade(DevScene S", "void k_shade_r(DevScene S"): [
                ("k_shade(DevScene", "k_shade_r(DevScene"), ("*L)", "*L, RaySamples src)"),
                ("FEAT>(S,", "FEAT | SHADE_FEAT_NO_DIFFERENTIALS>(S,"),
                ("shadeEpilogue<(FEAT & 8) != 0>(S,", "shadeEpilogueRays(src, S,"), ("blockIdx.x);", "blockIdx.x, nullptr);")]}
    for (sa, sb_), runs in want.items():
        ta, tb = _tokens(_between(a, sa)), _tokens(_between(b, sb_))
        assert len(ta) > 300 or sa.startswith("void k_shade(")
        got = [(" ".join(ta[i1:i2]), " ".join(tb[j1:j2])) for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, ta, tb, autojunk=False).get_opcodes() if op != "equal"]
        assert got == runs, got

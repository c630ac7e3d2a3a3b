"""phip_camera_rays_device, phip_film_device and the (key, sample) pairs of phip_radiance_device without a GPU: their place in the ABI, and the checks of their
arguments that need no device -- through phip_debug_host_camera_rays_args / phip_debug_host_film_args / phip_debug_host_radiance_args, the debug library's hooks on
the functions the entry points themselves call first (host_camera_film.h: cameraRaysArgsError, filmArgsError; host_radiance.h: radianceArgsError)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi
from mitsuba_amd.integrator import PathHIP, Scene

HERE = os.path.dirname(os.path.abspath(__file__))
BUF = 4096                                                         # never dereferenced: the hooks look at values only


def test_abi_of_the_two_entry_points(phip, have_gpu):
    header = open(os.path.join(HERE, "..", "include", "phip.h")).read()
    assert "int  phip_camera_rays_device(phip_scene *scene, const phip_render_params *params, const phip_camera_rays_desc *desc);" in header
    assert "int  phip_film_device(phip_scene *scene, const phip_render_params *params, const phip_film_desc *desc, phip_stats *out_stats" in header
    assert "} phip_camera_rays_desc;" in header and "} phip_film_desc;" in header and "#define PHIP_ABI_VERSION 7" in header
    assert "#define PHIP_RADIANCE_STREAM_PAIRS 1u" in header and "#define PHIP_FILM_SIGNED 1u" in header and "uint32_t        stream_layout;" in header
    assert phip.phip_abi_sizeof(17) == C.sizeof(A.phip_camera_rays_desc) == 40
    assert phip.phip_abi_sizeof(18) == C.sizeof(A.phip_film_desc) == 24
    assert phip.phip_abi_sizeof(14) == 0 and phip.phip_abi_sizeof(16) == 0 and phip.phip_abi_sizeof(19) == 0
    assert phip.phip_abi_sizeof(15) == C.sizeof(A.phip_radiance_desc) == 40 and phip.phip_abi_sizeof(6) == C.sizeof(A.phip_render_params)      # nothing else moved
    offsets = lambda s: {n: getattr(s, n).offset for n, _ in s._fields_}
    assert offsets(A.phip_camera_rays_desc) == dict(d_pixels=0, m=8, d_rays=16, d_keys=24, d_positions=32)
    assert offsets(A.phip_film_desc) == dict(d_values=0, d_out=8, flags=16, reserved=20)
    assert offsets(A.phip_radiance_desc)["reserved"] == 28 and A.PHIP_RADIANCE_STREAM_PAIRS == 1 and A.PHIP_FILM_SIGNED == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB], capture_output=True, text=True).stdout
    assert " phip_camera_rays_device" in out and " phip_film_device" in out and "phip_debug_" not in out
    assert ("phip_camera_film.hip", [], "phip_camera_film.o") in _ffi.UNITS                                    # a unit of its own
    for name in ("phip_camera_film.hip", "host_camera_film.h", "k_camera_film.h"):
        assert os.path.exists(os.path.join(_ffi.CSRC, name)), name
    p = A.default_render_params(spp=1)
    assert phip.phip_camera_rays_device(None, None, None) == A.PHIP_ERR_INVALID and phip.phip_film_device(None, None, None, None) == A.PHIP_ERR_INVALID
    cr = A.phip_camera_rays_desc(d_rays=BUF); fd = A.phip_film_desc(d_values=BUF, d_out=BUF)
    assert phip.phip_camera_rays_device(None, C.byref(p), C.byref(cr)) == A.PHIP_ERR_INVALID                   # no scene
    assert phip.phip_film_device(None, C.byref(p), C.byref(fd), None) == A.PHIP_ERR_INVALID
    if not have_gpu:
        never_read = C.create_string_buffer(64)
        scene = C.cast(never_read, C.c_void_p)
        assert phip.phip_camera_rays_device(scene, C.byref(p), C.byref(cr)) == A.PHIP_ERR_DEVICE               # no CPU fallback
        assert phip.phip_film_device(scene, C.byref(p), C.byref(fd), None) == A.PHIP_ERR_DEVICE
        assert phip.phip_last_error()


def rays_check(phip, desc_kw=None, **kw):
    p = A.default_render_params(**dict(dict(spp=3), **kw))
    d = A.phip_camera_rays_desc(**dict(dict(d_pixels=None, m=0, d_rays=BUF, d_keys=None, d_positions=None), **(desc_kw or {})))
    rc = phip.phip_debug_host_camera_rays_args(C.byref(p), C.byref(d))
    assert (rc == 0) or _ffi.debug_lib().phip_last_error().startswith(b"phip_camera_rays_device: ")
    return rc


def film_check(phip, desc_kw=None, **kw):
    p = A.default_render_params(**dict(dict(spp=3), **kw))
    d = A.phip_film_desc(**dict(dict(d_values=BUF, d_out=BUF, flags=0, reserved=0), **(desc_kw or {})))
    rc = phip.phip_debug_host_film_args(C.byref(p), C.byref(d))
    assert (rc == 0) or _ffi.debug_lib().phip_last_error().startswith(b"phip_film_device: ")
    return rc


def radiance_check(phip, desc_kw=None, **kw):
    p = A.default_render_params(spp=1, **kw)
    d = A.phip_radiance_desc(**dict(dict(d_rays=BUF, n=16, d_stream=BUF, first_stream=0, reserved=A.PHIP_RADIANCE_STREAM_PAIRS, d_out=BUF), **(desc_kw or {})))
    return phip.phip_debug_host_radiance_args(C.byref(p), C.byref(d))


QMC = (A.PHIP_SAMPLER_LD, A.PHIP_SAMPLER_SOBOL, A.PHIP_SAMPLER_STRATIFIED, A.PHIP_SAMPLER_HALTON, A.PHIP_SAMPLER_HAMMERSLEY)


def test_camera_rays_argument_checks_that_need_no_device(phip):
    INV, UNS = A.PHIP_ERR_INVALID, A.PHIP_ERR_UNSUPPORTED
    assert rays_check(phip) == 0
    assert rays_check(phip, dict(d_keys=BUF + 8, d_positions=BUF + 24, d_pixels=BUF + 4, m=7)) == 0
    assert rays_check(phip, dict(d_rays=None)) == INV
    assert rays_check(phip, dict(d_rays=BUF + 8)) == INV and rays_check(phip, dict(d_keys=BUF + 4)) == INV and rays_check(phip, dict(d_positions=BUF + 4)) == INV
    assert rays_check(phip, dict(d_pixels=BUF + 2, m=1)) == INV
    assert rays_check(phip, dict(d_pixels=BUF, m=0, d_rays=None)) == 0                           # an empty list: no pointer is looked at
    for sampler in QMC:
        assert rays_check(phip, sampler=sampler) == UNS
    assert rays_check(phip, sampler=6) == INV
    assert rays_check(phip, devices=[0]) == 0 and rays_check(phip, devices=[0, 1]) == INV
    assert rays_check(phip, spp=0) == INV and rays_check(phip, sample_offset=-1) == INV and rays_check(phip, sample_offset=5) == 0
    assert rays_check(phip, dict(d_pixels=BUF, m=(2 ** 32 - 256) // 3)) == 0 and rays_check(phip, dict(d_pixels=BUF, m=(2 ** 32 - 256) // 3 + 1)) == INV
    assert rays_check(phip, shard_count=2, flags=A.PHIP_FLAG_ACCUMULATE) == 0                    # what concerns the film is not read
    assert phip.phip_debug_host_camera_rays_args(None, None) == INV


def test_film_argument_checks_that_need_no_device(phip):
    INV, UNS = A.PHIP_ERR_INVALID, A.PHIP_ERR_UNSUPPORTED
    assert film_check(phip) == 0
    assert film_check(phip, dict(flags=A.PHIP_FILM_SIGNED), flags=A.PHIP_FLAG_ACCUMULATE | A.PHIP_FLAG_KERNEL_TIMING, block_size=8, sample_offset=5) == 0
    assert film_check(phip, dict(d_values=None)) == INV and film_check(phip, dict(d_out=None)) == INV
    assert film_check(phip, dict(d_values=BUF + 8)) == INV and film_check(phip, dict(d_out=BUF + 4)) == INV
    assert film_check(phip, dict(flags=2)) == INV
    for sampler in QMC:
        assert film_check(phip, sampler=sampler) == UNS
    assert film_check(phip, sampler=6) == INV
    assert film_check(phip, shard_count=2) == INV and film_check(phip, shard_count=1) == 0 and film_check(phip, shard_count=0) == 0
    assert film_check(phip, devices=[0, 1]) == INV
    assert film_check(phip, spp=0) == INV and film_check(phip, sample_offset=-1) == INV
    assert film_check(phip, block_size=24) == INV and film_check(phip, block_size=256) == INV and film_check(phip, block_size=1) == INV
    assert phip.phip_debug_host_film_args(None, None) == INV


def test_pairs_argument_checks_that_need_no_device(phip):
    INV = A.PHIP_ERR_INVALID
    assert radiance_check(phip) == 0
    assert radiance_check(phip, sample_offset=1, sample_total=4) == INV                          # the sample index is the pair's
    assert radiance_check(phip, dict(d_stream=None)) == INV
    assert radiance_check(phip, dict(d_stream=BUF + 4)) == INV                                   # pairs are 8-byte aligned
    assert radiance_check(phip, dict(reserved=2)) == INV and radiance_check(phip, dict(reserved=2, d_stream=None)) == INV      # an unknown layout
    assert radiance_check(phip, dict(n=0, d_rays=None, d_out=None, d_stream=None)) == 0          # n == 0: no pointer is looked at
    assert radiance_check(phip, dict(reserved=0, d_stream=BUF + 4), sample_offset=1, sample_total=4) == 0      # layout 0 is what it was
    assert radiance_check(phip, sampler=A.PHIP_SAMPLER_SOBOL) == A.PHIP_ERR_UNSUPPORTED


def test_wrappers_refuse_tensors_they_cannot_pass_on():
    torch = pytest.importorskip("torch")
    scene = types.SimpleNamespace(device=0, width=4, height=2, block_size=32)
    good = torch.zeros((8, 8), dtype=torch.float32)
    with pytest.raises(ValueError):
        PathHIP().radiance(scene, good, 1, pairs=torch.zeros((8, 2), dtype=torch.int32))         # (the rays: not on the device)
    for bad in (torch.zeros((8, 3, 4)).double(), torch.zeros((8, 3, 8))[..., :4], torch.zeros((8, 2, 4)), np.zeros((8, 3, 4), np.float32), torch.zeros((8, 3, 4))):
        with pytest.raises(ValueError):
            Scene.film(scene, bad, 3)
    for bad in (torch.zeros(4), torch.zeros((2, 2), dtype=torch.int32), np.zeros(4, np.int32), torch.zeros(4, dtype=torch.int32)):      # (the last: not on the device)
        with pytest.raises(ValueError):
            Scene.camera_rays(scene, 1, pixels=bad)
    assert PathHIP.radiance.__code__.co_varnames[:10] == ("self", "scene", "rays", "spp", "seed", "stream_ids", "first_stream", "flags", "stream", "pairs")

"""The argument checks at the C boundary (mitsuba_amd/csrc/phip.hip): every entry point that takes pointers refuses NULL with PHIP_ERR_INVALID and the
text phip_last_error() has always had for it, and phip_scene_replicate refuses a device count outside [1, PHIP_MAX_DEVICES].  Each of these checks returns
before the first HIP call and before the scene handle is looked into, so the file needs no device: the `scene` below is memory that is never read."""
import ctypes as C

import pytest

from mitsuba_amd import _abi as A


@pytest.fixture(scope="module")
def lib(phip):
    return phip


@pytest.fixture(scope="module")
def scene():
    """a non-NULL handle for the checks that come before any use of it"""
    buf = C.create_string_buffer(1 << 16)
    return C.c_void_p(C.addressof(buf)), buf


def err(lib):
    return lib.phip_last_error().decode()


def test_scene_create_refuses_a_null_description(lib):
    assert not lib.phip_scene_create(None, 0)
    assert err(lib) == "desc is NULL"


def test_render_entry_points_refuse_null_arguments(lib, scene):
    h, _ = scene
    p = A.default_render_params(spp=1)
    out = (C.c_float * 5)()
    st = A.phip_stats()
    fp = C.cast(out, C.POINTER(C.c_float))
    for args in [(None, C.byref(p), fp, C.byref(st)), (h, None, fp, C.byref(st)), (h, C.byref(p), None, C.byref(st)), (None, None, None, None)]:
        lib.phip_scene_create(None, 0)                                       # (another text in between: the next one is this call's)
        assert lib.phip_render(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "NULL argument"
    for args in [(None, C.byref(p), C.c_void_p(C.addressof(out)), C.byref(st)), (h, None, C.c_void_p(C.addressof(out)), C.byref(st)), (h, C.byref(p), None, C.byref(st)),
                 (None, None, None, None)]:
        lib.phip_scene_create(None, 0)
        assert lib.phip_render_device(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "NULL argument"


def test_film_samples_and_trace_refuse_null_arguments(lib, scene):
    h, _ = scene
    out = (C.c_float * 5)()
    fp = C.cast(out, C.POINTER(C.c_float))
    for args in [(None, C.c_void_p(C.addressof(out)), C.c_void_p(C.addressof(out))), (h, None, C.c_void_p(C.addressof(out))), (h, C.c_void_p(C.addressof(out)), None)]:
        lib.phip_scene_create(None, 0)
        assert lib.phip_film_to_host(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "NULL argument"
    for args in [(None, fp, 1), (h, None, 1)]:
        lib.phip_scene_create(None, 0)
        assert lib.phip_get_samples(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "NULL argument"
    ray = A.phip_ray()
    for args in [(None, C.byref(ray), 1, None, None, None), (h, None, 1, None, None, None)]:
        lib.phip_scene_create(None, 0)
        assert lib.phip_trace(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "NULL argument"
    info = A.phip_accel_info()
    for args in [(None, C.byref(info)), (h, None)]:
        lib.phip_scene_create(None, 0)
        assert lib.phip_scene_accel_info(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "NULL argument"


def test_scene_replicate_refuses_null_and_a_device_count_out_of_range(lib, scene):
    h, _ = scene
    devs = (C.c_int32 * (A.PHIP_MAX_DEVICES + 1))()
    for args in [(None, devs, 1), (h, None, 1)]:
        lib.phip_scene_create(None, 0)
        assert lib.phip_scene_replicate(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "NULL argument"
    for args in [(h, devs, 0), (h, None, 0), (h, devs, A.PHIP_MAX_DEVICES + 1), (h, devs, -1)]:
        lib.phip_scene_create(None, 0)
        assert lib.phip_scene_replicate(*args) == A.PHIP_ERR_INVALID
        assert err(lib) == "n_devices out of range"


def test_cancel_and_destroy_accept_null(lib):
    lib.phip_cancel(None)
    lib.phip_scene_destroy(None)

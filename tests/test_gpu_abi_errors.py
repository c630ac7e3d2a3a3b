"""The error paths of the C boundary that need a device to be reached, and the replica set behind a device list (mitsuba_amd/csrc/phip.hip: guarded,
host_scene.h: ensureReplicas), on a 32 x 32 Cornell box at 1 spp.  Every refusal is an argument error that returns before a launch.  The codes and texts are
those the boundary had before its six catch ladders became one guard: tests/test_gpu_parity.py::test_error_behaviour and
tests/test_gpu_round2.py::test_multi_device_render_equals_the_single_device_frame / test_scene_replicate hold that these calls fail, not with what."""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi, scene as S

pytestmark = pytest.mark.gpu

W = 32


@pytest.fixture(scope="module")
def box(phip, gauss):
    """(library, scene, number of visible devices, the single-device frame and its samples)"""
    if phip.phip_device_count() <= 0:
        pytest.fail("no HIP device visible: " + phip.phip_last_error().decode())
    from mitsuba_amd.integrator import Scene
    gs = Scene(S.cornell_box(W, W, gauss).desc())
    rc, frame, st = render(phip, gs)
    assert rc == A.PHIP_OK and st.n_devices == 1
    frame.setflags(write=False)
    yield phip, gs, phip.phip_device_count(), frame, st.samples
    gs.close()


def render(phip, gs, **kw):
    p = A.default_render_params(spp=1, max_depth=5, **kw)
    out = np.zeros((W, W, 5), np.float32)
    st = A.phip_stats()
    rc = phip.phip_render(gs._h, C.byref(p), _ffi.fptr(out), C.byref(st))
    return rc, out, st


def replicate(phip, gs, devices):
    return phip.phip_scene_replicate(gs._h, (C.c_int32 * len(devices))(*devices), len(devices))


def same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all()


def test_scene_description_of_another_abi_version_is_refused(box, gauss):
    """a std::runtime_error of the scene build: PHIP_ERR_INVALID in the create mapping (std::invalid_argument, a scene the back end does not serve, is
    PHIP_ERR_UNSUPPORTED) -- phip_scene_create itself can only return NULL, what it recorded is the text"""
    phip = box[0]
    d = S.cornell_box(W, W, gauss).desc()
    d.abi_version = A.PHIP_ABI_VERSION + 1
    assert not phip.phip_scene_create(C.byref(d), 0)
    assert phip.phip_last_error().decode() == "phip_scene_desc.abi_version mismatch"


def test_render_refuses_a_device_list_out_of_range_or_with_a_device_twice(box):
    phip, gs, visible, frame, samples = box
    rc, _, _ = render(phip, gs, devices=[0, visible])
    assert rc == A.PHIP_ERR_INVALID
    assert phip.phip_last_error().decode() == "device ordinal out of range"
    rc, _, _ = render(phip, gs, devices=[0, visible], flags=A.PHIP_FLAG_ALIAS_DEVICES)
    assert rc == A.PHIP_ERR_INVALID
    assert phip.phip_last_error().decode() == "device ordinal out of range"
    rc, _, _ = render(phip, gs, devices=[0, 0])
    assert rc == A.PHIP_ERR_INVALID
    assert phip.phip_last_error().decode() == "a device is listed twice (PHIP_FLAG_ALIAS_DEVICES allows it for tests)"
    rc, _, _ = render(phip, gs, devices=[visible, 0])
    assert rc == A.PHIP_ERR_INVALID
    assert phip.phip_last_error().decode() == "devices[0] must be the scene's device"
    # the refused calls left the scene as it was
    rc, again, st = render(phip, gs)
    assert rc == A.PHIP_OK and st.n_devices == 1 and st.samples == samples and same_bits(again, frame)


def test_aliased_device_list_gives_the_single_device_frame(box):
    """the film is one block: the second position of the list has no block of it, and the merge adds a film of zeros"""
    phip, gs, visible, frame, samples = box
    rc, multi, st = render(phip, gs, devices=[0, 0], flags=A.PHIP_FLAG_ALIAS_DEVICES)
    assert rc == A.PHIP_OK and st.n_devices == 2 and st.samples == samples
    assert same_bits(multi, frame)


def test_scene_replicate_checks_the_list_and_leaves_the_scene_renderable(box):
    phip, gs, visible, frame, samples = box
    assert replicate(phip, gs, [0, visible]) == A.PHIP_ERR_INVALID
    assert phip.phip_last_error().decode() == "device ordinal out of range"
    assert replicate(phip, gs, [0, -1]) == A.PHIP_ERR_INVALID
    assert phip.phip_last_error().decode() == "device ordinal out of range"
    assert replicate(phip, gs, [visible, 0]) == A.PHIP_ERR_INVALID
    assert phip.phip_last_error().decode() == "devices[0] must be the scene's device"
    rc, again, st = render(phip, gs)
    assert rc == A.PHIP_OK and st.n_devices == 1 and same_bits(again, frame)


def test_replicas_made_ahead_serve_the_render_of_the_same_list(box):
    """phip_scene_replicate and the render share one replica set: the list {0, 0} replicated ahead is the list the aliased render finds, call after call"""
    phip, gs, visible, frame, samples = box
    assert replicate(phip, gs, [0, 0]) == A.PHIP_OK
    for _ in range(2):
        rc, multi, st = render(phip, gs, devices=[0, 0], flags=A.PHIP_FLAG_ALIAS_DEVICES)
        assert rc == A.PHIP_OK and st.n_devices == 2 and st.samples == samples and same_bits(multi, frame)
    assert replicate(phip, gs, [0, 0]) == A.PHIP_OK
    assert replicate(phip, gs, [0]) == A.PHIP_OK
    rc, again, st = render(phip, gs)
    assert rc == A.PHIP_OK and st.n_devices == 1 and same_bits(again, frame)

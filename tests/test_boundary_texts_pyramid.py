"""The texts of phip_mip_pyramid_device and phip_mip_pyramid, pinned as tests/test_boundary_texts.py pins those of the other entry points on the caller's device
memory: every refusal of pyramidArgsError (host_pyramid.h) through the debug library's hook and through the host call, code and text byte for byte.  The
pointers are never dereferenced by the hook: the checks look at values only.  On the GPU: a host pointer in place of a device level."""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi

BUF = 1 << 20                                                       # 5 x 3: levels of 180, 72, 24, 12 bytes, 256 apart
INV = A.PHIP_ERR_INVALID
GOOD = dict(width=5, height=3, n_levels=4, wrap_u=A.PHIP_WRAP_REPEAT, wrap_v=A.PHIP_WRAP_MIRROR, max_value=1.0, d_level0=BUF,
            levels=(BUF + 256, BUF + 512, BUF + 768, BUF + 1024))

# (have_scene, what differs from GOOD -- None: a NULL descriptor --, code, text after the call's name)
REFUSALS = [
    (0, {}, INV, "NULL argument"),
    (1, None, INV, "NULL argument"),
    (1, dict(width=0), INV, "width and height must not be 0"),
    (1, dict(height=0), INV, "width and height must not be 0"),
    (1, dict(width=65536, n_levels=17), INV, "width and height must be smaller than 65536"),
    (1, dict(height=1 << 20), INV, "width and height must be smaller than 65536"),
    (1, dict(n_levels=3), INV, "n_levels must be the complete pyramid down to 1x1"),
    (1, dict(n_levels=1), INV, "n_levels must be the complete pyramid down to 1x1"),
    (1, dict(n_levels=5), INV, "n_levels must be the complete pyramid down to 1x1"),
    (1, dict(wrap_u=5), INV, "bad wrap mode"),
    (1, dict(wrap_v=0xFFFFFFFF), INV, "bad wrap mode"),
    (1, dict(max_value=0.0), INV, "max_value must be greater than 0"),
    (1, dict(max_value=-1.0), INV, "max_value must be greater than 0"),
    (1, dict(max_value=float("nan")), INV, "max_value must be greater than 0"),
    (1, dict(d_level0=None), INV, "d_level0 must not be NULL"),
    (1, dict(levels=(BUF + 256, None, BUF + 768, BUF + 1024)), INV, "d_levels[l] must not be NULL for 1 <= l < n_levels"),
    (1, dict(levels=(None, BUF + 512, BUF + 768, None)), INV, "d_levels[l] must not be NULL for 1 <= l < n_levels"),
    (1, dict(d_level0=BUF + 2), INV, "every pointer must be 4-byte aligned"),
    (1, dict(levels=(BUF + 256, BUF + 513, BUF + 768, BUF + 1024)), INV, "every pointer must be 4-byte aligned"),
    (1, dict(levels=(BUF + 4, BUF + 512, BUF + 768, BUF + 1024)), INV, "levels overlap: only d_levels[0] == d_level0 may"),          # level 0 shifted by a float
    (1, dict(levels=(BUF, BUF + 176, BUF + 768, BUF + 1024)), INV, "levels overlap: only d_levels[0] == d_level0 may"),             # level 1 in level 0's last float
    (1, dict(levels=(None, BUF + 512, BUF + 512, BUF + 1024)), INV, "levels overlap: only d_levels[0] == d_level0 may"),
    (1, dict(levels=(BUF + 256, BUF + 512, BUF + 768, BUF + 788)), INV, "levels overlap: only d_levels[0] == d_level0 may"),
    (1, dict(levels=(BUF, BUF + 512, BUF + 768, BUF)), INV, "levels overlap: only d_levels[0] == d_level0 may"),                    # in place, and the last level there too
    (1, {}, 0, None),
    (1, dict(levels=(None, BUF + 512, BUF + 768, BUF + 1024)), 0, None),                                                            # level 0 not asked for
    (1, dict(levels=(BUF, BUF + 180, BUF + 252, BUF + 276)), 0, None),                                                              # in place, the rest packed behind it
    (1, dict(max_value=float("inf"), wrap_u=A.PHIP_WRAP_ONE, wrap_v=A.PHIP_WRAP_CLAMP), 0, None),
    (1, dict(width=1, height=1, n_levels=1, levels=(None,)), 0, None),
    (1, dict(width=65535, height=1, n_levels=17, levels=tuple(BUF * (2 + l) for l in range(17))), 0, None),
]


def descriptor(diff):
    if diff is None:
        return None
    kw = dict(GOOD, **diff)
    p = A.phip_pyramid_desc()
    for name in ("width", "height", "n_levels", "wrap_u", "wrap_v", "max_value", "d_level0"):
        setattr(p, name, kw[name])
    for l, ptr in enumerate(kw["levels"]):
        p.d_levels[l] = ptr
    for l in range(len(kw["levels"]), A.PHIP_MIP_MAX_LEVELS):
        p.d_levels[l] = 3                                           # beyond n_levels: never looked at
    return p


@pytest.mark.parametrize("case", REFUSALS, ids=["%d-%s" % (i, (c[3] or "ok").split(":")[0][:32].replace(" ", "_")) for i, c in enumerate(REFUSALS)])
def test_refusal_code_and_text(phip, case):
    have_scene, diff, code, text = case
    p = descriptor(diff)
    rc = phip.phip_debug_host_pyramid_args(have_scene, C.byref(p) if p is not None else None)
    assert rc == code
    if text is not None:
        assert _ffi.debug_lib().phip_last_error().decode() == "phip_mip_pyramid_device: " + text


def test_entry_points_refuse_before_they_look_for_a_device(phip):
    """the product library: a NULL scene, a NULL descriptor and a bad descriptor come back with the same texts, with or without a device; the host call under its own name"""
    p = descriptor({})
    assert phip.phip_mip_pyramid_device(None, C.byref(p)) == INV and phip.phip_last_error().decode() == "phip_mip_pyramid_device: NULL argument"
    assert phip.phip_mip_pyramid_device(C.c_void_p(1), None) == INV and phip.phip_last_error().decode() == "phip_mip_pyramid_device: NULL argument"
    for have_scene, diff, code, text in REFUSALS:
        if not have_scene or code == 0:
            continue
        q = descriptor(diff)
        assert phip.phip_mip_pyramid_device(C.c_void_p(1), C.byref(q) if q is not None else None) == code
        assert phip.phip_last_error().decode() == "phip_mip_pyramid_device: " + text
        assert phip.phip_mip_pyramid(C.byref(q) if q is not None else None) == code
        assert phip.phip_last_error().decode() == "phip_mip_pyramid: " + text


@pytest.mark.gpu
def test_a_host_pointer_is_refused_and_nothing_is_written(phip, gauss):
    import torch
    from mitsuba_amd import scene as S
    from mitsuba_amd.integrator import Scene
    if phip.phip_device_count() <= 0:
        pytest.fail("no HIP device visible: " + phip.phip_last_error().decode())
    gs = Scene(S.cornell_box(16, 16, gauss).desc())
    level0 = torch.rand((3, 5, 3), device="cuda")
    outs = [torch.full((h, w, 3), 7.0, device="cuda") for h, w in S.pyramid_sizes(5, 3)]
    host = np.zeros((1, 2, 3), np.float32)
    p = A.phip_pyramid_desc()
    p.width, p.height, p.n_levels, p.wrap_u, p.wrap_v, p.max_value = 5, 3, 4, 1, 1, 1.0
    p.d_level0 = level0.data_ptr()
    for l, o in enumerate(outs):
        p.d_levels[l] = o.data_ptr()
    p.d_levels[2] = host.ctypes.data
    assert phip.phip_mip_pyramid_device(gs._h, C.byref(p)) == INV
    assert phip.phip_last_error().decode() == "phip_mip_pyramid_device: every pointer must be device memory of the scene's device"
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    p.d_levels[2] = outs[2].data_ptr()
    p.d_level0 = host.ctypes.data
    assert phip.phip_mip_pyramid_device(gs._h, C.byref(p)) == INV
    assert phip.phip_last_error().decode() == "phip_mip_pyramid_device: every pointer must be device memory of the scene's device"
    gs.close()

"""The texts of phip_vertex_normals_device and phip_vertex_normals, pinned as tests/test_boundary_texts_pyramid.py pins those of the pyramid calls: every refusal
of normalsArgsError (host_normals.h) through the debug library's hook, and those of the host call through the call itself, code and text byte for byte.  The
pointers are never dereferenced by the hook: the checks look at values only.  On the GPU: the refusals that need the scene or the device."""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi

BUF = 1 << 20
INV = A.PHIP_ERR_INVALID
NV, NT = 10, 4                                                      # the scene's counts the hook is told: 120 bytes of positions, of normals
GOOD = dict(n_vertices=NV, n_triangles=NT, indices=None, positions=BUF, normals=BUF + 256)

# (have_scene, what differs from GOOD -- None: a NULL descriptor --, code, text after the call's name)
REFUSALS = [
    (0, {}, INV, "NULL argument"),
    (1, None, INV, "NULL argument"),
    (1, dict(positions=None), INV, "positions and normals must not be NULL"),
    (1, dict(normals=None), INV, "positions and normals must not be NULL"),
    (1, dict(n_vertices=NV + 1), INV, "n_vertices and n_triangles must be the scene's"),
    (1, dict(n_triangles=0), INV, "n_vertices and n_triangles must be the scene's"),
    (1, dict(indices=BUF + 1024), INV, "indices must be NULL: the device call uses the scene's own"),
    (1, dict(positions=BUF + 2), INV, "every pointer must be 4-byte aligned"),
    (1, dict(normals=BUF + 257), INV, "every pointer must be 4-byte aligned"),
    (1, dict(normals=BUF), INV, "positions and normals overlap"),                                  # in place
    (1, dict(normals=BUF + 116), INV, "positions and normals overlap"),                            # the normals begin in the positions' last float
    (1, dict(positions=BUF + 256 + 116), INV, "positions and normals overlap"),                    # ... and the other way round
    (1, {}, 0, None),
    (1, dict(normals=BUF + 120), 0, None),                                                         # packed behind the positions
    (1, dict(positions=BUF + 256 + 120), 0, None),
]


def descriptor(diff):
    if diff is None:
        return None
    return A.phip_normals_desc(**dict(GOOD, **diff))


@pytest.mark.parametrize("case", REFUSALS, ids=["%d-%s" % (i, (c[3] or "ok").split(":")[0][:32].replace(" ", "_")) for i, c in enumerate(REFUSALS)])
def test_refusal_code_and_text(phip, case):
    have_scene, diff, code, text = case
    p = descriptor(diff)
    rc = phip.phip_debug_host_normals_args(have_scene, NV, NT, C.byref(p) if p is not None else None)
    assert rc == code
    if text is not None:
        assert _ffi.debug_lib().phip_last_error().decode() == "phip_vertex_normals_device: " + text


def test_device_call_refuses_a_null_scene_or_desc_before_it_looks_for_a_device(phip):
    p = descriptor({})
    assert phip.phip_vertex_normals_device(None, C.byref(p), None) == INV and phip.phip_last_error().decode() == "phip_vertex_normals_device: NULL argument"


def test_host_call_refusals_leave_the_output_untouched(phip):
    P = np.arange(12, dtype=np.float32).reshape(4, 3)
    T = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    N = np.full((4, 3), 7.0, np.float32)
    info = A.phip_normals_info(n_invalid=99)
    good = dict(n_vertices=4, n_triangles=2, indices=T.ctypes.data, positions=P.ctypes.data, normals=N.ctypes.data)
    bad_index = T.copy(); bad_index[1, 2] = 4
    cases = [(None, "NULL argument"),
             (dict(positions=None), "positions, normals and indices must not be NULL"), (dict(normals=None), "positions, normals and indices must not be NULL"),
             (dict(indices=None), "positions, normals and indices must not be NULL"),
             (dict(n_vertices=0), "n_vertices must not be 0"),
             (dict(positions=P.ctypes.data + 2), "every pointer must be 4-byte aligned"), (dict(indices=T.ctypes.data + 1), "every pointer must be 4-byte aligned"),
             (dict(normals=P.ctypes.data + 44), "positions and normals overlap"),
             (dict(indices=bad_index.ctypes.data), "triangle index out of range")]
    for diff, text in cases:
        d = A.phip_normals_desc(**dict(good, **diff)) if diff is not None else None
        assert phip.phip_vertex_normals(C.byref(d) if d is not None else None, C.byref(info)) == INV, text
        assert phip.phip_last_error().decode() == "phip_vertex_normals: " + text
        assert (N == 7.0).all() and info.n_invalid == 99
    d = A.phip_normals_desc(**good)
    assert phip.phip_vertex_normals(C.byref(d), None) == 0 and not (N == 7.0).any()       # out_info may be NULL
    e = A.phip_normals_desc(**dict(good, n_triangles=0, indices=None))
    assert phip.phip_vertex_normals(C.byref(e), C.byref(info)) == 0 and info.n_invalid == 4    # no triangles: no indices needed


@pytest.mark.gpu
def test_device_only_refusals_leave_the_output_untouched(phip, gauss):
    """foreign memory, overlap and counts against a live scene: code, text, and the sentinel in the output stays"""
    import torch
    from mitsuba_amd import scene as S
    from mitsuba_amd.integrator import Scene
    if phip.phip_device_count() <= 0:
        pytest.fail("no HIP device visible: " + phip.phip_last_error().decode())
    gs = Scene(S.cornell_box(16, 16, gauss).desc())
    nv, nt = gs.desc.n_vertices, gs.desc.n_triangles
    pos = torch.rand((nv, 3), device="cuda")
    out = torch.full((nv + 2, 3), 7.0, device="cuda")
    host = np.zeros((nv, 3), np.float32)
    info = A.phip_normals_info()
    good = dict(n_vertices=nv, n_triangles=nt, indices=None, positions=pos.data_ptr(), normals=out.data_ptr())
    where = "phip_vertex_normals_device: "
    for diff, text in ((dict(positions=host.ctypes.data), "every pointer must be device memory of the scene's device"),
                       (dict(normals=host.ctypes.data), "every pointer must be device memory of the scene's device"),
                       (dict(normals=pos.data_ptr() + 12), "positions and normals overlap"),
                       (dict(n_vertices=nv - 1), "n_vertices and n_triangles must be the scene's"),
                       (dict(n_triangles=nt + 1), "n_vertices and n_triangles must be the scene's"),
                       (dict(indices=pos.data_ptr()), "indices must be NULL: the device call uses the scene's own")):
        d = A.phip_normals_desc(**dict(good, **diff))
        assert phip.phip_vertex_normals_device(gs._h, C.byref(d), C.byref(info)) == INV, text
        assert phip.phip_last_error().decode() == where + text
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and (host == 0).all()
    with pytest.raises(ValueError):
        gs.vertex_normals(pos[:-1])
    gs.close()

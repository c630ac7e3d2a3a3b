"""phip_mip_pyramid, the host twin of phip_mip_pyramid_device's kernels (pyramid_hd.h): the MIP pyramid of the reference's TMIPMap, bit for bit -- against the
reference-built pyramids of tests/golden/ref_renders.npz, against the numpy restatement tests/pyramid_reference.py, and, where oracle/_ref exists, against the
reference's own code (RefMip).  Every comparison is on the uint32 view: there is no tolerance.  No GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import pyramid_reference as PR
import ref_scenes as RS
from conftest import bits
from mitsuba_amd import _abi as A, _ffi, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPS = ("clamp", "repeat", "mirror", "zero", "one")
INF = float("inf")


def same_levels(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, l, g.shape, w.shape)
        bad = bits(g) != bits(w)
        assert not bad.any(), "%s level %d: %d of %d floats differ, first at %s: %r != %r" % (
            what, l, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), g[tuple(np.argwhere(bad)[0])], w[tuple(np.argwhere(bad)[0])])


def golden_groups():
    """[(scene, key, kind, wrap_u, wrap_v, levels)] of every multi-level pyramid of the fixture, the wrap modes as tests/ref_scenes.py passes them"""
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "ref_renders.npz"))
    out = []
    for build in (RS.envmap, RS.textures, RS.roughness_maps):
        scene = build.__name__

        def mip(key, image, kind, wrap_u="repeat", wrap_v=None, **kw):
            levels = []
            while "mip/%s/%s/%d" % (scene, key, len(levels)) in fixture:
                levels.append(np.ascontiguousarray(fixture["mip/%s/%s/%d" % (scene, key, len(levels))]))
            if len(levels) > 1:
                out.append((scene, key, kind, wrap_u, wrap_v or wrap_u, levels))
            return levels
        build((2.0, [0.0] * 32), mip)                               # (the film's filter table is of no interest here, and no library is loaded at import)
    return out


GOLDEN = golden_groups()


def test_the_fixture_has_the_pyramids_the_issue_names():
    keys = {g[1]: g for g in GOLDEN}
    assert {"envmap", "floor", "tri", "ewa2", "rm_u"} <= set(keys), sorted(keys)
    assert keys["tri"][3:5] == ("mirror", "clamp") and keys["ewa2"][3:5] == ("clamp", "clamp") and keys["rm_u"][3:5] == ("mirror", "mirror")
    assert keys["envmap"][2] == "envmap" and keys["envmap"][5][0].shape == (32, 64, 3)


@pytest.mark.parametrize("group", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_host_call_equals_the_reference_built_fixture(phip, group):
    scene, key, kind, wrap_u, wrap_v, levels = group
    if kind == "envmap":
        got = S.mip_pyramid_lanczos(levels[0], "repeat", "clamp", INF)
    else:
        got = S.mip_pyramid_lanczos(levels[0], wrap_u, wrap_v, 1.0)
    same_levels(got, levels, key)


def test_bitmap_and_envmap_with_lanczos_pyramids_carry_the_fixtures_levels(phip):
    by_key = {g[1]: g for g in GOLDEN}
    sb = S.SceneBuilder()
    _, _, _, wu, wv, levels = by_key["tri"]
    t = sb.bitmap(levels[0], wrap=wu, wrap_v=wv, filter_type="trilinear", pyramid="lanczos")
    same_levels(sb.textures[t]["levels"], levels, "tri")
    assert len(sb.textures[sb.bitmap(levels[0], filter_type="bilinear", pyramid="lanczos")]["levels"]) == 1          # nearest / bilinear keep one level
    assert len(sb.textures[sb.bitmap(levels[0], filter_type="ewa")]["levels"]) == len(levels)                          # the default: the box stand-in, as before
    assert not np.array_equal(sb.textures[-1]["levels"][1], levels[1])
    env = by_key["envmap"][5]
    sb.envmap(env[0], pyramid="lanczos")
    same_levels(sb._envmap[3], env, "envmap")


# ---- sizes and values the fixtures do not cover: the numpy restatement, and the reference itself where it is built ----
def image(w, h, seed, lo=0.0, hi=1.0, half_exact=True):
    img = np.random.default_rng(seed).uniform(lo, hi, (h, w, 3)).astype(np.float32)
    return img.astype(np.float16).astype(np.float32) if half_exact else img


SIZES = ((1, 1), (2, 1), (1, 2), (1, 9), (9, 1), (3, 5), (2, 2), (65, 33))
# (id, image, kind, wrap_u, wrap_v): what the issue lists
CASES = [("wrap-%s-%s" % (u, v), image(13, 7, 100 + i), "texture", u, v) for i, (u, v) in enumerate(itertools.product(WRAPS, WRAPS))]
CASES += [("size-%dx%d" % (w, h), image(w, h, 200 + i), "texture", "repeat", "mirror") for i, (w, h) in enumerate(SIZES)]
CASES += [("not-half-exact", image(13, 7, 300, half_exact=False), "texture", "repeat", "repeat"),
          ("above-1-below-0", image(13, 7, 301, -0.5, 1.8, half_exact=False), "texture", "mirror", "one"),
          ("env-plain", image(16, 8, 302, 0.0, 30.0), "envmap", "repeat", "clamp")]
_e = image(12, 6, 303, 0.0, 4.0, half_exact=False)
_e[0, :4] = (70000.0, 65519.9, 131072.0); _e[1, :3] = (65520.0, 65504.0, 3.0e5); _e[3, 2:6] = (5.0e-8, 2.0e-8, 6.1e-5); _e[4, :2] = (2.9e-8, 3.0e-8, 1.0e-10); _e[5, 3] = (-2.0, 0.5, -0.0)
CASES += [("env-above-65504-below-6e-8", _e, "envmap", "repeat", "clamp")]


def host_pyramid(img, kind, wu, wv):
    return S.mip_pyramid_lanczos(img, "repeat", "clamp", INF) if kind == "envmap" else S.mip_pyramid_lanczos(img, wu, wv, 1.0)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_call_equals_the_numpy_restatement(phip, case):
    name, img, kind, wu, wv = case
    want = PR.pyramid(img, "repeat", "clamp", INF) if kind == "envmap" else PR.pyramid(img, wu, wv, 1.0)
    assert [l.shape[:2] for l in want] == PR.sizes(img.shape[1], img.shape[0])
    same_levels(host_pyramid(img, kind, wu, wv), want, name)


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_ffi
    if not ref_ffi.available():
        pytest.skip("neither /root/reference nor a prebuilt oracle/_ref is present")
    ref_ffi.lib()
    return ref_ffi


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_call_equals_the_reference_itself(phip, ref, case):
    name, img, kind, wu, wv = case
    m = ref.RefMip(img, kind=kind, wrap_u=wu, wrap_v=wv)
    try:
        same_levels(host_pyramid(img, kind, wu, wv), m.levels, name)
    finally:
        m.close()


# ---- the boundary ----
def test_abi_mirror_units_and_symbols(phip):
    header = open(os.path.join(ROOT, "include", "phip.h")).read()
    assert "} phip_pyramid_desc;" in header and "#define PHIP_ABI_VERSION 7" in header            # entry points and one new struct: no struct of the ABI changed
    assert phip.phip_abi_sizeof(29) == C.sizeof(A.phip_pyramid_desc) == 176
    assert phip.phip_abi_sizeof(28) == 0 and phip.phip_abi_sizeof(30) == 0
    assert phip.phip_abi_sizeof(20) == C.sizeof(A.phip_appearance_desc) and phip.phip_abi_sizeof(5) == C.sizeof(A.phip_scene_desc)      # nothing else moved
    assert hasattr(phip, "phip_mip_pyramid_device") and hasattr(phip, "phip_mip_pyramid")
    assert ("phip_pyramid.hip", [], "phip_pyramid.o") in _ffi.UNITS                                 # a unit of its own
    assert all("phip_pyramid.hip" in v.split() for v in _ffi.VARIANT_REUSE.values())


def test_device_call_without_a_device_is_a_device_error(phip, have_gpu):
    if have_gpu:
        pytest.skip("a GPU is present")
    img = image(4, 2, 1)
    out = [np.zeros((h, w, 3), np.float32) for h, w in PR.sizes(4, 2)]
    p = A.phip_pyramid_desc()
    p.width, p.height, p.n_levels, p.wrap_u, p.wrap_v, p.max_value = 4, 2, len(out), 1, 1, 1.0
    p.d_level0 = img.ctypes.data
    for l, o in enumerate(out):
        p.d_levels[l] = o.ctypes.data
    fake = C.c_void_p(1)                                            # never dereferenced: the device count comes first
    assert phip.phip_mip_pyramid_device(fake, C.byref(p)) == A.PHIP_ERR_DEVICE
    assert phip.phip_last_error().decode().startswith("phip_mip_pyramid_device: ")


def test_a_refused_host_call_writes_nothing(phip):
    img = image(5, 3, 2)
    sizes = PR.sizes(5, 3)
    out = [np.full((h, w, 3), 7.0, np.float32) for h, w in sizes]
    p = A.phip_pyramid_desc()
    p.width, p.height, p.n_levels, p.wrap_u, p.wrap_v, p.max_value = 5, 3, len(out), 1, 1, 1.0
    p.d_level0 = img.ctypes.data
    for l, o in enumerate(out):
        p.d_levels[l] = o.ctypes.data
    p.d_levels[len(out) - 1] = out[0].ctypes.data + 12            # the last level inside level 0's output
    assert phip.phip_mip_pyramid(C.byref(p)) == A.PHIP_ERR_INVALID
    assert all((o == 7.0).all() for o in out)
    p.d_levels[len(out) - 1] = out[-1].ctypes.data
    p.d_levels[0] = None                                            # level 0 not asked for
    assert phip.phip_mip_pyramid(C.byref(p)) == 0
    assert (out[0] == 7.0).all() and not (out[1] == 7.0).any()
    p.d_levels[0] = img.ctypes.data                                 # in place
    want = S.mip_pyramid_lanczos(img.copy())
    assert phip.phip_mip_pyramid(C.byref(p)) == 0
    same_levels([img] + out[1:], want, "in place")

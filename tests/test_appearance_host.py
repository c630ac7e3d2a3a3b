"""phip_scene_update_appearance without a GPU: its place in the ABI, its refusals -- through phip_debug_host_appearance_args, the debug library's hook that takes the
scene's look from the descriptor of its creation by the creation's host stages and runs the call's own checks on it (host_appearance.h: appearanceArgs,
appearanceLook; the textures' maxima and the environment map's CDF through appearance_hd.h, the functions the kernels run) -- and the environment map's tables as
the creation builds them around appearance_hd.h, against a numpy float32 restatement of EnvironmentMap::configure (envmap.cpp:262-328) written here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi, scene as S

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED = A.PHIP_ERR_INVALID, A.PHIP_ERR_UNSUPPORTED


def test_abi_of_the_entry_point(phip, have_gpu):
    header = open(os.path.join(HERE, "..", "include", "phip.h")).read()
    assert "int phip_scene_update_appearance(phip_scene *scene, const phip_appearance_desc *desc, phip_appearance_info *out_info /* may be NULL */);" in header
    assert "} phip_appearance_desc;" in header and "} phip_appearance_info;" in header and "#define PHIP_ABI_VERSION 7" in header
    assert phip.phip_abi_sizeof(20) == C.sizeof(A.phip_appearance_desc) == 56
    assert phip.phip_abi_sizeof(21) == C.sizeof(A.phip_appearance_info) == 24
    for unassigned in (14, 16, 19, 22):
        assert phip.phip_abi_sizeof(unassigned) == 0, unassigned
    assert phip.phip_abi_sizeof(11) == C.sizeof(A.phip_update_desc) and phip.phip_abi_sizeof(5) == C.sizeof(A.phip_scene_desc)      # nothing else moved
    offsets = lambda s: {n: getattr(s, n).offset for n, _ in s._fields_}
    assert offsets(A.phip_appearance_desc) == dict(n_materials=0, n_emitters=4, n_textures=8, device_pointers=12, materials=16, emitters=24, textures=32, envmap=40, stream=48)
    assert offsets(A.phip_appearance_info) == dict(update_ms=0, kernel_ms=8, material_mask_changed=16, reserved=20)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB], capture_output=True, text=True).stdout
    assert " phip_scene_update_appearance" in out and "phip_debug_" not in out
    assert ("phip_appearance.hip", [], "phip_appearance.o") in _ffi.UNITS                                        # a unit of its own
    for name in ("phip_appearance.hip", "host_appearance.h", "k_appearance.h", "appearance_hd.h"):
        assert os.path.exists(os.path.join(_ffi.CSRC, name)), name
    assert phip.phip_scene_update_appearance(None, None, None) == INVALID                                       # no scene
    never_read = C.create_string_buffer(64)
    scene = C.cast(never_read, C.c_void_p)
    info = A.phip_appearance_info(update_ms=1.0)
    assert phip.phip_scene_update_appearance(scene, None, C.byref(info)) == A.PHIP_OK and info.update_ms == 0.0  # nothing to change: the scene is not looked at
    assert phip.phip_scene_update_appearance(scene, C.byref(A.phip_appearance_desc()), None) == A.PHIP_OK
    if not have_gpu:
        m = A.phip_material()
        a = A.phip_appearance_desc(n_materials=1, materials=C.pointer(m))
        assert phip.phip_scene_update_appearance(scene, C.byref(a), None) == A.PHIP_ERR_DEVICE                    # no CPU fallback
        assert phip.phip_last_error()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------

def build(gauss, env=True, tex_max=0.9, env_level0=None, env_to_world=None):
    """three quads: a textured one (5 x 3 texels with their pyramid, texture coordinates), a two-sided plain one without texture coordinates, a light; an
    environment map of 16 x 8 with its pyramid"""
    rng = np.random.default_rng(3)
    sb = S.SceneBuilder()
    if env:
        sky = rng.uniform(0.1, 2.0, (8, 16, 3)).astype(np.float32) if env_level0 is None else env_level0
        sb.envmap(sky, scale=0.7, to_world=env_to_world, pyramid=True)
    img = rng.uniform(0.05, 0.8, (3, 5, 3)).astype(np.float32)
    img[1, 2, 1] = tex_max
    t0 = sb.bitmap(img, filter_type="ewa")
    m_tex = sb.diffuse(texture=t0)
    m_plain = sb.diffuse((0.5, 0.4, 0.3))
    m_two = sb.twosided(m_plain)
    m_light = sb.diffuse((0.0, 0.0, 0.0))
    sb.quad((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), m_tex, uvs=True)
    sb.quad((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1), m_two)
    sb.quad((0.4, 0.99, 0.4), (0.6, 0.99, 0.4), (0.6, 0.99, 0.6), (0.4, 0.99, 0.6), m_light, radiance=(10, 10, 10))
    sb.perspective((0.5, 0.5, -2.0), (0.5, 0.5, 0.5), (0, 1, 0), 40.0)
    sb.hdrfilm(16, 16, gauss)
    return sb


def look(d, materials=False, emitters=False, textures=False, envmap=False):
    """the phip_appearance_desc that takes these parts of descriptor d"""
    a = A.phip_appearance_desc()
    if materials:
        a.n_materials, a.materials = d.n_materials, d.materials
    if emitters:
        a.n_emitters, a.emitters = d.n_emitters, d.emitters
    if textures:
        a.n_textures, a.textures = d.n_textures, d.textures
    if envmap:
        a.envmap = C.pointer(d.envmap)
    a._keep = d
    return a


def check(phip, created, a, of_the_call=True):
    rc = phip.phip_debug_host_appearance_args(C.byref(created), C.byref(a) if a is not None else None)
    msg = _ffi.debug_lib().phip_last_error().decode()
    assert rc == 0 or not of_the_call or msg.startswith("phip_scene_update_appearance: "), msg
    return rc, msg


@pytest.fixture(scope="module")
def created(gauss):
    return build(gauss).desc()


def test_nothing_to_change_and_a_valid_look_pass(phip, created, gauss):
    assert check(phip, created, None)[0] == 0
    assert check(phip, created, A.phip_appearance_desc())[0] == 0
    sb = build(gauss, tex_max=1.0)
    sb.materials[1].reflectance[:] = [0.0, 0.0, 0.0]
    sb.materials[3].type = A.PHIP_BSDF_DIELECTRIC; sb.materials[3].eta[0] = 1.5
    sb.emitters[1]["radiance"] = [3.0, 2.0, 1.0]; sb.emitters[1]["weight"] = 0.25
    d = sb.desc()
    assert check(phip, created, look(d, True, True, True, True))[0] == 0
    for part in range(4):
        assert check(phip, created, look(d, *[k == part for k in range(4)]))[0] == 0, part
    skip = look(d, textures=True); skip.textures[0].width = 0                       # width 0: this texture stays, nothing of the entry is looked at
    skip.textures[0].levels[0] = None
    assert check(phip, created, skip)[0] == 0
    dev = look(d, textures=True, envmap=True); dev.device_pointers = 1              # device pointers: what needs no texel is still checked, and passes
    assert check(phip, created, dev)[0] == 0


def material_case(gauss, edit):
    sb = build(gauss)
    edit(sb)
    return look(sb.desc(), materials=True)


MATERIAL_REFUSALS = {
    "unknown type": (lambda sb: setattr(sb.materials[1], "type", 9), INVALID, "unknown bsdf type"),
    "reflectance above one": (lambda sb: sb.materials[1].reflectance.__setitem__(1, 1.5), INVALID, "diffuse reflectance > 1"),
    "twosided nests glass": (lambda sb: (setattr(sb.materials[1], "type", A.PHIP_BSDF_DIELECTRIC), sb.materials[1].eta.__setitem__(0, 1.5)), INVALID, "twosided: only materials without a transmission component"),
    "twosided nests a later material": (lambda sb: sb.materials[2].nested.__setitem__(1, 3), INVALID, "twosided: nested materials must precede the adapter"),
    "texture id out of range": (lambda sb: setattr(sb.materials[1], "reflectance_texture", 2), INVALID, "material texture id out of range"),
    "eta not positive": (lambda sb: (setattr(sb.materials[3], "type", A.PHIP_BSDF_DIELECTRIC), sb.materials[3].eta.__setitem__(0, 0.0)), INVALID, "dielectric eta must be positive"),
    "anisotropic without texture coordinates": (lambda sb: (setattr(sb.materials[1], "type", A.PHIP_BSDF_ROUGHCONDUCTOR), setattr(sb.materials[1], "alpha_u", 0.1), setattr(sb.materials[1], "alpha_v", 0.3)),
                                                INVALID, "computeUVTangents(): texture coordinates are required"),
    "unsupported distribution": (lambda sb: (setattr(sb.materials[3], "type", A.PHIP_BSDF_ROUGHCONDUCTOR), setattr(sb.materials[3], "distribution", 2)), UNSUPPORTED, "unsupported microfacet distribution"),
}


@pytest.mark.parametrize("case", sorted(MATERIAL_REFUSALS))
def test_what_the_creation_refuses_of_a_material_array(phip, created, gauss, case):
    edit, code, text = MATERIAL_REFUSALS[case]
    rc, msg = check(phip, created, material_case(gauss, edit))
    assert rc == code and text in msg, (rc, msg)


def test_an_isotropic_rough_conductor_without_texture_coordinates_is_served(phip, created, gauss):
    a = material_case(gauss, lambda sb: (setattr(sb.materials[1], "type", A.PHIP_BSDF_ROUGHCONDUCTOR), setattr(sb.materials[1], "alpha_u", 0.2), setattr(sb.materials[1], "alpha_v", 0.2)))
    assert check(phip, created, a)[0] == 0


def test_counts_and_what_has_to_be_the_creations(phip, created, gauss):
    d = build(gauss).desc()
    for field in ("n_materials", "n_emitters", "n_textures"):
        a = look(d, True, True, True)
        setattr(a, field, getattr(a, field) + 1)
        rc, msg = check(phip, created, a)
        assert rc == INVALID and field in msg, msg
    a = look(d, emitters=True); a.emitters[1].type = A.PHIP_EMITTER_CONSTANT
    assert check(phip, created, a)[0] == INVALID
    a = look(build(gauss).desc(), emitters=True); a.emitters[1].shape = 0
    rc, msg = check(phip, created, a)
    assert rc == INVALID and "type and shape must be the creation's" in msg
    for edit in (lambda t: setattr(t, "width", 6), lambda t: setattr(t, "height", 4), lambda t: setattr(t, "n_levels", 1)):
        a = look(build(gauss).desc(), textures=True); edit(a.textures[0])
        rc, msg = check(phip, created, a)
        assert rc == INVALID and "must be the creation's" in msg, msg
    a = look(build(gauss).desc(), textures=True); a.textures[0].levels[2] = None
    assert check(phip, created, a) == (INVALID, "phip_scene_update_appearance: texture: level pointer is NULL")
    a = look(build(gauss).desc(), textures=True); a.textures[0].levels[0] = None
    assert check(phip, created, a) == (INVALID, "phip_scene_update_appearance: texture without level 0")
    a = look(build(gauss).desc(), textures=True); a.textures[0].wrap_v = 5
    assert check(phip, created, a) == (INVALID, "phip_scene_update_appearance: bad texture wrap mode / filter type")
    for edit in (lambda e: setattr(e, "width", 15), lambda e: setattr(e, "height", 9), lambda e: setattr(e, "n_levels", 1)):
        a = look(build(gauss).desc(), envmap=True); edit(a.envmap.contents)
        rc, msg = check(phip, created, a)
        assert rc == INVALID and "envmap: width, height and n_levels must be the creation's" in msg, msg
    a = look(build(gauss).desc(), envmap=True); a.envmap.contents.levels[3] = None
    assert check(phip, created, a) == (INVALID, "phip_scene_update_appearance: envmap: level pointer is NULL")
    a = look(build(gauss).desc(), envmap=True); a.envmap.contents.texels = None
    assert check(phip, created, a) == (INVALID, "phip_scene_update_appearance: envmap emitter without texels")
    no_env = build(gauss, env=False).desc()
    rc, msg = check(phip, no_env, look(d, envmap=True))
    assert rc == INVALID and "without an envmap emitter" in msg


def test_energy_conservation_against_the_new_texels(phip, created, gauss):
    """the maximum is the NEW texture's; a NaN channel is ignored exactly as packTextures ignores it"""
    hot = build(gauss, tex_max=1.5).desc()
    rc, msg = check(phip, created, look(hot, textures=True))                        # the materials are the scene's own: they read the new maximum
    assert rc == INVALID and "diffuse reflectance > 1 (ensureEnergyConservation, diffuse.cpp:95)" in msg
    rc, msg = check(phip, created, look(hot, materials=True, textures=True))
    assert rc == INVALID and "diffuse reflectance > 1" in msg
    assert check(phip, created, look(build(gauss, tex_max=1.0).desc(), textures=True))[0] == 0
    assert check(phip, hot, None, of_the_call=False)[0] == INVALID                                    # ... as the creation refuses it
    sb = build(gauss); sb.textures[0]["levels"][0][1, 2, 0] = np.nan; sb.textures[0]["levels"][0][1, 2, 1] = 7.0
    assert check(phip, created, look(sb.desc(), textures=True))[0] == 0             # std::max(NaN, x) is NaN, std::max(m, NaN) is m: that texel does not count
    assert check(phip, sb.desc(), None)[0] == 0                                      # ... and the creation accepts the same texture


def test_environment_maps_that_cannot_be_sampled(phip, created, gauss):
    black = build(gauss, env_level0=np.zeros((8, 16, 3), np.float32)).desc()
    assert check(phip, created, look(black, envmap=True)) == (INVALID, "phip_scene_update_appearance: The environment map is completely black -- this is not allowed.")
    bad = np.full((8, 16, 3), 0.5, np.float32); bad[3, 4, 1] = np.inf
    rc, msg = check(phip, created, look(build(gauss, env_level0=bad).desc(), envmap=True))
    assert rc == INVALID and "invalid floating point value (nan/inf)" in msg
    singular = np.eye(4, dtype=np.float32); singular[1, 1] = 0.0
    assert check(phip, created, look(build(gauss, env_to_world=singular).desc(), envmap=True)) == (INVALID, "phip_scene_update_appearance: envmap toWorld is singular")
    turned = np.eye(4, dtype=np.float32); turned[0, 0] = turned[2, 2] = 0.0; turned[0, 2] = 1.0; turned[2, 0] = -1.0
    assert check(phip, created, look(build(gauss, env_to_world=turned).desc(), envmap=True))[0] == 0


# ---- appearance_hd.h on the host: the creation's environment-map tables --------------------------------------------------------------------------------------

def configure_restated(phip, tex):
    """envmap.cpp:262-328 in numpy float32: every sum sequential (np.cumsum accumulates in order), every product rounded on its own"""
    f = np.float32
    h, w = tex.shape[:2]
    lum = (tex[..., 0] * f(0.212671) + tex[..., 1] * f(0.715160)) + tex[..., 2] * f(0.072169)
    cols = np.zeros((h, w + 1), f)
    cols[:, 1:] = np.cumsum(lum, axis=1, dtype=f)
    col_sum = cols[:, w].copy()
    with np.errstate(all="ignore"):
        norm = f(1.0) / col_sum
        cols[:, 1:w] *= norm[:, None]
    cols[:, w] = 1.0
    theta = np.ascontiguousarray((np.arange(h, dtype=f) + f(0.5)) * f(np.pi) / f(h), dtype=f)
    sn = np.zeros(h, f)
    phip.phip_debug_fmath(0, 0, h, _ffi.fptr(theta), _ffi.fptr(theta), _ffi.fptr(sn))          # pm_sincosf's sine, the library's deterministic function
    rows = np.zeros(h + 1, f)
    rows[1:] = np.cumsum(col_sum * sn, dtype=f)
    row_sum = rows[h]
    rows[1:h] *= f(1.0) / row_sum
    rows[h] = 1.0
    normalization = f(1.0) / (row_sum * (f(2) * f(np.pi) / f(w)) * (f(np.pi) / f(h)))
    return cols, rows, sn, normalization


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 130)])
def test_the_creations_envmap_tables_are_the_restated_ones(phip, w, h):
    rng = np.random.default_rng(100 * w + h)
    tex = rng.uniform(0.0, 4.0, (h, w, 3)).astype(np.float32)
    if h > 2:
        tex[1] = 0.0                                                # an all-zero row: its conditional CDF is 0 * inf
        tex[h - 1] = 0.0; tex[h - 1, w // 2, 1] = 2.5               # a row with a single non-zero texel
    e = A.phip_envmap()
    e.texels = _ffi.fptr(tex); e.width, e.height, e.scale, e.n_levels = w, h, 1.0, 1
    e.to_world[:] = [float(v) for v in np.eye(4).reshape(-1)]
    cols, rows, weights, norm = np.zeros((h, w + 1), np.float32), np.zeros(h + 1, np.float32), np.zeros(h, np.float32), C.c_float()
    assert phip.phip_debug_host_envmap_cdf(C.byref(e), _ffi.fptr(cols), _ffi.fptr(rows), _ffi.fptr(weights), C.byref(norm)) == 0, _ffi.debug_lib().phip_last_error()
    want_cols, want_rows, want_weights, want_norm = configure_restated(phip, tex)
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert (u(weights) == u(want_weights)).all()
    nan = np.isnan(want_cols)
    assert (np.isnan(cols) == nan).all() and (nan.any() == (h > 2))                  # (the all-zero row; a NaN's sign is the host's business)
    assert (u(cols)[~nan] == u(want_cols)[~nan]).all()
    assert (u(rows) == u(want_rows)).all()
    assert u(np.float32(norm.value)) == u(want_norm)

"""phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device without a GPU: their place in the ABI, every refusal of their arguments through the debug
library's hooks on the functions the entry points call first (host_shading_parts.h), and the host twins -- the per-item statements of k_shading_parts.h the kernels
evaluate, run over the creation's host stages -- against the oracle, bit for bit.

The scenes are those of the GPU test (tests/test_gpu_shading_parts.py imports them from here), 16 x 16 pixels each."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi, scene as S
from test_raycast_device_host import host_surfaces, fields

HERE = os.path.dirname(os.path.abspath(__file__))
BUF = 4096                                                         # never dereferenced: the argument hooks look at values only
NO_HIT = 0xFFFFFFFF
W = H = 16
CU = dict(eta=S.CU_ETA, k=S.CU_K)
ONE_BELOW = np.float32(1) - np.float32(2 ** -24)


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------------------

def cornell(g):
    return S.cornell_box(W, H, g)


def mixed(g):
    """the Cornell box with a glass block, a block under a `twosided` that nests rough copper (Beckmann) in front of a diffuse back, a one-sided GGX copper quad and
    an anisotropic Beckmann one on a mesh with texture coordinates"""
    sb = S.cornell_box(W, H, g, short_bsdf=lambda b: b.twosided(b.roughconductor(alpha=0.1, **CU), b.diffuse((0.2, 0.5, 0.8))), tall_bsdf=lambda b: b.dielectric())
    sb.quad((60, 300, 300), (200, 300, 300), (200, 440, 350), (60, 440, 350), sb.roughconductor(alpha=0.2, distribution="ggx", **CU))
    sb.quad((350, 60, 100), (500, 60, 100), (500, 200, 150), (350, 200, 150), sb.twosided(sb.roughconductor(alpha=0.08, alpha_v=0.3, **CU)), uvs=True)
    return sb


def textured(g):
    """bitmap textures on a diffuse reflectance and on a copper roughness, on spheres with texture coordinates and vertex normals"""
    from test_gpu_appearance import textured_box
    sb = textured_box(g, (5, 7))
    sb.hdrfilm(W, H, g)
    return sb


def env_box(g, kind, light=True):
    """the open Cornell box under a `constant` or an `envmap` environment, seen from a camera that looks past its ceiling: hits and misses in one frame.
    light = False: the environment is the scene's only emitter (the oracle's environment hooks sample it without the emitter selection)"""
    from test_oracle_path import _sky
    sb = S.SceneBuilder()
    if kind == "constant":
        sb.constant((0.8, 0.9, 1.1))
    else:
        rng = np.random.default_rng(5)
        sb.envmap((_sky(16, 8) * rng.uniform(0.5, 1.5, (8, 16, 1))).astype(np.float32), scale=0.6, pyramid=True)
    if light:
        S.cornell_box(W, H, g, sb=sb)
    else:
        sb.quad((552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2), sb.diffuse((0.7, 0.7, 0.7)), facing=(0, 1, 0))
        sb.quad((130, 165, 65), (82, 165, 225), (240, 165, 272), (290, 165, 114), sb.twosided(sb.diffuse((0.3, 0.6, 0.3))), facing=(0, 1, 0))
    sb.perspective(origin=(278.0, 273.0, -300.0), target=(278.0, 400.0, 0.0), up=(0, 1, 0), fov_x_deg=80.0, near=10.0, far=2800.0)
    sb.hdrfilm(W, H, g)
    return sb


SCENES = {"cornell": cornell, "mixed": mixed, "textured": textured, "constant": lambda g: env_box(g, "constant"), "envmap": lambda g: env_box(g, "envmap")}


# ---- the host twins ------------------------------------------------------------------------------------------------------------------------------

def f32(a, cols):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, cols)
    assert a.ctypes.data % 16 == 0
    return a


def twin_bsdf(phip, desc, rays, hits, wo=None, samples=None, local=False, wi_local=True):
    """(eval, sampled, wi_local) as uint32 words, None where not asked for"""
    r, h = f32(rays, 8), f32(hits, 4); n = len(r)
    wo4 = None if wo is None else f32(np.concatenate([np.asarray(wo, np.float32).reshape(n, -1)[:, :3], np.zeros((n, 1), np.float32)], 1), 4)
    smp = None if samples is None else f32(samples, 2)
    ev = np.full((n, 4), 0xCDCDCDCD, np.uint32) if wo is not None else None
    sampled = np.full((n, 12), 0xCDCDCDCD, np.uint32) if samples is not None else None
    wi = np.full((n, 4), 0xCDCDCDCD, np.uint32) if wi_local else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    d = A.phip_bsdf_desc(d_rays=ptr(r), d_hits=ptr(h), n=n, d_wo=ptr(wo4), d_samples=ptr(smp), d_eval=ptr(ev), d_sampled=ptr(sampled), d_wi_local=ptr(wi),
                         flags=A.PHIP_BSDF_LOCAL if local else 0)
    rc = phip.phip_debug_host_bsdf_parts(C.byref(desc), C.byref(d))
    assert rc == 0, _ffi.debug_lib().phip_last_error()
    return ev, sampled, wi


def twin_emitter_sample(phip, desc, ref, ref_n, samples, shadow_rays=True):
    p = f32(np.concatenate([np.asarray(ref, np.float32).reshape(-1, 3), np.zeros((len(ref), 1), np.float32)], 1), 4); n = len(p)
    rn = None if ref_n is None else f32(np.concatenate([np.asarray(ref_n, np.float32).reshape(-1, 3), np.zeros((n, 1), np.float32)], 1), 4)
    smp = f32(samples, 2)
    sampled = np.full((n, 12), 0xCDCDCDCD, np.uint32); rays = np.full((n, 8), 0xCDCDCDCD, np.uint32) if shadow_rays else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    d = A.phip_emitter_sample_desc(d_ref=ptr(p), d_ref_n=ptr(rn), d_samples=ptr(smp), n=n, d_sampled=ptr(sampled), d_shadow_rays=ptr(rays))
    rc = phip.phip_debug_host_emitter_sample(C.byref(desc), C.byref(d))
    assert rc == 0, _ffi.debug_lib().phip_last_error()
    return sampled, rays


def twin_emitter_eval(phip, desc, rays, hits, ref_n=None):
    r, h = f32(rays, 8), f32(hits, 4); n = len(r)
    rn = None if ref_n is None else f32(np.concatenate([np.asarray(ref_n, np.float32).reshape(-1, 3), np.zeros((n, 1), np.float32)], 1), 4)
    ev = np.full((n, 4), 0xCDCDCDCD, np.uint32); em = np.full(n, 0x0DCDCDCD, np.int32)
    ptr = lambda a: a.ctypes.data if a is not None else None
    d = A.phip_emitter_eval_desc(d_rays=ptr(r), d_hits=ptr(h), d_ref_n=ptr(rn), n=n, d_eval=ptr(ev), d_emitter=ptr(em))
    rc = phip.phip_debug_host_emitter_eval(C.byref(desc), C.byref(d))
    assert rc == 0, _ffi.debug_lib().phip_last_error()
    return ev, em


def sampled_fields(words):
    f = words.view(np.float32)
    return dict(wo=f[:, 0:3], pdf=f[:, 3], weight=f[:, 4:7], eta=f[:, 7], flags=words[:, 8], reserved=words[:, 9:12])


def emitter_fields(words):
    f = words.view(np.float32)
    return dict(d=f[:, 0:3], dist=f[:, 3], value=f[:, 4:7], pdf=f[:, 7], emitter=words[:, 8].view(np.int32), reserved=words[:, 9:12])


def scene_rays(desc, n_random=600, seed=3):
    """rays that meet every shape from both sides (from just off the centroid of its first triangle, along the face normal) and random rays through the scene's box"""
    P = np.ctypeslib.as_array(desc.positions, shape=(desc.n_vertices, 3)).astype(np.float64)
    T = np.ctypeslib.as_array(desc.indices, shape=(desc.n_triangles, 3))
    rays = []
    for i in range(desc.n_shapes):
        a, b, c = P[T[desc.shapes[i].first_triangle]]
        n = np.cross(b - a, c - a); n /= np.linalg.norm(n)
        for s in (1.0, -1.0):
            rays.append(list((a + b + c) / 3 + s * 0.05 * n) + [1e-3] + list(-s * n) + [np.inf])
    rng = np.random.default_rng(seed)
    o = rng.uniform(P.min(0), P.max(0), (n_random, 3)); d = rng.normal(size=(n_random, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays += [list(o[i]) + [1e-3] + list(d[i]) + [np.inf] for i in range(n_random)]
    return np.asarray(rays, np.float32)


def sweep(oracle, desc, rays):
    osc = oracle.OracleScene(desc)
    hits, _, _ = osc.trace(rays, True, False, bruteforce=True)
    osc.close()
    return np.ascontiguousarray(hits, np.float32)


def unit(rng, n):
    v = rng.normal(size=(n, 3)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---- 1. the ABI -----------------------------------------------------------------------------------------------------------------------------------

def test_abi_of_the_three_entry_points(phip, have_gpu):
    header = open(os.path.join(HERE, "..", "include", "phip.h")).read()
    assert "int  phip_bsdf_device(phip_scene *scene, const phip_bsdf_desc *desc);" in header
    assert "int  phip_emitter_sample_device(phip_scene *scene, const phip_emitter_sample_desc *desc);" in header
    assert "int  phip_emitter_eval_device(phip_scene *scene, const phip_emitter_eval_desc *desc);" in header
    assert "#define PHIP_ABI_VERSION 7" in header
    assert phip.phip_abi_sizeof(23) == C.sizeof(A.phip_bsdf_desc) == 80
    assert phip.phip_abi_sizeof(24) == C.sizeof(A.phip_bsdf_sample) == 48
    assert phip.phip_abi_sizeof(25) == C.sizeof(A.phip_emitter_sample_desc) == 56
    assert phip.phip_abi_sizeof(26) == C.sizeof(A.phip_emitter_sample) == 48
    assert phip.phip_abi_sizeof(27) == C.sizeof(A.phip_emitter_eval_desc) == 56
    assert phip.phip_abi_sizeof(28) == 0 and phip.phip_abi_sizeof(22) == 0 and phip.phip_abi_sizeof(19) == 0
    assert phip.phip_abi_sizeof(20) == C.sizeof(A.phip_appearance_desc) and phip.phip_abi_sizeof(6) == C.sizeof(A.phip_render_params)      # nothing else moved
    offsets = lambda s: {n: getattr(s, n).offset for n, _ in s._fields_}
    assert offsets(A.phip_bsdf_desc) == dict(d_rays=0, d_hits=8, n=16, d_wo=24, d_samples=32, d_eval=40, d_sampled=48, d_wi_local=56, flags=64, reserved=68, stream=72)
    assert offsets(A.phip_bsdf_sample) == dict(wo=0, pdf=12, weight=16, eta=28, flags=32, reserved=36)
    assert offsets(A.phip_emitter_sample) == dict(d=0, dist=12, value=16, pdf=28, emitter=32, reserved=36)
    assert offsets(A.phip_emitter_sample_desc) == dict(d_ref=0, d_ref_n=8, d_samples=16, n=24, d_sampled=32, d_shadow_rays=40, stream=48)
    assert offsets(A.phip_emitter_eval_desc) == dict(d_rays=0, d_hits=8, d_ref_n=16, n=24, d_eval=32, d_emitter=40, stream=48)
    for name, value in (("PHIP_BSDF_SAMPLED_DELTA", 1), ("PHIP_BSDF_SAMPLED_VALID", 2), ("PHIP_BSDF_LOCAL", 1)):
        assert getattr(A, name) == value and "#define %s %du" % (name, value) in header
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB], capture_output=True, text=True).stdout
    assert " phip_bsdf_device" in out and " phip_emitter_sample_device" in out and " phip_emitter_eval_device" in out and "phip_debug_" not in out
    assert ("phip_shading_parts.hip", [], "phip_shading_parts.o") in _ffi.UNITS                               # a unit of its own
    for name in ("phip_shading_parts.hip", "host_shading_parts.h", "k_shading_parts.h"):
        assert os.path.exists(os.path.join(_ffi.CSRC, name)), name
    b = A.phip_bsdf_desc(d_rays=BUF, d_hits=BUF, n=4, d_wi_local=BUF)
    s = A.phip_emitter_sample_desc(d_ref=BUF, d_samples=BUF, n=4, d_sampled=BUF)
    e = A.phip_emitter_eval_desc(d_rays=BUF, d_hits=BUF, n=4, d_eval=BUF)
    never_read = C.create_string_buffer(64)
    scene = C.cast(never_read, C.c_void_p)
    for fn, d, who in ((phip.phip_bsdf_device, b, b"phip_bsdf_device: "), (phip.phip_emitter_sample_device, s, b"phip_emitter_sample_device: "),
                       (phip.phip_emitter_eval_device, e, b"phip_emitter_eval_device: ")):
        assert fn(None, C.byref(d)) == A.PHIP_ERR_INVALID and phip.phip_last_error().startswith(who)           # no scene
        assert fn(scene, None) == A.PHIP_ERR_INVALID and fn(None, None) == A.PHIP_ERR_INVALID
        d.n = 0
        assert fn(scene, C.byref(d)) == A.PHIP_OK                                                               # n == 0 touches nothing, the scene included
        d.n = 4
        if not have_gpu:
            assert fn(scene, C.byref(d)) == A.PHIP_ERR_DEVICE and phip.phip_last_error().startswith(who)       # no CPU fallback


# ---- 2. every refusal, without a device ----------------------------------------------------------------------------------------------------------------

def bsdf_check(phip, have_scene=1, **kw):
    d = A.phip_bsdf_desc(**dict(dict(d_rays=BUF, d_hits=BUF, n=5, d_wo=BUF, d_samples=BUF + 8, d_eval=BUF, d_sampled=BUF, d_wi_local=BUF, flags=0), **kw))
    rc = phip.phip_debug_host_bsdf_args(have_scene, C.byref(d))
    assert rc in (0, A.PHIP_ERR_INVALID) and ((rc == 0) or _ffi.debug_lib().phip_last_error().startswith(b"phip_bsdf_device: "))
    return rc


def sample_check(phip, have_scene=1, **kw):
    d = A.phip_emitter_sample_desc(**dict(dict(d_ref=BUF, d_ref_n=BUF, d_samples=BUF + 8, n=5, d_sampled=BUF, d_shadow_rays=BUF), **kw))
    rc = phip.phip_debug_host_emitter_sample_args(have_scene, C.byref(d))
    assert rc in (0, A.PHIP_ERR_INVALID) and ((rc == 0) or _ffi.debug_lib().phip_last_error().startswith(b"phip_emitter_sample_device: "))
    return rc


def eval_check(phip, have_scene=1, **kw):
    d = A.phip_emitter_eval_desc(**dict(dict(d_rays=BUF, d_hits=BUF, d_ref_n=BUF, n=5, d_eval=BUF, d_emitter=BUF), **kw))
    rc = phip.phip_debug_host_emitter_eval_args(have_scene, C.byref(d))
    assert rc in (0, A.PHIP_ERR_INVALID) and ((rc == 0) or _ffi.debug_lib().phip_last_error().startswith(b"phip_emitter_eval_device: "))
    return rc


LIMIT = 2 ** 32 - 256


def test_bsdf_argument_checks_that_need_no_device(phip):
    INV = A.PHIP_ERR_INVALID
    assert bsdf_check(phip) == 0 and bsdf_check(phip, flags=A.PHIP_BSDF_LOCAL) == 0
    assert bsdf_check(phip, have_scene=0) == INV and phip.phip_debug_host_bsdf_args(1, None) == INV
    assert bsdf_check(phip, d_rays=None) == INV and bsdf_check(phip, d_hits=None) == INV
    assert bsdf_check(phip, d_eval=None, d_sampled=None, d_wi_local=None) == INV                                # no output
    assert bsdf_check(phip, d_wo=None) == INV and bsdf_check(phip, d_wo=None, d_eval=None) == 0                 # an output without its input
    assert bsdf_check(phip, d_samples=None) == INV and bsdf_check(phip, d_samples=None, d_sampled=None) == 0
    assert bsdf_check(phip, d_eval=None, d_sampled=None) == 0                                                   # wi alone; the unused inputs may stay
    for name in ("d_rays", "d_hits", "d_wo", "d_eval", "d_sampled", "d_wi_local"):
        assert bsdf_check(phip, **{name: BUF + 8}) == INV, name
    assert bsdf_check(phip, d_samples=BUF + 4) == INV and bsdf_check(phip, d_samples=BUF) == 0
    assert bsdf_check(phip, flags=2) == INV and bsdf_check(phip, flags=3) == INV
    assert bsdf_check(phip, n=LIMIT) == 0 and bsdf_check(phip, n=LIMIT + 1) == INV
    assert bsdf_check(phip, n=0, d_rays=None, d_hits=None, d_wo=None, d_samples=None, d_eval=None, d_sampled=None, d_wi_local=None) == 0      # n == 0: no pointer is looked at
    assert bsdf_check(phip, n=0, flags=2) == INV


def test_emitter_sample_argument_checks_that_need_no_device(phip):
    INV = A.PHIP_ERR_INVALID
    assert sample_check(phip) == 0 and sample_check(phip, d_ref_n=None, d_shadow_rays=None) == 0
    assert sample_check(phip, have_scene=0) == INV and phip.phip_debug_host_emitter_sample_args(1, None) == INV
    for name in ("d_ref", "d_samples", "d_sampled"):
        assert sample_check(phip, **{name: None}) == INV, name
    for name in ("d_ref", "d_ref_n", "d_sampled", "d_shadow_rays"):
        assert sample_check(phip, **{name: BUF + 8}) == INV, name
    assert sample_check(phip, d_samples=BUF + 4) == INV
    assert sample_check(phip, n=LIMIT) == 0 and sample_check(phip, n=LIMIT + 1) == INV
    assert sample_check(phip, n=0, d_ref=None, d_samples=None, d_sampled=None) == 0


def test_emitter_eval_argument_checks_that_need_no_device(phip):
    INV = A.PHIP_ERR_INVALID
    assert eval_check(phip) == 0 and eval_check(phip, d_ref_n=None, d_emitter=None) == 0
    assert eval_check(phip, have_scene=0) == INV and phip.phip_debug_host_emitter_eval_args(1, None) == INV
    for name in ("d_rays", "d_hits", "d_eval"):
        assert eval_check(phip, **{name: None}) == INV, name
    for name in ("d_rays", "d_hits", "d_ref_n", "d_eval", "d_emitter"):
        assert eval_check(phip, **{name: BUF + 8}) == INV, name
    assert eval_check(phip, n=LIMIT) == 0 and eval_check(phip, n=LIMIT + 1) == INV
    assert eval_check(phip, n=0, d_rays=None, d_hits=None, d_eval=None) == 0


def test_wrappers_refuse_tensors_they_cannot_pass_on():
    torch = pytest.importorskip("torch")
    import types
    from mitsuba_amd.integrator import Scene
    scene = types.SimpleNamespace(device=0, _device_tensor=lambda *a, **k: Scene._device_tensor(scene, *a, **k))
    rays, hits = torch.zeros((8, 8)), torch.zeros((8, 4))
    for bad in (torch.zeros((8, 8)).double(), torch.zeros((8, 16))[:, :8], torch.zeros((8, 7)), np.zeros((8, 8), np.float32), rays):      # (the last: not on the device)
        with pytest.raises(ValueError):
            Scene.bsdf(scene, bad, hits)
        with pytest.raises(ValueError):
            Scene.emitter_eval(scene, bad, hits)
    with pytest.raises(ValueError):
        Scene.emitter_sample(scene, torch.zeros((8, 3)), None, torch.zeros((8, 2)))


# ---- 3. the host twins against the oracle ---------------------------------------------------------------------------------------------------------------

def test_bsdf_twin_equals_the_oracle_on_every_material_and_side(phip, oracle, gauss):
    desc = mixed(gauss).desc()
    rays = scene_rays(desc)
    hits = sweep(oracle, desc, rays)
    n = len(rays)
    rng = np.random.default_rng(21)
    wo = unit(rng, n); smp = np.minimum(rng.random((n, 2)).astype(np.float32), ONE_BELOW)
    ev, sampled, wi = twin_bsdf(phip, desc, rays, hits, wo=wo, samples=smp, local=True)
    prim = hits.view(np.uint32)[:, 3]
    hit = prim != NO_HIT
    assert hit.sum() > 400 and (~hit).sum() > 0
    assert (ev[~hit] == 0).all() and (sampled[~hit] == 0).all() and (wi[~hit] == 0).all()                      # a miss: zeros in every output
    surf = fields(host_surfaces(phip, desc, rays, hits))
    wif = wi.view(np.float32)
    assert (wi[:, 3] == 0).all()
    # wi is the frame's toLocal(-d): its z is dot(-d, ns), the sign the surface record's side flag is made of
    assert (((surf["flags"] & A.PHIP_SURFACE_BACK) != 0) == (wif[:, 2] <= 0))[hit].all()
    shape_of = np.zeros(desc.n_triangles, np.int64)
    for i in range(desc.n_shapes):
        shape_of[desc.shapes[i].first_triangle:desc.shapes[i].first_triangle + desc.shapes[i].n_triangles] = i
    mat = np.array([desc.shapes[i].material for i in range(desc.n_shapes)])[shape_of[np.where(hit, prim, 0)]]
    osc = oracle.OracleScene(desc); OL = oracle.lib()
    s = sampled_fields(sampled)
    sides = set()
    for m in sorted(set(mat[hit].tolist())):
        sel = hit & (mat == m)
        k = int(sel.sum())
        wi3 = np.ascontiguousarray(wif[sel, :3]); wo3 = np.ascontiguousarray(wo[sel]); sm = np.ascontiguousarray(smp[sel])
        v = np.zeros((k, 3), np.float32); p = np.zeros(k, np.float32)
        OL.oracle_bsdf_eval_pdf(osc.h, m, k, fp(wi3), fp(wo3), fp(v), fp(p))
        assert (ev[sel, :3] == v.view(np.uint32)).all() and (ev[sel, 3] == p.view(np.uint32)).all(), m
        owo = np.zeros((k, 3), np.float32); ow = np.zeros((k, 3), np.float32); op = np.zeros(k, np.float32); od = np.zeros(k, np.uint8)
        OL.oracle_bsdf_sample(osc.h, m, k, fp(wi3), fp(sm), fp(owo), fp(ow), fp(op), od.ctypes.data_as(C.POINTER(C.c_uint8)))
        ok = (ow != 0).any(axis=1)
        assert (s["weight"][sel].view(np.uint32) == ow.view(np.uint32)).all(), m
        assert (s["pdf"][sel][ok].view(np.uint32) == op[ok].view(np.uint32)).all() and (s["wo"][sel][ok].view(np.uint32) == owo[ok].view(np.uint32)).all(), m
        assert (((s["flags"][sel] & A.PHIP_BSDF_SAMPLED_DELTA) != 0)[ok] == (od[ok] != 0)).all(), m
        assert (((s["flags"][sel] & A.PHIP_BSDF_SAMPLED_VALID) != 0) == ok).all() and (sampled[sel][~ok] == 0).all(), m      # a failed sample is all zero
        sides |= {(m, bool(z)) for z in (wif[sel, 2] > 0)}
    osc.close()
    assert (s["reserved"] == 0).all() and (s["flags"] & ~np.uint32(3) == 0).all()
    shape_mats = sorted({desc.shapes[i].material for i in range(desc.n_shapes)})
    assert sorted(sides) == [(m, side) for m in shape_mats for side in (False, True)], sides                  # every material of a shape, both sides
    types_ = {desc.materials[m].type for m in shape_mats}
    assert types_ == {A.PHIP_BSDF_DIFFUSE, A.PHIP_BSDF_DIELECTRIC, A.PHIP_BSDF_ROUGHCONDUCTOR, A.PHIP_BSDF_TWOSIDED}
    eta = s["eta"][hit & ((s["flags"] & A.PHIP_BSDF_SAMPLED_VALID) != 0)]
    assert (eta != 1).any() and (eta == 1).any()                                                                # refraction through the glass, and none elsewhere


def test_world_space_mode_is_the_frames_to_world_of_the_local_result(phip, oracle, gauss):
    desc = mixed(gauss).desc()
    rays = scene_rays(desc, 400, seed=4)
    hits = sweep(oracle, desc, rays)
    n = len(rays)
    rng = np.random.default_rng(22)
    smp = np.minimum(rng.random((n, 2)).astype(np.float32), ONE_BELOW)
    _, loc, wi_l = twin_bsdf(phip, desc, rays, hits, samples=smp, local=True)
    _, wld, wi_w = twin_bsdf(phip, desc, rays, hits, samples=smp, local=False)
    assert (wi_l == wi_w).all()
    assert (loc[:, 3:] == wld[:, 3:]).all()                                                                     # pdf, weight, eta, flags: the frame does not enter
    a, b = sampled_fields(loc), sampled_fields(wld)
    ok = (a["flags"] & A.PHIP_BSDF_SAMPLED_VALID) != 0
    assert ok.sum() > 200
    ns = fields(host_surfaces(phip, desc, rays, hits))["ns"][ok].astype(np.float64)
    wl, ww = a["wo"][ok].astype(np.float64), b["wo"][ok].astype(np.float64)
    # wo_world = s x + t y + n z in float32, so dot(n, wo_world) - z = z (|n|^2 - 1) + x (n.s) + y (n.t) + n.delta, delta the rounding of the three sums.
    # With u = 2^-24: a normalised float32 vector has | |n|^2 - 1 | <= 6 u (three products, two sums, the root and the division of normalize), the frame's
    # n.s and n.t are each the rounding of a Gram-Schmidt step and a normalisation, <= 6 u, and every component of wo_world carries at most three roundings of a
    # sum of magnitude <= |x| + |y| + |z| <= sqrt(3), so |n.delta| <= 3 sqrt(3) u |n|_1 / sqrt(3) ... <= 6 u.  Together (|x| + |y| + |z| <= sqrt(3)):
    # 6 u sqrt(3) + 6 u + 6 u < 24 u; the bound below is 32 u = 32 * 2^-24, "a few ulp of a three-term dot product".
    bound = 32 * 2.0 ** -24
    assert np.abs(np.einsum("ij,ij->i", ns, ww) - wl[:, 2]).max() <= bound
    assert np.abs(np.linalg.norm(ww, axis=1) - np.linalg.norm(wl, axis=1)).max() <= bound and np.abs(np.linalg.norm(ww, axis=1) - 1).max() <= 2 * bound
    # eval in world space: toLocal of the world direction the sample came back as gives the local direction up to that rounding, so value and pdf agree closely
    ev_l, _, _ = twin_bsdf(phip, desc, rays, hits, wo=a["wo"], local=True)
    ev_w, _, _ = twin_bsdf(phip, desc, rays, hits, wo=b["wo"], local=False)
    smooth = ok & ((a["flags"] & A.PHIP_BSDF_SAMPLED_DELTA) == 0)
    assert np.allclose(ev_l.view(np.float32)[smooth], ev_w.view(np.float32)[smooth], rtol=2e-3, atol=1e-6)


def light_triangle(desc):
    sh = next(desc.shapes[i] for i in range(desc.n_shapes) if desc.shapes[i].emitter >= 0)
    return sh.first_triangle


def test_emitter_sample_twin_equals_the_oracle_on_area_emitters(phip, oracle, gauss):
    desc = cornell(gauss).desc()
    osc = oracle.OracleScene(desc); OL = oracle.lib()
    rng = np.random.default_rng(23)
    m = 257
    for trial in range(6):
        refp = rng.uniform(100, 450, 3).astype(np.float32)
        refn = unit(rng, 1)[0] if trial else np.zeros(3, np.float32)                                           # (the first: a point on no surface)
        refn[1] = abs(refn[1])                                                                                 # (the light is above: part of it in front of the point)
        smp = np.minimum(rng.random((m, 2)).astype(np.float32), ONE_BELOW)
        od = np.zeros((m, 3), np.float32); odist = np.zeros(m, np.float32); opdf = np.zeros(m, np.float32); oval = np.zeros((m, 3), np.float32); ochk = np.zeros(m, np.float32)
        OL.oracle_sample_emitter(osc.h, fp(refp), fp(refn), m, fp(smp), fp(od), fp(odist), fp(opdf), fp(oval), fp(ochk))
        sampled, srays = twin_emitter_sample(phip, desc, np.tile(refp, (m, 1)), None if trial == 0 else np.tile(refn, (m, 1)), smp)
        s = emitter_fields(sampled)
        ok = opdf != 0
        assert ok.sum() > 20
        assert (s["pdf"].view(np.uint32) == opdf.view(np.uint32)).all() and (s["value"].view(np.uint32) == oval.view(np.uint32)).all()
        assert (s["d"][ok].view(np.uint32) == od[ok].view(np.uint32)).all() and (s["dist"][ok].view(np.uint32) == odist[ok].view(np.uint32)).all()
        assert (s["emitter"][ok] == 0).all() and (s["emitter"][~ok] == -1).all() and (np.delete(sampled[~ok], 8, axis=1) == 0).all() and (s["reserved"] == 0).all()
        # the shadow ray: (ref, Epsilon, d, dist (1 - ShadowEpsilon)); the empty interval without a sample
        sr = srays.view(np.float32)
        assert (sr[:, :3].view(np.uint32) == refp.view(np.uint32)).all()
        assert (sr[ok, 3] == np.float32(1e-4)).all() and (sr[ok, 4:7].view(np.uint32) == od[ok].view(np.uint32)).all()
        assert (sr[ok, 7].view(np.uint32) == (odist[ok] * (np.float32(1) - np.float32(1e-3))).view(np.uint32)).all()
        assert (sr[~ok, 3] == 0).all() and (sr[~ok, 7] == -1).all() and (sr[~ok, 4:7] == 0).all()
        # pdfEmitterDirect of the sampled record, from the other entry point: a hit on the (flat) light at distance dist along d
        hits = np.zeros((m, 4), np.float32); hits[:, 0] = s["dist"]; hits[:, 1:3] = 0.25; hits.view(np.uint32)[:, 3] = np.where(ok, light_triangle(desc), NO_HIT)
        rays = np.concatenate([sr[:, :4], s["d"], np.full((m, 1), np.inf, np.float32)], 1)
        ev, em = twin_emitter_eval(phip, desc, rays, hits, None if trial == 0 else np.tile(refn, (m, 1)))
        assert (ev[ok, 3] == ochk[ok].view(np.uint32)).all() and (em[ok] == 0).all()
        assert (ev[~ok] == 0).all() and (em[~ok] == -1).all()
        assert (ev.view(np.float32)[ok, :3] == np.array(desc.emitters[0].radiance, np.float32)).all()          # Le(-d): the sample lies on the front of the light
    osc.close()


@pytest.mark.parametrize("kind", ["constant", "envmap"])
def test_environment_twins_equal_the_oracle(phip, oracle, gauss, kind):
    desc = env_box(gauss, kind, light=False).desc()
    osc = oracle.OracleScene(desc); OL = oracle.lib()
    rng = np.random.default_rng(24)
    m = 257
    refp = np.array([250.0, 120.0, 200.0], np.float32)
    smp = np.minimum(rng.random((m, 2)).astype(np.float32), ONE_BELOW)
    od = np.zeros((m, 3), np.float32); opdf = np.zeros(m, np.float32); oval = np.zeros((m, 3), np.float32)
    assert OL.oracle_env_sample_direct(osc.h, fp(refp), m, fp(smp), fp(od), fp(opdf), fp(oval)) == 0
    sampled, srays = twin_emitter_sample(phip, desc, np.tile(refp, (m, 1)), None, smp)
    s = emitter_fields(sampled)
    ok = opdf != 0
    assert ok.sum() > 200
    assert (s["pdf"].view(np.uint32) == opdf.view(np.uint32)).all() and (s["value"].view(np.uint32) == oval.view(np.uint32)).all()
    assert (s["d"][ok].view(np.uint32) == od[ok].view(np.uint32)).all() and (s["emitter"][ok] == 0).all() and (s["dist"][ok] > 0).all()
    # the density of the same directions from the other entry point: rays that leave the scene
    dirs = np.ascontiguousarray(np.where(ok[:, None], od, unit(rng, m)))
    want = np.zeros(m, np.float32)
    assert OL.oracle_env_pdf_direct(osc.h, fp(refp), m, fp(dirs), fp(want)) == 0
    rays = np.concatenate([np.tile(refp, (m, 1)), np.full((m, 1), 1e-4, np.float32), dirs, np.full((m, 1), np.inf, np.float32)], 1).astype(np.float32)
    hits = np.zeros((m, 4), np.float32); hits.view(np.uint32)[:, 3] = NO_HIT
    ev, em = twin_emitter_eval(phip, desc, rays, hits)
    assert (ev[:, 3] == want.view(np.uint32)).all() and (em == 0).all()
    if kind == "constant":
        assert (ev.view(np.float32)[:, :3] == np.array(desc.emitters[0].radiance, np.float32)).all()
    else:
        assert (ev.view(np.float32)[:, :3] >= 0).all() and (ev.view(np.float32)[:, :3] > 0).any()
    osc.close()


def test_a_scene_without_emitters_has_no_sample_and_no_radiance(phip, oracle, gauss):
    sb = S.SceneBuilder()
    sb.quad((552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2), sb.diffuse((0.7, 0.7, 0.7)), facing=(0, 1, 0))
    sb.perspective(origin=(278.0, 273.0, -800.0), target=(278.0, 273.0, -799.0), up=(0, 1, 0), fov_x_deg=39.3077, near=10.0, far=2800.0)
    sb.hdrfilm(W, H, gauss)
    desc = sb.desc()
    rng = np.random.default_rng(25)
    sampled, srays = twin_emitter_sample(phip, desc, rng.uniform(0, 500, (65, 3)), unit(rng, 65), rng.random((65, 2)))
    s = emitter_fields(sampled)
    assert (s["emitter"] == -1).all() and (np.delete(sampled, 8, axis=1) == 0).all()
    assert (srays.view(np.float32)[:, 3] == 0).all() and (srays.view(np.float32)[:, 7] == -1).all()
    rays = scene_rays(desc, 63)
    ev, em = twin_emitter_eval(phip, desc, rays, sweep(oracle, desc, rays))
    assert (ev == 0).all() and (em == -1).all()

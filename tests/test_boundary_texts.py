"""The texts of the boundary, pinned: what the entry points on the caller's device memory return and say (mitsuba_amd/csrc/host_boundary.h and the guard of
phip.hip), byte for byte.  The tables below were recorded from a build of the commit before the boundary was restated in one place; a later entry point of
the family adds its rows.

Without a device: every distinct refusal of the six `*ArgsError` functions through the debug library's hooks, the NULL-argument case of the ten guarded entry
points, and -- where no device is visible -- what each of the ten returns once its own checks have passed.  The scene handle is memory that is never read.
On the GPU: one test on the Cornell box of tests/ref_scenes.py with arrays of 257 items (one block of 256 and one lane of the next; phip_film_device takes
the crop window's own 24 x 24 samples, which the scene fixes): a host pointer in place of a device array, another device in the parameters, and the scene's
stream against a caller's."""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi

BUF = 4096                                                          # never dereferenced: the checks look at values only
LIMIT = 2 ** 32 - 256
INV, UNS, DEV = A.PHIP_ERR_INVALID, A.PHIP_ERR_UNSUPPORTED, A.PHIP_ERR_DEVICE
PAIRS = A.PHIP_RADIANCE_STREAM_PAIRS
LD = A.PHIP_SAMPLER_LD
CTR_ONLY = "PHIP_SAMPLER_CTR only: the other samplers' streams are addressed by film coordinates"
ONE_DEVICE = "one device: the buffers are device memory of the scene's device (n_devices must be 0 or 1)"

# arguments that pass every check of the call: (render parameters or have_scene, descriptor)
GOOD = {
    "radiance": (dict(spp=1), dict(d_rays=BUF, n=5, d_stream=BUF, first_stream=0, reserved=0, d_out=BUF)),
    "camera_rays": (dict(spp=1), dict(d_pixels=BUF, m=5, d_rays=BUF, d_keys=BUF, d_positions=BUF)),
    "film": (dict(spp=1), dict(d_values=BUF, d_out=BUF, flags=0, reserved=0)),
    "bsdf": (1, dict(d_rays=BUF, d_hits=BUF, n=5, d_wo=BUF, d_samples=BUF + 8, d_eval=BUF, d_sampled=BUF, d_wi_local=BUF, flags=0)),
    "emitter_sample": (1, dict(d_ref=BUF, d_ref_n=BUF, d_samples=BUF + 8, n=5, d_sampled=BUF, d_shadow_rays=BUF)),
    "emitter_eval": (1, dict(d_rays=BUF, d_hits=BUF, d_ref_n=BUF, n=5, d_eval=BUF, d_emitter=BUF)),
}
DESC = {"radiance": A.phip_radiance_desc, "camera_rays": A.phip_camera_rays_desc, "film": A.phip_film_desc, "bsdf": A.phip_bsdf_desc,
        "emitter_sample": A.phip_emitter_sample_desc, "emitter_eval": A.phip_emitter_eval_desc}

# (call, what differs from GOOD in the parameters / have_scene -- None: NULL --, what differs in the descriptor -- None: NULL --, code, text)
REFUSALS = [
    ("radiance", None, {}, INV, "phip_radiance_device: NULL argument"),
    ("radiance", {}, None, INV, "phip_radiance_device: NULL argument"),
    ("radiance", dict(integrator=3), {}, INV, "phip_radiance_device: unknown integrator kind"),
    ("radiance", dict(sampler=6), {}, INV, "phip_radiance_device: unknown sampler kind"),
    ("radiance", dict(devices=[0, 1]), {}, INV, "phip_radiance_device: one device: the rays and the result are device memory of the scene's device (n_devices must be 0 or 1)"),
    ("radiance", dict(n_devices=-1), {}, INV, "phip_radiance_device: one device: the rays and the result are device memory of the scene's device (n_devices must be 0 or 1)"),
    ("radiance", dict(flags=A.PHIP_FLAG_SAMPLE_BUFFER), {}, INV, "phip_radiance_device: PHIP_FLAG_SAMPLE_BUFFER and PHIP_FLAG_ACCUMULATE concern the film: the call has none"),
    ("radiance", dict(flags=A.PHIP_FLAG_ACCUMULATE), {}, INV, "phip_radiance_device: PHIP_FLAG_SAMPLE_BUFFER and PHIP_FLAG_ACCUMULATE concern the film: the call has none"),
    ("radiance", {}, dict(n=LIMIT + 1), INV, "phip_radiance_device: more than 2^32 - 256 rays in one call"),
    ("radiance", {}, dict(d_rays=None), INV, "phip_radiance_device: d_rays and d_out must not be NULL"),
    ("radiance", {}, dict(d_out=None), INV, "phip_radiance_device: d_rays and d_out must not be NULL"),
    ("radiance", {}, dict(d_rays=BUF + 8), INV, "phip_radiance_device: d_rays and d_out must be 16-byte aligned"),
    ("radiance", {}, dict(d_out=BUF + 8), INV, "phip_radiance_device: d_rays and d_out must be 16-byte aligned"),
    ("radiance", {}, dict(d_stream=BUF + 2), INV, "phip_radiance_device: d_stream must be 4-byte aligned"),
    ("radiance", {}, dict(reserved=2), INV, "phip_radiance_device: unknown stream_layout"),
    ("radiance", dict(sample_offset=1), dict(reserved=PAIRS), INV, "phip_radiance_device: PHIP_RADIANCE_STREAM_PAIRS: the sample index is the pair's, sample_offset must be 0"),
    ("radiance", {}, dict(reserved=PAIRS, d_stream=None), INV, "phip_radiance_device: PHIP_RADIANCE_STREAM_PAIRS: d_stream must not be NULL"),
    ("radiance", {}, dict(reserved=PAIRS, d_stream=BUF + 4), INV, "phip_radiance_device: PHIP_RADIANCE_STREAM_PAIRS: d_stream must be 8-byte aligned"),
    ("radiance", dict(integrator=A.PHIP_INTEGRATOR_DIRECT), {}, UNS, "phip_radiance_device: PHIP_INTEGRATOR_DIRECT is not served: its sample arrays are addressed by film coordinates"),
    ("radiance", dict(sampler=LD), {}, UNS, "phip_radiance_device: " + CTR_ONLY),
    ("radiance", {}, dict(n=LIMIT), 0, None),
    ("radiance", {}, dict(n=0, d_rays=None, d_out=None, d_stream=BUF + 2), 0, None),

    ("camera_rays", None, {}, INV, "phip_camera_rays_device: NULL argument"),
    ("camera_rays", {}, None, INV, "phip_camera_rays_device: NULL argument"),
    ("camera_rays", dict(sampler=6), {}, INV, "phip_camera_rays_device: unknown sampler kind"),
    ("camera_rays", dict(devices=[0, 1]), {}, INV, "phip_camera_rays_device: " + ONE_DEVICE),
    ("camera_rays", dict(spp=0), {}, INV, "phip_camera_rays_device: spp must be > 0"),
    ("camera_rays", dict(sample_offset=-1), {}, INV, "phip_camera_rays_device: sample_offset must not be negative"),
    ("camera_rays", dict(sample_offset=0x7FFFFFFF), {}, INV, "phip_camera_rays_device: sample_offset + spp exceeds the 31 bits of a sample index"),
    ("camera_rays", {}, dict(d_rays=None), INV, "phip_camera_rays_device: d_rays must not be NULL"),
    ("camera_rays", {}, dict(d_rays=BUF + 8), INV, "phip_camera_rays_device: d_rays must be 16-byte aligned"),
    ("camera_rays", {}, dict(d_keys=BUF + 4), INV, "phip_camera_rays_device: d_keys and d_positions must be 8-byte aligned"),
    ("camera_rays", {}, dict(d_positions=BUF + 4), INV, "phip_camera_rays_device: d_keys and d_positions must be 8-byte aligned"),
    ("camera_rays", {}, dict(d_pixels=BUF + 2), INV, "phip_camera_rays_device: d_pixels must be 4-byte aligned"),
    ("camera_rays", {}, dict(m=LIMIT + 1), INV, "phip_camera_rays_device: more than 2^32 - 256 samples in one call"),
    ("camera_rays", dict(spp=2), dict(m=LIMIT // 2 + 1), INV, "phip_camera_rays_device: more than 2^32 - 256 samples in one call"),
    ("camera_rays", dict(sampler=LD), {}, UNS, "phip_camera_rays_device: " + CTR_ONLY),
    ("camera_rays", {}, dict(m=LIMIT), 0, None),
    ("camera_rays", {}, dict(m=0, d_rays=None, d_keys=BUF + 4), 0, None),          # an empty list: no pointer is looked at

    ("film", None, {}, INV, "phip_film_device: NULL argument"),
    ("film", {}, None, INV, "phip_film_device: NULL argument"),
    ("film", dict(sampler=6), {}, INV, "phip_film_device: unknown sampler kind"),
    ("film", dict(n_devices=-1), {}, INV, "phip_film_device: " + ONE_DEVICE),
    ("film", dict(spp=0), {}, INV, "phip_film_device: spp must be > 0"),
    ("film", dict(sample_offset=-1), {}, INV, "phip_film_device: sample_offset must not be negative"),
    ("film", dict(sample_offset=0x7FFFFFFF), {}, INV, "phip_film_device: sample_offset + spp exceeds the 31 bits of a sample index"),
    ("film", dict(shard_count=2), {}, INV, "phip_film_device: shard_count > 1: the call puts every sample of the crop window"),
    ("film", dict(block_size=1), {}, INV, "phip_film_device: block_size must be a power of two in [2,128]"),
    ("film", dict(block_size=48), {}, INV, "phip_film_device: block_size must be a power of two in [2,128]"),
    ("film", dict(block_size=256), {}, INV, "phip_film_device: block_size must be a power of two in [2,128]"),
    ("film", {}, dict(d_values=None), INV, "phip_film_device: d_values and d_out must not be NULL"),
    ("film", {}, dict(d_out=None), INV, "phip_film_device: d_values and d_out must not be NULL"),
    ("film", {}, dict(d_values=BUF + 8), INV, "phip_film_device: d_values and d_out must be 16-byte aligned"),
    ("film", {}, dict(d_out=BUF + 4), INV, "phip_film_device: d_values and d_out must be 16-byte aligned"),
    ("film", {}, dict(flags=2), INV, "phip_film_device: unknown flag"),
    ("film", dict(sampler=LD), {}, UNS, "phip_film_device: " + CTR_ONLY),
    ("film", dict(block_size=0), dict(flags=A.PHIP_FILM_SIGNED), 0, None),

    ("bsdf", 0, {}, INV, "phip_bsdf_device: NULL argument"),
    ("bsdf", 1, None, INV, "phip_bsdf_device: NULL argument"),
    ("bsdf", 1, dict(flags=2), INV, "phip_bsdf_device: unknown flag"),
    ("bsdf", 1, dict(n=0, flags=2), INV, "phip_bsdf_device: unknown flag"),
    ("bsdf", 1, dict(n=LIMIT + 1), INV, "phip_bsdf_device: more than 2^32 - 256 items in one call"),
    ("bsdf", 1, dict(d_rays=None), INV, "phip_bsdf_device: d_rays and d_hits must not be NULL"),
    ("bsdf", 1, dict(d_hits=None), INV, "phip_bsdf_device: d_rays and d_hits must not be NULL"),
    ("bsdf", 1, dict(d_eval=None, d_sampled=None, d_wi_local=None), INV, "phip_bsdf_device: no output: one of d_eval, d_sampled and d_wi_local must be set"),
    ("bsdf", 1, dict(d_wo=None), INV, "phip_bsdf_device: d_eval needs d_wo"),
    ("bsdf", 1, dict(d_samples=None), INV, "phip_bsdf_device: d_sampled needs d_samples"),
    ("bsdf", 1, dict(d_samples=BUF + 4), INV, "phip_bsdf_device: d_samples must be 8-byte aligned"),
    ("bsdf", 1, dict(n=LIMIT), 0, None),
    ("bsdf", 1, dict(n=0, d_rays=None, d_hits=BUF + 8), 0, None),                  # n == 0: no pointer is looked at

    ("emitter_sample", 0, {}, INV, "phip_emitter_sample_device: NULL argument"),
    ("emitter_sample", 1, None, INV, "phip_emitter_sample_device: NULL argument"),
    ("emitter_sample", 1, dict(n=LIMIT + 1), INV, "phip_emitter_sample_device: more than 2^32 - 256 items in one call"),
    ("emitter_sample", 1, dict(d_samples=BUF + 4), INV, "phip_emitter_sample_device: d_samples must be 8-byte aligned"),
    ("emitter_sample", 1, dict(n=LIMIT, d_ref_n=None, d_shadow_rays=None), 0, None),
    ("emitter_sample", 1, dict(n=0, d_ref=None), 0, None),

    ("emitter_eval", 0, {}, INV, "phip_emitter_eval_device: NULL argument"),
    ("emitter_eval", 1, None, INV, "phip_emitter_eval_device: NULL argument"),
    ("emitter_eval", 1, dict(n=LIMIT + 1), INV, "phip_emitter_eval_device: more than 2^32 - 256 items in one call"),
    ("emitter_eval", 1, dict(n=LIMIT, d_ref_n=None, d_emitter=None), 0, None),
    ("emitter_eval", 1, dict(n=0, d_rays=None), 0, None),
]
REFUSALS += [("bsdf", 1, {name: BUF + 8}, INV, "phip_bsdf_device: d_rays, d_hits, d_wo, d_eval, d_sampled and d_wi_local must be 16-byte aligned")
             for name in ("d_rays", "d_hits", "d_wo", "d_eval", "d_sampled", "d_wi_local")]
REFUSALS += [("emitter_sample", 1, {name: None}, INV, "phip_emitter_sample_device: d_ref, d_samples and d_sampled must not be NULL") for name in ("d_ref", "d_samples", "d_sampled")]
REFUSALS += [("emitter_sample", 1, {name: BUF + 8}, INV, "phip_emitter_sample_device: d_ref, d_ref_n, d_sampled and d_shadow_rays must be 16-byte aligned")
             for name in ("d_ref", "d_ref_n", "d_sampled", "d_shadow_rays")]
REFUSALS += [("emitter_eval", 1, {name: None}, INV, "phip_emitter_eval_device: d_rays, d_hits and d_eval must not be NULL") for name in ("d_rays", "d_hits", "d_eval")]
REFUSALS += [("emitter_eval", 1, {name: BUF + 8}, INV, "phip_emitter_eval_device: d_rays, d_hits, d_ref_n, d_eval and d_emitter must be 16-byte aligned")
             for name in ("d_rays", "d_hits", "d_ref_n", "d_eval", "d_emitter")]

NO_DEVICE = "no HIP device visible: path_hip has no CPU fallback"
# the ten guarded entry points: (call, which argument is NULL, code, text) ...
NULL_ARGUMENTS = [
    ("scene_update", "scene", INV, "NULL argument"), ("scene_update", "desc", INV, "NULL argument"),
    ("scene_rebuild", "scene", INV, "NULL argument"),
    ("scene_update_appearance", "scene", INV, "NULL argument"),
    ("trace", "scene", INV, "NULL argument"), ("trace", "desc", INV, "NULL argument"),
    ("radiance", "scene", INV, "NULL argument"), ("radiance", "params", INV, "phip_radiance_device: NULL argument"), ("radiance", "desc", INV, "phip_radiance_device: NULL argument"),
    ("camera_rays", "scene", INV, "NULL argument"), ("camera_rays", "params", INV, "phip_camera_rays_device: NULL argument"),
    ("camera_rays", "desc", INV, "phip_camera_rays_device: NULL argument"),
    ("film", "scene", INV, "NULL argument"), ("film", "params", INV, "phip_film_device: NULL argument"), ("film", "desc", INV, "phip_film_device: NULL argument"),
    ("bsdf", "scene", INV, "phip_bsdf_device: NULL argument"), ("bsdf", "desc", INV, "phip_bsdf_device: NULL argument"),
    ("emitter_sample", "scene", INV, "phip_emitter_sample_device: NULL argument"), ("emitter_sample", "desc", INV, "phip_emitter_sample_device: NULL argument"),
    ("emitter_eval", "scene", INV, "phip_emitter_eval_device: NULL argument"), ("emitter_eval", "desc", INV, "phip_emitter_eval_device: NULL argument"),
]
# ... and what they say without a device once their own checks have passed: the call's name in front for the three shading parts, and for them alone
WITHOUT_A_DEVICE = [
    ("scene_update", DEV, "%s"), ("scene_rebuild", DEV, "%s"), ("scene_update_appearance", DEV, "%s"), ("trace", DEV, "%s"), ("radiance", DEV, "%s"),
    ("camera_rays", DEV, "%s"), ("film", DEV, "%s"),
    ("bsdf", DEV, "phip_bsdf_device: %s"), ("emitter_sample", DEV, "phip_emitter_sample_device: %s"), ("emitter_eval", DEV, "phip_emitter_eval_device: %s"),
]


@pytest.fixture(scope="module")
def never_read():
    """a non-NULL scene handle for the checks that come before any use of it"""
    buf = C.create_string_buffer(1 << 16)
    return C.c_void_p(C.addressof(buf)), buf


def arguments(call, first, desc):
    """(render parameters or have_scene, descriptor) as the C side takes them"""
    good_first, good_desc = GOOD[call]
    if isinstance(good_first, dict):
        first = None if first is None else C.byref(A.default_render_params(**dict(good_first, **first)))
    d = None if desc is None else C.byref(DESC[call](**dict(good_desc, **desc)))
    return first, d


@pytest.mark.parametrize("row", range(len(REFUSALS)))
def test_every_refusal_of_the_argument_checks(phip, row):
    call, first, desc, code, text = REFUSALS[row]
    first, d = arguments(call, first, desc)
    phip.phip_debug_host_film_args(None, None)                       # (another text in between: the next one is this call's)
    rc = getattr(phip, "phip_debug_host_%s_args" % call)(first, d)
    assert rc == code, (REFUSALS[row], _ffi.debug_lib().phip_last_error())
    if code:
        assert _ffi.debug_lib().phip_last_error().decode() == text


def entry_point(phip, call, scene, null=None):
    """the real entry point on arguments that pass its own checks, `null` of them NULL"""
    keep = []
    if call in GOOD:
        first, d = arguments(call, None if null == "params" else {}, None if null == "desc" else {})
        fn = getattr(phip, "phip_%s_device" % call)
        if isinstance(GOOD[call][0], dict):
            return fn(scene, first, d, None) if call != "camera_rays" else fn(scene, first, d)
        return fn(scene, d)
    if call == "trace":
        return phip.phip_trace_device(scene, None if null == "desc" else BUF, 5, BUF, None, None, None, None)
    if call == "scene_update_appearance":
        mats = (A.phip_material * 1)(); keep.append(mats)
        a = A.phip_appearance_desc(n_materials=1, materials=mats)
        return phip.phip_scene_update_appearance(scene, C.byref(a), None)
    u = A.phip_update_desc()
    return getattr(phip, "phip_" + call)(scene, None if null == "desc" else C.byref(u), None)


@pytest.mark.parametrize("row", range(len(NULL_ARGUMENTS)))
def test_the_guarded_entry_points_refuse_null(phip, never_read, row):
    call, null, code, text = NULL_ARGUMENTS[row]
    phip.phip_scene_create(None, 0)                                  # (another text in between)
    assert entry_point(phip, call, None if null == "scene" else never_read[0], null) == code
    assert phip.phip_last_error().decode() == text


def test_the_guarded_entry_points_without_a_device(phip, never_read):
    n = phip.phip_device_count()
    if n > 0:
        pytest.skip("a device is visible")
    said = NO_DEVICE if n == 0 else phip.phip_last_error().decode()   # (n < 0: what the runtime said of its own failure, under the count's name)
    assert n == 0 or (n == DEV and said.startswith("hipGetDeviceCount: "))
    for call, code, text in WITHOUT_A_DEVICE:
        phip.phip_scene_create(None, 0)
        assert entry_point(phip, call, never_read[0]) == code, call
        assert phip.phip_last_error().decode() == text % said, call


def test_nothing_to_do_needs_no_device(phip, never_read):
    """the early returns that come before the device count: an empty call touches nothing, the scene included"""
    h = never_read[0]
    p = C.byref(A.default_render_params(spp=1))
    assert phip.phip_radiance_device(h, p, C.byref(A.phip_radiance_desc(n=0)), None) == 0
    assert phip.phip_camera_rays_device(h, p, C.byref(A.phip_camera_rays_desc(d_pixels=BUF, m=0))) == 0
    assert phip.phip_scene_update_appearance(h, None, None) == 0 and phip.phip_scene_update_appearance(h, C.byref(A.phip_appearance_desc()), None) == 0
    for call in ("bsdf", "emitter_sample", "emitter_eval"):
        assert getattr(phip, "phip_%s_device" % call)(h, C.byref(DESC[call](**dict(GOOD[call][1], n=0)))) == 0


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------------------

N = 257
FILL = 1234.5


def host_buffer(n_bytes):
    """host memory at a 16-byte boundary: the alignment checks pass, the pointer's attributes do not"""
    raw = np.zeros(n_bytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n_bytes]


@pytest.mark.gpu
def test_host_pointers_other_devices_and_streams_on_the_cornell_box(phip, gauss):
    import torch
    if phip.phip_device_count() <= 0:
        pytest.fail("no HIP device visible: " + phip.phip_last_error().decode())
    from mitsuba_amd.integrator import Scene, PathHIP
    from ref_scenes import cornell
    gs = Scene(cornell(gauss, None).desc())
    integ = PathHIP(maxDepth=3)
    h, dev = gs._h, torch.device("cuda", 0)
    pixels = torch.arange(N, dtype=torch.int32, device=dev)
    rays, keys, _ = gs.camera_rays(1, pixels=pixels)
    hits, _, _, _ = gs.rayIntersectDevice(rays)
    rng = np.random.default_rng(41)
    unit = rng.normal(size=(N, 4)).astype(np.float32); unit[:, 3] = 0; unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    wo = torch.from_numpy(unit).to(dev)
    smp = torch.from_numpy(rng.random((N, 2)).astype(np.float32) * np.float32(0.999)).to(dev)
    ref = torch.from_numpy(np.concatenate([rng.uniform(100, 450, (N, 3)), np.zeros((N, 1))], 1).astype(np.float32)).to(dev)
    values = torch.from_numpy(rng.random((gs.height * gs.width, 4)).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    full = lambda *shape: torch.full(shape, FILL, dtype=torch.float32, device=dev)
    untouched = lambda *ts: all(bool((t == FILL).all()) for t in ts)
    host = host_buffer(N * 32).ctypes.data
    host_film = host_buffer(gs.height * gs.width * 16).ctypes.data
    err = lambda: phip.phip_last_error().decode()
    params = lambda device=0: C.byref(A.default_render_params(spp=1, max_depth=3, device=device))

    # a host pointer in place of one device array: refused before any launch, nothing written
    o_hits, o_surf = full(N, 4), full(N, 16)
    assert phip.phip_trace_device(h, host, N, o_hits.data_ptr(), None, o_surf.data_ptr(), None, None) == INV
    assert err() == "phip_trace_device: rays, hits, occlusion and surfaces must be device memory of the scene's device" and untouched(o_hits, o_surf)
    out = full(N, 4)
    d = A.phip_radiance_desc(d_rays=host, n=N, d_out=out.data_ptr())
    assert phip.phip_radiance_device(h, params(), C.byref(d), None) == INV
    assert err() == "phip_radiance_device: d_rays, d_out and d_stream must be device memory of the scene's device" and untouched(out)
    o_rays, o_pos = full(N, 8), full(N, 2)
    d = A.phip_camera_rays_desc(d_pixels=host, m=N, d_rays=o_rays.data_ptr(), d_positions=o_pos.data_ptr())
    assert phip.phip_camera_rays_device(h, params(), C.byref(d)) == INV
    assert err() == "phip_camera_rays_device: d_pixels, d_rays, d_keys and d_positions must be device memory of the scene's device" and untouched(o_rays, o_pos)
    o_film = full(gs.height, gs.width, 5)
    d = A.phip_film_desc(d_values=host_film, d_out=o_film.data_ptr())
    assert phip.phip_film_device(h, params(), C.byref(d), None) == INV
    assert err() == "phip_film_device: d_values and d_out must be device memory of the scene's device" and untouched(o_film)
    o_eval, o_sampled, o_wi = full(N, 4), full(N, 12), full(N, 4)
    d = A.phip_bsdf_desc(d_rays=rays.data_ptr(), d_hits=host, n=N, d_wo=wo.data_ptr(), d_samples=smp.data_ptr(), d_eval=o_eval.data_ptr(), d_sampled=o_sampled.data_ptr(),
                         d_wi_local=o_wi.data_ptr())
    assert phip.phip_bsdf_device(h, C.byref(d)) == INV
    assert err() == "phip_bsdf_device: every pointer must be device memory of the scene's device" and untouched(o_eval, o_sampled, o_wi)
    o_shadow = full(N, 8)
    d = A.phip_emitter_sample_desc(d_ref=ref.data_ptr(), d_samples=host, n=N, d_sampled=o_sampled.data_ptr(), d_shadow_rays=o_shadow.data_ptr())
    assert phip.phip_emitter_sample_device(h, C.byref(d)) == INV
    assert err() == "phip_emitter_sample_device: every pointer must be device memory of the scene's device" and untouched(o_sampled, o_shadow)
    d = A.phip_emitter_eval_desc(d_rays=host, d_hits=hits.data_ptr(), n=N, d_eval=o_eval.data_ptr())
    assert phip.phip_emitter_eval_device(h, C.byref(d)) == INV
    assert err() == "phip_emitter_eval_device: every pointer must be device memory of the scene's device" and untouched(o_eval)

    # device = 1 in the parameters, a scene of device 0
    d = A.phip_radiance_desc(d_rays=rays.data_ptr(), n=N, d_out=out.data_ptr())
    assert phip.phip_radiance_device(h, params(1), C.byref(d), None) == INV
    assert err() == "phip_radiance_device: scene was created on a different device" and untouched(out)
    d = A.phip_camera_rays_desc(d_pixels=pixels.data_ptr(), m=N, d_rays=o_rays.data_ptr(), d_positions=o_pos.data_ptr())
    assert phip.phip_camera_rays_device(h, params(1), C.byref(d)) == INV
    assert err() == "phip_camera_rays_device: scene was created on a different device" and untouched(o_rays, o_pos)
    d = A.phip_film_desc(d_values=values.data_ptr(), d_out=o_film.data_ptr())
    assert phip.phip_film_device(h, params(1), C.byref(d), None) == INV
    assert err() == "phip_film_device: scene was created on a different device" and untouched(o_film)

    # the scene's stream and a caller's: the same bits
    def everything(stream):
        out = list(gs.rayIntersectDevice(rays, closest=True, shadow=True, surfaces=True, stream=stream)[:3])
        out.append(integ.radiance(gs, rays, 2, seed=5, pairs=keys, stream=stream))
        out += [t for t in gs.camera_rays(1, pixels=pixels, keys=True, positions=True, stream=stream)]
        out.append(gs.film(values, 1, stream=stream)[0])
        out += [t for t in gs.bsdf(rays, hits, wo=wo, samples=smp, wi_local=True, stream=stream)]
        out += [t for t in gs.emitter_sample(ref, None, smp, shadow_rays=True, stream=stream)]
        out += [t for t in gs.emitter_eval(rays, hits, emitter=True, stream=stream)]
        return [t.cpu().numpy().copy() for t in out]
    ours, theirs = everything(None), everything(torch.cuda.Stream(device=dev))
    assert len(ours) == 15 and all(a.shape[0] in (N, gs.height) for a in ours)
    for i, (a, b) in enumerate(zip(ours, theirs)):
        assert a.tobytes() == b.tobytes(), i
    assert (ours[0].view(np.uint32)[:, 3] != A.PHIP_NO_HIT).sum() > 200               # the box is in front of the camera: the calls had work to do
    gs.close()

"""phip_bsdf_device, phip_emitter_sample_device and phip_emitter_eval_device on the GPU.

Arbiters:
    the kernels       their host twins (phip_debug_host_bsdf_parts / _emitter_sample / _emitter_eval: the statements of k_shading_parts.h over the creation's host
                      stages), bit for bit, at n = 1, 63, 64, 65 and 257 -- lane, wave and block tails -- on the five scenes of tests/test_shading_parts_host.py,
                      misses interleaved with hits; the twins themselves are held to the oracle there
    composition       phip_trace_device: the shadow rays of an emitter-sample call against shadow rays the test builds from (ref, d, dist)
    the capstone      phip_render(PHIP_FLAG_SAMPLE_BUFFER) of `path` at maxDepth 2 on the Cornell box: every sample rebuilt from the parts in float32 numpy, bit for bit
    a new look        a scene created with the look phip_scene_update_appearance gave the other one"""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi, scene as S
from test_gpu_parity import gpu  # noqa: F401  (the fixture)
from test_raycast_device_host import fields
from test_shading_parts_host import (SCENES, W, H, NO_HIT, ONE_BELOW, cornell, emitter_fields, sampled_fields, twin_bsdf, twin_emitter_eval, twin_emitter_sample,
                                     unit)

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
SENTINEL = 0xCDCDCDCD


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def pad4(a):
    a = np.asarray(a, np.float32)
    return np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 1), np.float32)], 1))


class Shot:
    """one scene on the device with 512 camera rays (every fifth turned round: a miss between hits, whatever the scene), their hits and surface records, random
    inputs, and what the host twins say for all of it -- computed once"""

    def __init__(self, gpu, phip, name, gauss):
        self.desc = SCENES[name](gauss).desc()
        self.gs = gpu.Scene(self.desc)
        rays, _, _ = self.gs.camera_rays(2)
        r = rays.cpu().numpy().copy()
        r[::5, 4:7] *= -1
        self.rays = dev(r)
        self.hits, _, surf, _ = self.gs.rayIntersectDevice(self.rays, surfaces=True)
        self.r, self.h = r, self.hits.cpu().numpy()
        sf = fields(u32(surf))
        self.hit = sf["prim"] != NO_HIT
        n = len(r)
        rng = np.random.default_rng(31)
        self.wo = pad4(unit(rng, n)); self.smp = np.minimum(rng.random((n, 2)).astype(np.float32), ONE_BELOW); self.smp2 = np.minimum(rng.random((n, 2)).astype(np.float32), ONE_BELOW)
        self.ref = pad4(np.where(self.hit[:, None], sf["p"], r[:, :3])); self.refn = pad4(np.where(self.hit[:, None], sf["ns"], unit(rng, n)))
        self.bsdf = {local: twin_bsdf(phip, self.desc, r, self.h, wo=self.wo, samples=self.smp, local=local) for local in (False, True)}
        self.es = {with_n: twin_emitter_sample(phip, self.desc, self.ref[:, :3], self.refn[:, :3] if with_n else None, self.smp2) for with_n in (False, True)}
        self.ee = {with_n: twin_emitter_eval(phip, self.desc, r, self.h, self.refn[:, :3] if with_n else None) for with_n in (False, True)}


@pytest.fixture(scope="module")
def shots(gpu, phip, gauss):
    out = {}
    yield lambda name: out[name] if name in out else out.setdefault(name, Shot(gpu, phip, name, gauss))
    for s in out.values():
        s.gs.close()


# ---- 1. every kernel against its host twin ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_kernels_equal_their_host_twins(shots, scene, n):
    s = shots(scene); gs = s.gs
    rays, hits = s.rays[:n].contiguous(), s.hits[:n].contiguous()
    wo, smp, smp2, ref, refn = (dev(a[:n]) for a in (s.wo, s.smp, s.smp2, s.ref, s.refn))
    if n == 257:
        assert s.hit[:n].sum() > 40 and (~s.hit[:n]).sum() > 40                                    # misses interleaved with hits: more than half a wave of each
    for local in (False, True):
        tev, tsm, twi = (a[:n] for a in s.bsdf[local])
        for want_eval, want_sample, want_wi in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1)):     # each output combination
            ev, sm, wi = gs.bsdf(rays, hits, wo=wo if want_eval else None, samples=smp if want_sample else None, local=local, wi_local=bool(want_wi))
            assert (ev is not None, sm is not None, wi is not None) == (bool(want_eval), bool(want_sample), bool(want_wi))
            if want_eval:
                assert (u32(ev) == tev).all(), (scene, n, local, int((u32(ev) != tev).any(axis=1).sum()))
            if want_sample:
                assert (u32(sm) == tsm).all(), (scene, n, local, int((u32(sm) != tsm).any(axis=1).sum()))
            if want_wi:
                assert (u32(wi) == twi).all()
    for with_n in (False, True):
        tsampled, trays = (a[:n] for a in s.es[with_n])
        sampled, srays = gs.emitter_sample(ref, refn if with_n else None, smp2, shadow_rays=True)
        assert (u32(sampled) == tsampled).all(), (scene, n, with_n)
        assert (u32(srays) == trays).all(), (scene, n, with_n)
        only, none = gs.emitter_sample(ref, refn if with_n else None, smp2)
        assert none is None and (u32(only) == tsampled).all()
        tev, tem = (a[:n] for a in s.ee[with_n])
        ev, em = gs.emitter_eval(rays, hits, refn if with_n else None, emitter=True)
        assert (u32(ev) == tev).all() and (em.cpu().numpy() == tem).all(), (scene, n, with_n)
        ev, none = gs.emitter_eval(rays, hits, refn if with_n else None)
        assert none is None and (u32(ev) == tev).all()


def test_the_scenes_exercise_what_they_are_there_for(shots):
    """the twins' answers over the 512 rays: samples from every kind of emitter, radiance met at hits and at misses, textured and two-sided leaves"""
    for scene, kinds in (("cornell", {0}), ("constant", {0, 1}), ("envmap", {0, 1})):
        s = shots(scene)
        e = emitter_fields(s.es[True][0])
        assert set(e["emitter"][e["emitter"] >= 0].tolist()) == kinds, scene
        assert (e["emitter"] == -1).any()
        ev, em = s.ee[True]
        if scene != "cornell":
            assert (em[~s.hit] == 0).all() and (ev.view(np.float32)[~s.hit, 3] > 0).any()             # the environment behind every miss
        else:
            assert (em[~s.hit] == -1).all() and (ev[~s.hit] == 0).all()
    for scene in ("mixed", "textured"):
        b = sampled_fields(shots(scene).bsdf[False][1])
        assert ((b["flags"] & A.PHIP_BSDF_SAMPLED_VALID) != 0).sum() > 200


# ---- 2. nothing else is written ------------------------------------------------------------------------------------------------------------------

def test_outputs_not_asked_for_and_refused_calls_leave_memory_alone(shots):
    import torch
    s = shots("mixed"); gs = s.gs; L = gs._L
    n = 65
    fill = lambda words: torch.full((words,), -842150451, dtype=torch.int32, device="cuda")          # 0xCDCDCDCD
    ev, sm, wi = fill(4 * (n + 3)), fill(12 * (n + 3)), fill(4 * (n + 3))
    wo, smp = dev(s.wo[:n]), dev(s.smp[:n])
    base = dict(d_rays=s.rays.data_ptr(), d_hits=s.hits.data_ptr(), n=n, d_wo=wo.data_ptr(), d_samples=smp.data_ptr())
    intact = lambda t: bool((t == -842150451).all())
    # eval alone: the other two buffers -- not passed -- and the words behind entry n stay as they were
    assert L.phip_bsdf_device(gs._h, C.byref(A.phip_bsdf_desc(d_eval=ev.data_ptr(), **base))) == 0
    assert (u32(ev)[:4 * n].reshape(n, 4) == s.bsdf[False][0][:n]).all() and intact(ev[4 * n:]) and intact(sm) and intact(wi)
    assert L.phip_bsdf_device(gs._h, C.byref(A.phip_bsdf_desc(d_sampled=sm.data_ptr(), d_wi_local=wi.data_ptr(), **base))) == 0
    assert (u32(sm)[:12 * n].reshape(n, 12) == s.bsdf[False][1][:n]).all() and intact(sm[12 * n:]) and intact(wi[4 * n:])
    # refusals: a misaligned pointer, a host pointer, an output without its input, an unknown flag, no output, too many items
    ev, sm, wi = fill(4 * (n + 3)), fill(12 * (n + 3)), fill(4 * (n + 3))
    host = np.zeros((n, 4), np.float32)
    all_out = dict(d_eval=ev.data_ptr(), d_sampled=sm.data_ptr(), d_wi_local=wi.data_ptr())
    for bad in (dict(all_out, d_eval=ev.data_ptr() + 8), dict(all_out, d_wi_local=host.ctypes.data), dict(all_out, d_wo=None), dict(all_out, d_samples=None),
                dict(all_out, flags=4), dict(d_eval=None), dict(all_out, n=2 ** 32 - 255), dict(all_out, d_hits=host.ctypes.data)):
        assert L.phip_bsdf_device(gs._h, C.byref(A.phip_bsdf_desc(**dict(base, **bad)))) == A.PHIP_ERR_INVALID, bad
        assert L.phip_last_error().startswith(b"phip_bsdf_device: ")
        assert intact(ev) and intact(sm) and intact(wi) and (host == 0).all(), bad
    es, sr, ee, em = fill(12 * (n + 3)), fill(8 * (n + 3)), fill(4 * (n + 3)), fill(n + 3)
    ref, refn, smp2 = dev(s.ref[:n]), dev(s.refn[:n]), dev(s.smp2[:n])
    sbase = dict(d_ref=ref.data_ptr(), d_ref_n=refn.data_ptr(), d_samples=smp2.data_ptr(), n=n, d_sampled=es.data_ptr())
    for bad in (dict(d_shadow_rays=sr.data_ptr() + 4), dict(d_sampled=host.ctypes.data), dict(d_samples=None), dict(d_ref=ref.data_ptr() + 8, d_shadow_rays=sr.data_ptr())):
        assert L.phip_emitter_sample_device(gs._h, C.byref(A.phip_emitter_sample_desc(**dict(sbase, **bad)))) == A.PHIP_ERR_INVALID, bad
        assert intact(es) and intact(sr)
    assert L.phip_emitter_sample_device(gs._h, C.byref(A.phip_emitter_sample_desc(**sbase))) == 0
    assert (u32(es)[:12 * n].reshape(n, 12) == s.es[True][0][:n]).all() and intact(es[12 * n:]) and intact(sr)
    ebase = dict(d_rays=s.rays.data_ptr(), d_hits=s.hits.data_ptr(), d_ref_n=refn.data_ptr(), n=n, d_eval=ee.data_ptr())
    for bad in (dict(d_emitter=em.data_ptr() + 4), dict(d_eval=host.ctypes.data), dict(d_rays=None), dict(d_emitter=em.data_ptr(), d_ref_n=host.ctypes.data)):
        assert L.phip_emitter_eval_device(gs._h, C.byref(A.phip_emitter_eval_desc(**dict(ebase, **bad)))) == A.PHIP_ERR_INVALID, bad
        assert intact(ee) and intact(em)
    assert L.phip_emitter_eval_device(gs._h, C.byref(A.phip_emitter_eval_desc(**ebase))) == 0
    assert (u32(ee)[:4 * n].reshape(n, 4) == s.ee[True][0][:n]).all() and intact(ee[4 * n:]) and intact(em)
    for fn, d in ((L.phip_bsdf_device, A.phip_bsdf_desc(n=0)), (L.phip_emitter_sample_device, A.phip_emitter_sample_desc(n=0)), (L.phip_emitter_eval_device, A.phip_emitter_eval_desc(n=0))):
        assert fn(gs._h, C.byref(d)) == 0                                                            # n == 0: PHIP_OK, nothing touched


# ---- 3. composition with the ray cast ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cornell", "mixed", "envmap"])
def test_shadow_rays_are_the_ones_the_sample_describes(shots, scene):
    s = shots(scene); gs = s.gs
    sampled, srays = gs.emitter_sample(dev(s.ref), dev(s.refn), dev(s.smp2), shadow_rays=True)
    e = emitter_fields(u32(sampled))
    have = e["emitter"] >= 0
    assert have.sum() > 50 and (~have).sum() > 20
    mine = np.zeros((len(have), 8), np.float32)
    mine[:, :3] = s.ref[:, :3]; mine[:, 3] = np.float32(1e-4); mine[:, 4:7] = e["d"]; mine[:, 7] = e["dist"] * (np.float32(1) - np.float32(1e-3))
    _, occ, _, _ = gs.rayIntersectDevice(srays, closest=False, shadow=True)
    _, want, _, _ = gs.rayIntersectDevice(dev(mine), closest=False, shadow=True)
    occ, want = occ.cpu().numpy(), want.cpu().numpy()
    assert (occ[have] == want[have]).all() and (u32(srays)[have] == mine.view(np.uint32)[have]).all()
    assert (occ[~have] == 0).all()                                                                   # no sample: the empty interval, not occluded
    assert 0 < occ[have].sum() < have.sum()                                                          # both answers occur


# ---- 4. `path` at maxDepth 2, rebuilt from the parts ---------------------------------------------------------------------------------------------------

def mi_weight(a, b):
    a = a * a; b = b * b
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / (a + b)


def test_path_at_depth_two_is_rebuilt_from_the_parts_bit_for_bit(gpu, phip, gauss):
    """MIPathTracer::Li at maxDepth 2 (path.cpp:119-300 as shadeVertex states it, k_shade.h), every statement a single float32 operation:
        L  = Le(first hit)                                                           0 + throughput (1) * Le
        L += value * bsdfVal * miWeight(emitterPdf, bsdfPdf)     if not occluded      ((1 * value) * bsdfVal) * weight: one emitter sample at the first vertex
        L += (1 * bsdfWeight) * Le(second hit) * miWeight(bsdfPdf, pdfEmitterDirect)  the BSDF-sampled ray
    the stream: block 1 of (pixel, sample, seed) -- .xy the emitter sample, .zw the BSDF sample (a smooth vertex at depth 1: k0 = 0); block 0 is the pixel jitter.
    Russian roulette starts at depth 5 and the second vertex samples nothing (depth >= maxDepth)."""
    f = np.float32
    spp, seed = 4, 0
    gs = gpu.Scene(cornell(gauss).desc())
    integ = gpu.PathHIP(maxDepth=2)
    assert integ.render(gs, gpu.HDRFilm(W, H), spp, seed=seed, flags=A.PHIP_FLAG_SAMPLE_BUFFER)
    want = integ.samples(gs, spp).reshape(W * H * spp, 4)
    rays, keys, _ = gs.camera_rays(spp, seed=seed)
    N = W * H * spp
    k = keys.cpu().numpy()
    blk = np.zeros((N, 4), f); out4 = (C.c_float * 4)()
    for i in range(N):
        phip.phip_debug_host_ctr_block(int(k[i, 0]), int(k[i, 1]), 1, seed, out4)
        blk[i] = out4[:]
    smp_e, smp_b = np.ascontiguousarray(blk[:, :2]), np.ascontiguousarray(blk[:, 2:])
    # 1. camera rays, first hits
    hits, _, surf, _ = gs.rayIntersectDevice(rays, surfaces=True)
    sf = fields(u32(surf))
    hit1 = sf["prim"] != NO_HIT
    ref, refn = dev(pad4(sf["p"])), dev(pad4(sf["ns"]))                                               # (diffuse, one-sided: refN is the shading normal)
    le1 = gs.emitter_eval(rays, hits)[0].cpu().numpy()[:, :3]
    # 2. the emitter sample with the sample's own numbers, any-hit
    es, srays = gs.emitter_sample(ref, refn, dev(smp_e), shadow_rays=True)
    _, occ, _, _ = gs.rayIntersectDevice(srays, closest=False, shadow=True)
    occ = occ.cpu().numpy() != 0
    e = emitter_fields(u32(es))
    # 3. the BSDF at the emitter's direction, the BSDF sample, its ray, what it meets
    ev, bs, _ = gs.bsdf(rays, hits, wo=dev(pad4(e["d"])), samples=dev(smp_b))
    ev = ev.cpu().numpy(); b = sampled_fields(u32(bs))
    valid = hit1 & ((b["flags"] & A.PHIP_BSDF_SAMPLED_VALID) != 0)
    nxt = np.zeros((N, 8), f)
    nxt[:, :3] = sf["p"]; nxt[:, 3] = f(1e-4); nxt[:, 4:7] = b["wo"]; nxt[:, 7] = np.inf
    nxt[~valid] = (0, 0, 0, 0, 0, 0, 1, -1)                                                          # no ray: an empty interval
    nxt = dev(nxt)
    hits2, _, _, _ = gs.rayIntersectDevice(nxt)
    ev2, em2 = gs.emitter_eval(nxt, hits2, refn, emitter=True)
    ev2, em2 = ev2.cpu().numpy(), em2.cpu().numpy()
    # 4. path.cpp's statements in shadeVertex's operation order
    L = np.zeros((N, 4), f)
    L[hit1, 3] = 1
    L[hit1, :3] = (f(0) + f(1) * le1)[hit1]
    bsdf_val, b_pdf = ev[:, :3], ev[:, 3]
    nee = hit1 & (e["pdf"] != 0) & (e["value"] != 0).any(axis=1) & (bsdf_val != 0).any(axis=1)
    sh_c = ((f(1) * e["value"]) * bsdf_val) * mi_weight(e["pdf"], b_pdf)[:, None]
    add = nee & ~occ
    L[add, :3] = L[add, :3] + sh_c[add]
    met = valid & (em2 >= 0)
    thr = f(1) * b["weight"]
    c2 = (thr * ev2[:, :3]) * mi_weight(b["pdf"], ev2[:, 3])[:, None]
    L[met, :3] = L[met, :3] + c2[met]
    print("first hits %d of %d, emitted %d, next-event %d (occluded %d), emitter met by the BSDF ray %d" % (hit1.sum(), N, (le1 != 0).any(axis=1).sum(), add.sum(), (nee & occ).sum(), met.sum()))
    assert hit1.sum() > N // 2 and add.sum() > 100 and (nee & occ).sum() > 10 and met.sum() > 5 and (le1 != 0).any()      # every term is exercised
    diff = (L.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert not diff.any(), "%d of %d samples differ, first: %s vs %s" % (diff.sum(), N, L[diff][:1], want[diff][:1])
    assert (L[:, 3] == want[:, 3]).all()                                                             # alpha: 1 at a first hit, 0 at a miss
    gs.close()


# ---- 5. after phip_scene_update_appearance ------------------------------------------------------------------------------------------------------------------

def test_the_parts_answer_for_the_new_look(gpu, gauss):
    sb = cornell(gauss)
    gs = gpu.Scene(sb.desc())
    rays, _, _ = gs.camera_rays(1)
    n = rays.shape[0]
    rng = np.random.default_rng(33)
    wo, smp, smp2 = dev(pad4(unit(rng, n))), dev(np.minimum(rng.random((n, 2)).astype(np.float32), ONE_BELOW)), dev(np.minimum(rng.random((n, 2)).astype(np.float32), ONE_BELOW))

    def answers(scene):
        hits, _, surf, _ = scene.rayIntersectDevice(rays, surfaces=True)
        sf = fields(u32(surf))
        ref, refn = dev(pad4(sf["p"])), dev(pad4(sf["ns"]))
        ev, sm, _ = scene.bsdf(rays, hits, wo=wo, samples=smp)
        es, _ = scene.emitter_sample(ref, refn, smp2)
        ee, _ = scene.emitter_eval(rays, hits)
        return [u32(t) for t in (ev, sm, es, ee)]

    before = answers(gs)
    wall = sb.materials[0]; wall.type = A.PHIP_BSDF_ROUGHCONDUCTOR                                    # the white of floor, ceiling, back wall and blocks turns to copper
    wall.eta[:] = list(S.CU_ETA); wall.k[:] = list(S.CU_K); wall.alpha_u = wall.alpha_v = 0.2; wall.reflectance[:] = [1, 1, 1]; wall.sample_visible = 1
    sb.emitters[0]["radiance"] = [3.0, 20.0, 5.0]
    d = sb.desc()
    info = gs.update_appearance(materials=list(sb.materials), emitters=[d.emitters[i] for i in range(d.n_emitters)])
    assert info["material_mask_changed"] == 1
    after = answers(gs)
    fresh = gpu.Scene(sb.desc())
    want = answers(fresh)
    for name, a, b, w in zip(("eval", "sampled", "emitter sample", "emitter eval"), after, before, want):
        assert (a == w).all(), name
        assert (a != b).any(), name                                                                   # ... and it is another answer than before
    gs.close(); fresh.close()


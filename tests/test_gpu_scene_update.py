"""phip_scene_update on the GPU: create(A) -> update(B) must be create(B), bit for bit -- sample buffers and films as uint32, and the counters samples, closest_rays,
shadow_rays, path_vertices, invalid_samples -- on every device path the scene admits (default, PHIP_FLAG_NO_MEGA, PHIP_FLAG_NO_FUSED, PHIP_FLAG_FUSED_ANY), and the
oracle's render of B.  Node-visit and triangle-test counters are not compared: the refitted boxes are conservative, not the builder's.  Films are 48 x 48 to 64 x 64
(and compare_render's ragged 100 x 70 once) at 4 spp."""
import ctypes as C

import numpy as np
import pytest

from mitsuba_amd import _abi as A, scene as S
from test_gpu_parity import gpu, random_rays, soup  # noqa: F401  (the fixture)
from test_gpu_shade_trace_wide import sphere_box

pytestmark = pytest.mark.gpu

PATHS = (0, A.PHIP_FLAG_NO_MEGA, A.PHIP_FLAG_NO_FUSED, A.PHIP_FLAG_FUSED_ANY)
COUNTERS = ("samples", "closest_rays", "shadow_rays", "path_vertices", "invalid_samples")


def render(gpu, gs, integ, spp, flags=0, **kw):
    film = gpu.HDRFilm(gs.width, gs.height)
    assert integ.render(gs, film, spp, flags=A.PHIP_FLAG_SAMPLE_BUFFER | flags, **kw)
    return film.storage.copy(), integ.samples(gs, spp).copy(), tuple(int(getattr(integ.stats, c)) for c in COUNTERS)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def assert_same_renders(gpu, a, b, integ, spp, paths=PATHS, **kw):
    first = None
    for flags in paths:
        fa, sa, ca = render(gpu, a, integ, spp, flags, **kw)
        fb, sb_, cb = render(gpu, b, integ, spp, flags, **kw)
        assert same_bits(sa, sb_), "samples differ under flags %d: %.6f identical" % (flags, (sa.view(np.uint32) == sb_.view(np.uint32)).all(axis=-1).mean())
        assert same_bits(fa, fb), "films differ under flags %d" % flags
        assert ca == cb, (flags, ca, cb)
        first = first or (fa, sa, ca)
    return first


def assert_oracle(oracle, desc, gs, integ, spp, smp, **kw):
    """the samples against the oracle on the same descriptor, as compare_render holds them: bit for bit against the sweep over all triangles where that is in reach
    (<= 512 triangles); on bigger scenes against the kd-tree, the few samples that differ re-evaluated one by one against the sweep"""
    osc = oracle.OracleScene(desc)
    p = integ.params(gs, spp, **kw)
    if desc.n_triangles <= 512:
        osc.set_bruteforce(True)
    _, osmp, ost = osc.render(p, want_samples=True)
    same = (smp.view(np.uint32) == osmp.view(np.uint32)).all(axis=-1)
    if desc.n_triangles > 512 and not same.all():
        idx = np.argwhere(~same)
        assert len(idx) <= 400 and same.mean() >= 0.9999, same.mean()
        osc.set_bruteforce(True)
        for y, x, k in idx:
            assert (osc.path_sample(p, int(x), int(y), int(k)).view(np.uint32) == smp[y, x, k].view(np.uint32)).all(), (x, y, k)
    else:
        assert same.all(), same.mean()
    assert int(ost.samples) == smp.shape[0] * smp.shape[1] * smp.shape[2]
    osc.close()


def check_update(gpu, oracle, sb, mutate, spp=4, cls=None, paths=PATHS, with_oracle=True, **ikw):
    """create(A) -> update(B) against create(B) and the oracle on B; returns (updated scene, fresh scene, descriptor of B, update info)"""
    gs = gpu.Scene(sb.desc())
    before = gs.accel_info()
    mutate(sb)
    info = gs.update(positions=sb.flat_positions(), normals=sb.flat_normals(), camera=sb.camera)
    desc_b = sb.desc()
    fresh = gpu.Scene(desc_b)
    after, want = gs.accel_info(), fresh.accel_info()
    for f in ("n_nodes", "n_leaves", "n_triangle_refs", "max_depth", "fits_lds", "fused_traversal"):
        assert getattr(after, f) == getattr(before, f), f                    # the topology and the device paths are the creation's
    assert (after.fits_lds, after.fused_traversal) == (want.fits_lds, want.fused_traversal)
    assert after.sah_cost == info.sah_cost and info.sah_cost > 1.0 and info.kernel_ms > 0 and info.update_ms >= info.kernel_ms * 0.5
    integ = (cls or gpu.PathHIP)(**(ikw or dict(maxDepth=6)))
    film, smp, counters = assert_same_renders(gpu, gs, fresh, integ, spp, paths)
    assert np.isfinite(film).all() and counters[0] == gs.width * gs.height * spp
    if with_oracle:
        assert_oracle(oracle, desc_b, gs, integ, spp, smp)
    return gs, fresh, desc_b, info


def move_shapes(sb, ids, offset=(0, 0, 0), rotate_y_deg=0.0, scale=(1, 1, 1)):
    """rotates the meshes `ids` about the vertical axis through their common centre, scales them about it, then translates them; normals follow the rotation and the
    inverse scale"""
    P = np.concatenate([sb.positions[i] for i in ids]).astype(np.float64)
    c = 0.5 * (P.min(axis=0) + P.max(axis=0))
    a = np.radians(rotate_y_deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    s = np.asarray(scale, np.float64)
    for i in ids:
        sb.positions[i] = (((sb.positions[i].astype(np.float64) - c) * s) @ R.T + c + np.asarray(offset, np.float64)).astype(np.float32)
        if sb.normals[i] is not None:
            n = (sb.normals[i].astype(np.float64) / s) @ R.T
            sb.normals[i] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


TALL, SHORT, LIGHT = range(11, 16), range(6, 11), [5]
EXTENT = 559.2


def test_cornell_block_rotates_and_camera_moves(gpu, oracle, gauss):
    """32 triangles: the packed leaf table, k_mega"""
    def mutate(sb):
        move_shapes(sb, TALL, offset=(-40.0, 0.0, -60.0), rotate_y_deg=25.0)
        sb.perspective(origin=(150.0, 330.0, -700.0), target=(278.0, 250.0, 0.0), up=(0, 1, 0), fov_x_deg=42.0, near=10.0, far=2800.0)
    gs, fresh, _, info = check_update(gpu, oracle, S.cornell_box(48, 48, gauss), mutate)
    assert gs.accel_info().fits_lds == 1 and info.n_degenerate == 0


def test_cornell_camera_alone_moves_400_extents_away(gpu, oracle, gauss):
    def mutate(sb):
        sb.perspective(origin=(278.0, 273.0, -400.0 * EXTENT), target=(278.0, 273.0, 0.0), up=(0, 1, 0), fov_x_deg=0.14, near=10.0, far=1e6)
    sb = S.cornell_box(48, 48, gauss)
    gs = gpu.Scene(sb.desc())
    mutate(sb)
    info = gs.update(camera=sb.camera)                                  # no positions: the triangle pass is skipped, the refit runs (the pad changed)
    desc_b = sb.desc(); fresh = gpu.Scene(desc_b)
    integ = gpu.PathHIP(maxDepth=6)
    film, smp, _ = assert_same_renders(gpu, gs, fresh, integ, 4)
    assert film[..., :3].max() > 0
    assert_oracle(oracle, desc_b, gs, integ, 4, smp)


def test_cornell_light_moves(gpu, oracle, gauss):
    """the area CDF, 1 / area and the emitter records in the LDS emitter table"""
    def mutate(sb):
        move_shapes(sb, LIGHT, offset=(60.0, -120.0, 40.0), rotate_y_deg=30.0, scale=(1.5, 1.0, 0.6))
    check_update(gpu, oracle, S.cornell_box(64, 64, gauss), mutate)


def test_cornell_mixed_blocks_move(gpu, oracle, gauss):
    """copper and glass: the mailbox build of k_mega, k_shade_trace under PHIP_FLAG_NO_MEGA"""
    def mutate(sb):
        move_shapes(sb, SHORT, offset=(30.0, 0.0, 20.0), rotate_y_deg=-20.0)
        move_shapes(sb, TALL, offset=(-20.0, 0.0, -30.0), scale=(1.0, 0.8, 1.0))
    check_update(gpu, oracle, S.cornell_mixed(48, 48, gauss), mutate)


@pytest.mark.parametrize("integrator", ["path", "direct", "volpath_simple"])
def test_cornell_spheres_sphere_translated_and_squashed(gpu, oracle, gauss, integrator):
    """1088 triangles with vertex normals: k_mega on the 8-wide tree"""
    def mutate(sb):
        move_shapes(sb, [16], offset=(40.0, 60.0, -30.0), scale=(1.0, 0.6, 1.2))
    cls = {"path": gpu.PathHIP, "direct": gpu.DirectHIP, "volpath_simple": gpu.VolPathSimpleHIP}[integrator]
    ikw = dict(shadingSamples=2) if integrator == "direct" else dict(maxDepth=6)
    gs, _, _, _ = check_update(gpu, oracle, S.cornell_spheres(48, 48, gauss), mutate, cls=cls, with_oracle=integrator == "path", **ikw)
    assert gs.accel_info().fused_traversal >= 4


@pytest.mark.parametrize("kind,size,res", [("constant", None, (48, 48)), ("albedo", (6, 4), (100, 70)), ("envmap", (24, 12), (48, 48))])
def test_textures_and_environment_emitters(gpu, oracle, gauss, kind, size, res):
    """k_shade_trace on the small scene (the Cornell box under a `constant` emitter), k_shade_trace_w under PHIP_FLAG_FUSED_ANY on the sphere boxes: UV tangents and the
    environment sphere are recomputed; the camera leaves the scene box"""
    if size is None:
        sb = S.SceneBuilder(); sb.constant((0.5, 0.6, 0.8), sampling_weight=0.7); S.cornell_box(res[0], res[1], gauss, sb=sb)
        moved = TALL
    else:
        sb = sphere_box(gauss, kind, size[0], size[1], w=res[0], h=res[1])
        moved = [len(sb.positions) - 1]

    def mutate(sb):
        move_shapes(sb, moved, offset=(-30.0, 40.0, 20.0), rotate_y_deg=35.0, scale=(1.1, 0.7, 1.0))
        sb.perspective(origin=(900.0, 700.0, -1500.0), target=(278.0, 250.0, 280.0), up=(0, 1, 0), fov_x_deg=30.0, near=10.0, far=6000.0)
    check_update(gpu, oracle, sb, mutate)


def soup_scene(gauss, P, T):
    sb = S.SceneBuilder()
    sb.constant((0.8, 0.8, 0.8))
    sb.mesh(P, T, sb.diffuse((0.5, 0.5, 0.5)))
    sb.perspective((0, 0, -30), (0, 0, 0), (0, 1, 0), 40.0)
    sb.hdrfilm(48, 48, gauss)
    return sb


def test_triangle_soup_with_spatial_splits(gpu, oracle, gauss):
    """6000 triangles: split references (several records per triangle), the wavefront kernels; phip_trace after the update"""
    rng = np.random.default_rng(17)
    P, T = soup(rng, 6000, size=0.3, extent=8.0)

    def mutate(sb):
        p = sb.positions[0]
        sb.positions[0] = (p + 1.6 * np.sin(p[:, [1, 2, 0]] * (np.pi / 8.0) + np.array([0.3, 1.1, 2.0]))).astype(np.float32)
    gs, fresh, desc_b, _ = check_update(gpu, oracle, soup_scene(gauss, P, T), mutate, spp=4, maxDepth=4)
    assert gs.accel_info().n_triangle_refs > 6000
    rays = random_rays(rng, 50000, -9, 9, mint=0.0)
    gh, go, _ = gs.rayIntersect(rays, True, True)
    fh, fo, _ = fresh.rayIntersect(rays, True, True)
    assert same_bits(gh, fh) and (go == fo).all()
    osc = oracle.OracleScene(desc_b)
    bh, _, _ = osc.trace(rays[:5000], True, False, bruteforce=True)
    assert same_bits(gh[:5000], bh)
    oh, oo, _ = osc.trace(rays, True, True)
    assert (gh.view(np.uint32) == oh.view(np.uint32)).all(axis=1).mean() > 0.9999 and (go == oo).mean() > 0.9999
    osc.close()


def test_torch_tensor_on_the_device_and_a_chain_back(gpu, gauss):
    import torch
    sb = S.cornell_spheres(48, 48, gauss)
    desc_a = sb.desc()
    Pa, Na = sb.flat_positions(), sb.flat_normals()
    untouched, host, dev = gpu.Scene(desc_a), gpu.Scene(desc_a), gpu.Scene(desc_a)
    move_shapes(sb, [16], offset=(40.0, 60.0, -30.0), scale=(1.0, 0.6, 1.2))
    Pb, Nb = sb.flat_positions(), sb.flat_normals()
    host.update(positions=Pb, normals=Nb)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tp = torch.from_numpy(Pa).cuda() + torch.from_numpy(Pb - Pa).cuda()      # produced on the caller's stream
        tn = torch.from_numpy(Nb).cuda()
    tp_host = tp.cpu().numpy()
    info = dev.update(positions=tp, normals=tn, stream=stream)
    assert info.kernel_ms > 0
    if not same_bits(tp_host, Pb):                                             # (Pa + (Pb - Pa) may round: compare with what the tensor holds)
        host.update(positions=tp_host, normals=Nb)
    integ = gpu.PathHIP(maxDepth=6)
    assert_same_renders(gpu, dev, host, integ, 4)
    with pytest.raises(ValueError):
        dev.update(positions=tp.double())
    with pytest.raises(ValueError):
        dev.update(positions=tp[:-1])
    # A -> B -> A: the untouched creation, bit for bit
    dev.update(positions=torch.from_numpy(Pa).cuda(), normals=torch.from_numpy(Na).cuda())
    assert_same_renders(gpu, dev, untouched, integ, 4)


def test_errors_leave_the_scene_unchanged(gpu, gauss):
    sb = S.cornell_box(48, 48, gauss)
    # one triangle of the short block is degenerate when the scene is created
    good = sb.positions[7].copy()
    sb.positions[7][1] = sb.positions[7][0]                                   # (vertex 1 belongs to the first triangle of the quad only)
    gs = gpu.Scene(sb.desc())
    integ = gpu.PathHIP(maxDepth=6)
    before = render(gpu, gs, integ, 4)
    P = sb.flat_positions()
    bad = P.copy(); bad[40, 1] = np.nan
    grown = P.copy(); first = sum(len(p) for p in sb.positions[:7]); grown[first:first + 4] = good
    for kw, code in ((dict(positions=bad), A.PHIP_ERR_INVALID), (dict(normals=np.zeros_like(P)), A.PHIP_ERR_INVALID), (dict(positions=grown), A.PHIP_ERR_UNSUPPORTED)):
        with pytest.raises(Exception) as e:
            gs.update(**kw)
        assert getattr(e.value, "code", None) == code, (kw.keys(), e.value)
        after = render(gpu, gs, integ, 4)
        assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2] == after[2]
    assert "1 triangles" in str(e.value)
    # the light collapsed to a line: an area emitter without area is refused as at creation
    flat = P.copy(); lf = sum(len(p) for p in sb.positions[:5]); flat[lf:lf + 4] = flat[lf]
    with pytest.raises(Exception) as e:
        gs.update(positions=flat)
    assert e.value.code == A.PHIP_ERR_INVALID
    assert same_bits(before[1], render(gpu, gs, integ, 4)[1])
    # a triangle that collapses is served, and comes back
    victim = P.copy(); v0 = sum(len(p) for p in sb.positions[:12]); victim[v0 + 2] = victim[v0]
    assert gs.update(positions=victim).n_degenerate == 2                       # (the one of the creation never had a record: not counted; both triangles of the quad share the vertex)
    assert gs.update(positions=P).n_degenerate == 0
    assert same_bits(before[1], render(gpu, gs, integ, 4)[1])


def test_multi_device_replicas_are_refreshed(gpu, gauss):
    sb = S.cornell_spheres(48, 48, gauss)
    gs = gpu.Scene(sb.desc())
    integ = gpu.PathHIP(maxDepth=6)
    kw = dict(flags=A.PHIP_FLAG_ALIAS_DEVICES, devices=[0, 0])
    stale = gpu.HDRFilm(48, 48); assert integ.render(gs, stale, 4, **kw)          # the replica exists, of A
    move_shapes(sb, [17], offset=(-50.0, -80.0, 30.0), scale=(0.7, 1.2, 1.0))
    gs.update(positions=sb.flat_positions(), normals=sb.flat_normals())
    fresh = gpu.Scene(sb.desc())
    a, b = gpu.HDRFilm(48, 48), gpu.HDRFilm(48, 48)
    assert integ.render(gs, a, 4, **kw) and integ.render(fresh, b, 4, **kw)
    assert same_bits(a.storage, b.storage) and not same_bits(a.storage, stale.storage)


def test_update_of_the_atrium_is_cheaper_than_its_build(gpu, gauss):
    """251 k triangles: a refit that is not cheaper than the build is not the feature (expected: two orders of magnitude)"""
    sb = S.atrium(64, 64, gauss, detail=1.0)
    gs = gpu.Scene(sb.desc())
    build_ms = gs.accel_info().build_ms
    rng = np.random.default_rng(3)
    for i in rng.choice(len(sb.positions), len(sb.positions) // 3, replace=False):
        if sb.shapes[i]["emitter"] < 0:
            sb.positions[i] = (sb.positions[i] + rng.uniform(-0.05, 0.05, 3)).astype(np.float32)
    info = gs.update(positions=sb.flat_positions(), normals=sb.flat_normals())
    print("atrium: build_ms %.1f update_ms %.2f kernel_ms %.3f sah %.2f -> %.2f" % (build_ms, info.update_ms, info.kernel_ms, gs.accel_info().sah_cost, info.sah_cost))
    assert info.update_ms < build_ms, (info.update_ms, build_ms)
    fresh = gpu.Scene(sb.desc())
    integ = gpu.PathHIP(maxDepth=6)
    assert_same_renders(gpu, gs, fresh, integ, 1, paths=(0,))

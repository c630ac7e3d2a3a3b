"""phip_scene_update_appearance on the GPU: create(X) -> update_appearance(Y) must be create(Y), bit for bit -- sample buffers and films as uint32 and the counters
samples, closest_rays, shadow_rays, path_vertices, invalid_samples -- for `path`, `volpath_simple` and, where the scene admits it, `direct`, on the device paths the
scene admits.  The arbiter is phip_scene_create on the new descriptor, which the other suites pin to the oracle.  Films are 32 x 32 at most, 4 spp."""
import numpy as np
import pytest

from mitsuba_amd import _abi as A, _ffi, scene as S
from ref_scenes import _sky, half
from test_gpu_parity import gpu, soup  # noqa: F401  (the fixture)
from test_gpu_scene_update import assert_same_renders, render, same_bits
from test_gpu_shade_trace_wide import sphere_box

pytestmark = pytest.mark.gpu

SMALL_PATHS = (0, A.PHIP_FLAG_NO_MEGA, A.PHIP_FLAG_NO_FUSED)
WIDE_PATHS = (A.PHIP_FLAG_FUSED_ANY, A.PHIP_FLAG_NO_FUSED)


def materials_of(sb):
    return list(sb.materials)


def emitters_of(d):
    return [d.emitters[i] for i in range(d.n_emitters)]


def integrators(gpu, direct=True):
    out = [gpu.PathHIP(maxDepth=5), gpu.VolPathSimpleHIP(maxDepth=5)]
    return out + ([gpu.DirectHIP()] if direct else [])


def assert_is_fresh(gpu, gs, sb, paths, direct=True, **kw):
    """the updated scene against a creation from the builder's current state"""
    fresh = gpu.Scene(sb.desc())
    a, b = gs.accel_info(), fresh.accel_info()
    assert (a.fits_lds, a.fused_traversal, a.n_nodes, a.n_triangle_refs) == (b.fits_lds, b.fused_traversal, b.n_nodes, b.n_triangle_refs)
    for integ in integrators(gpu, direct):
        film, smp, counters = assert_same_renders(gpu, gs, fresh, integ, 4, paths, **kw)
        assert np.isfinite(film).all() and counters[0] == gs.width * gs.height * 4
    return fresh


def two_light_box(gauss, w=32, h=32):
    sb = S.cornell_box(w, h, gauss, short_bsdf=lambda b: b.diffuse((0.7, 0.7, 0.7)), tall_bsdf=lambda b: b.diffuse((0.6, 0.6, 0.7)))      # materials 4 and 5: the blocks' own
    sb.quad((100, 1, 100), (160, 1, 100), (160, 1, 160), (100, 1, 160), sb.diffuse((0.0, 0.0, 0.0)), facing=(0, 1, 0), radiance=(4.0, 6.0, 9.0))
    return sb


def test_cornell_reflectances_a_black_wall_and_the_lights(gpu, gauss):
    """32 + 2 triangles: the packed leaf table, k_mega; a reflectance of 0 takes TS_MF_SMOOTH out of the wall's records"""
    sb = two_light_box(gauss)
    gs = gpu.Scene(sb.desc())
    before = gs.accel_info().as_dict()
    sb.materials[0].reflectance[:] = [0.2, 0.7, 0.3]
    sb.materials[1].reflectance[:] = [0.0, 0.0, 0.0]
    sb.emitters[0]["radiance"] = [30.0, 20.0, 5.0]; sb.emitters[0]["weight"] = 0.3
    sb.emitters[1]["weight"] = 2.0
    d = sb.desc()
    info = gs.update_appearance(materials=materials_of(sb), emitters=emitters_of(d))
    assert info["material_mask_changed"] == 0 and info["kernel_ms"] > 0 and info["update_ms"] > 0
    assert gs.accel_info().as_dict() == before and before["fits_lds"] == 1
    assert_is_fresh(gpu, gs, sb, SMALL_PATHS)
    again = gs.update_appearance(materials=materials_of(sb), emitters=emitters_of(d))              # a second identical call changes nothing
    assert again["material_mask_changed"] == 0
    assert_is_fresh(gpu, gs, sb, (0,), direct=False)


def test_cornell_types_change_and_come_back(gpu, gauss):
    sb = two_light_box(gauss)
    gs = gpu.Scene(sb.desc())
    before = gs.accel_info().as_dict()
    original = [A.phip_material.from_buffer_copy(m) for m in sb.materials]
    wall = sb.materials[1]; wall.type = A.PHIP_BSDF_ROUGHCONDUCTOR
    wall.eta[:] = list(S.CU_ETA); wall.k[:] = list(S.CU_K); wall.alpha_u = wall.alpha_v = 0.2; wall.reflectance[:] = [1, 1, 1]; wall.sample_visible = 1
    block = sb.materials[5]; block.type = A.PHIP_BSDF_DIELECTRIC; block.eta[0] = 1.5; block.reflectance[:] = [1, 1, 1]; block.transmittance[:] = [1, 1, 1]
    info = gs.update_appearance(materials=materials_of(sb))
    assert info["material_mask_changed"] == 1
    assert gs.accel_info().as_dict() == before
    fresh = assert_is_fresh(gpu, gs, sb, SMALL_PATHS)
    integ = gpu.PathHIP(maxDepth=5)
    render(gpu, gs, integ, 4); fused = integ.stats.fused
    render(gpu, fresh, integ, 4); assert fused == integ.stats.fused == 1
    sb.materials[:] = original
    assert gs.update_appearance(materials=materials_of(sb))["material_mask_changed"] == 1
    assert_is_fresh(gpu, gs, sb, SMALL_PATHS)


def test_twosided_adapter_swaps_what_it_nests(gpu, gauss):
    sb = S.cornell_box(32, 32, gauss)
    front, back = sb.diffuse((0.8, 0.2, 0.2)), sb.roughconductor(S.CU_ETA, S.CU_K, alpha=0.2)
    two = sb.twosided(front, back)
    sb.quad((200, 100, 250), (400, 100, 250), (400, 300, 350), (200, 300, 350), two)
    gs = gpu.Scene(sb.desc())
    sb.materials[two].nested[0], sb.materials[two].nested[1] = back, front
    assert gs.update_appearance(materials=materials_of(sb))["material_mask_changed"] == 0
    assert_is_fresh(gpu, gs, sb, SMALL_PATHS, direct=False)


def test_sphere_box_on_the_wide_tree_with_surfaces_and_radiance(gpu, gauss):
    """1 k triangles: the 8-wide tree, fused_traversal 4 / 5; phip_trace_device's material ids and phip_radiance_device's plan after the update"""
    import torch
    sb = sphere_box(gauss, "plain", 24, 12, 32, 32)
    gs = gpu.Scene(sb.desc())
    assert gs.accel_info().fused_traversal in (4, 5)
    integ = gpu.PathHIP(maxDepth=5)
    rays, _, _ = gs.camera_rays(1)
    integ.radiance(gs, rays, 2)                                                       # resolves the scene's RadiancePlan for the materials as created
    glass = next(i for i, m in enumerate(sb.materials) if m.type == A.PHIP_BSDF_DIELECTRIC)
    m = sb.materials[glass]; m.type = A.PHIP_BSDF_DIFFUSE; m.reflectance[:] = [0.3, 0.5, 0.7]
    info = gs.update_appearance(materials=materials_of(sb))
    assert info["material_mask_changed"] == 1
    fresh = assert_is_fresh(gpu, gs, sb, WIDE_PATHS, direct=False)
    _, _, sa, _ = gs.rayIntersectDevice(rays, surfaces=True)
    _, _, sf, _ = fresh.rayIntersectDevice(rays, surfaces=True)
    assert torch.equal(sa.view(torch.int32), sf.view(torch.int32))                    # phip_surface.material among them
    ra = integ.radiance(gs, rays, 2)
    rf = integ.radiance(fresh, rays, 2)
    assert torch.equal(ra.view(torch.int32), rf.view(torch.int32))                    # a stale RadiancePlan would shade with the creation's kernels


def soup_builder(gauss, P, T):
    sb = S.SceneBuilder()
    sb.constant((0.8, 0.8, 0.8))
    half_t = len(T) // 2
    sb.mesh(P, T[:half_t], sb.diffuse((0.5, 0.5, 0.5)))
    sb.mesh(P, T[half_t:], sb.twosided(sb.diffuse((0.3, 0.6, 0.3))))
    sb.perspective((0, 0, -30), (0, 0, 0), (0, 1, 0), 40.0)
    sb.hdrfilm(32, 32, gauss)
    return sb


@pytest.mark.parametrize("entry", ["rebuild", "update"])
def test_split_soup_classes_survive_rebuild_and_refit(gpu, gauss, entry):
    """4096 triangles: the builder's spatial splits give triangles several Wald records; every class changes, then the vertices move"""
    rng = np.random.default_rng(17)
    P, T = soup(rng, 4096, size=0.3, extent=8.0)
    sb = soup_builder(gauss, P, T)
    gs = gpu.Scene(sb.desc())
    assert gs.accel_info().n_triangle_refs > 4096
    m = sb.materials[0]; m.type = A.PHIP_BSDF_DIELECTRIC; m.eta[0] = 1.4; m.reflectance[:] = [1, 1, 1]; m.transmittance[:] = [1, 1, 1]
    m = sb.materials[1]; m.type = A.PHIP_BSDF_ROUGHCONDUCTOR; m.eta[:] = list(S.CU_ETA); m.k[:] = list(S.CU_K); m.alpha_u = m.alpha_v = 0.3; m.reflectance[:] = [1, 1, 1]; m.sample_visible = 1
    assert gs.update_appearance(materials=materials_of(sb))["material_mask_changed"] == 1
    assert_is_fresh(gpu, gs, sb, (A.PHIP_FLAG_NO_FUSED,), direct=False)
    for i in (0, 1):
        p = sb.positions[i]
        sb.positions[i] = (p + (0.05 if entry == "update" else 1.2) * np.sin(p[:, [1, 2, 0]] * (np.pi / 8.0) + np.array([0.3, 1.1, 2.0]))).astype(np.float32)
    getattr(gs, entry)(positions=sb.flat_positions())
    fresh = gpu.Scene(sb.desc())
    integ = gpu.PathHIP(maxDepth=5)
    assert_same_renders(gpu, gs, fresh, integ, 4, (A.PHIP_FLAG_NO_FUSED,))


def textured_box(gauss, size, seed=11):
    """the albedo sphere box with a texture of `size` on a diffuse reflectance and one on a copper roughness"""
    rng = np.random.default_rng(seed)
    h, w = size
    sb = S.SceneBuilder()
    S.cornell_box(32, 32, gauss, sb=sb)
    t_alb = sb.bitmap(half(rng.uniform(0.05, 0.95, (h, w, 3))), filter_type="ewa", uscale=2.0)
    t_rough = sb.bitmap(half(rng.uniform(0.05, 0.6, (h, w, 3))), filter_type="trilinear", wrap="mirror")
    m0, m1 = sb.diffuse(texture=t_alb), sb.twosided(sb.roughconductor(S.CU_ETA, S.CU_K, alpha=0.15, alpha_texture=t_rough))
    from ref_scenes import _sphere_uvs
    for centre, radius, m in (((185, 120, 170), 70.0, m0), ((370, 330, 350), 60.0, m1)):
        P, T, N = S.sphere_mesh(centre, radius, 6, 4)
        sb.mesh(P, T, m, normals=N, uvs=_sphere_uvs(N))
    return sb


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (64, 64)])
def test_textures_from_numpy_and_from_torch(gpu, gauss, size):
    import torch
    sb = textured_box(gauss, size)
    new = textured_box(gauss, size, seed=12)
    new.textures[0]["scale"] = (3.0, 1.5); new.textures[0]["wrap_u"] = A.PHIP_WRAP_CLAMP
    fresh = gpu.Scene(new.desc())
    integ = gpu.PathHIP(maxDepth=5)
    want = render(gpu, fresh, integ, 4, A.PHIP_FLAG_NO_FUSED)
    for kind in ("numpy", "torch"):
        gs = gpu.Scene(sb.desc())
        texs = [dict(t) for t in new.textures]
        if kind == "torch":
            for t in texs:
                t["levels"] = [torch.from_numpy(l).cuda() for l in t["levels"]]
        gs.update_appearance(textures=texs)
        got = render(gpu, gs, integ, 4, A.PHIP_FLAG_NO_FUSED)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], kind
        if kind == "numpy":
            assert_is_fresh(gpu, gs, new, (0, A.PHIP_FLAG_FUSED_ANY), direct=False)
            hot = [dict(texs[0]), None]                                               # (None: the roughness texture stays)
            hot[0]["levels"] = [l.copy() for l in texs[0]["levels"]]
            hot[0]["levels"][0][0, 0, 1] = 1.5
            with pytest.raises(_ffi.PhipError) as e:
                gs.update_appearance(textures=hot)
            assert e.value.code == A.PHIP_ERR_INVALID and "diffuse reflectance > 1" in str(e.value)
            after = render(gpu, gs, integ, 4, A.PHIP_FLAG_NO_FUSED)                   # the refusal left the scene as it was
            assert same_bits(after[0], want[0]) and same_bits(after[1], want[1])


def env_scene(gauss, size, seed, scale=0.6, to_world=None, constant=None):
    rng = np.random.default_rng(seed)
    h, w = size
    sb = S.SceneBuilder()
    sb.envmap(half(_sky(w, h) * rng.uniform(0.5, 1.5, (h, w, 1))), scale=scale, to_world=to_world, pyramid=True)
    S.cornell_box(32, 32, gauss, sb=sb)
    sb.perspective(origin=(278.0, 273.0, -300.0), target=(278.0, 400.0, 0.0), up=(0, 1, 0), fov_x_deg=80.0, near=10.0, far=2800.0)       # the sky is directly visible
    return sb


@pytest.mark.parametrize("size", [(8, 16), (130, 67)])
def test_environment_map_texels_scale_and_rotation(gpu, gauss, size):
    import torch
    a = np.radians(40.0)
    R = np.eye(4, dtype=np.float32); R[0, 0] = R[2, 2] = np.cos(a); R[0, 2] = np.sin(a); R[2, 0] = -np.sin(a)
    sb, new = env_scene(gauss, size, 5), env_scene(gauss, size, 6, scale=1.3, to_world=R)
    fresh = gpu.Scene(new.desc())
    integ = gpu.PathHIP(maxDepth=5)
    want = render(gpu, fresh, integ, 4, A.PHIP_FLAG_NO_FUSED)
    t, scale, m, levels = new._envmap
    for kind in ("numpy", "torch"):
        gs = gpu.Scene(sb.desc())
        lv = levels if kind == "numpy" else [torch.from_numpy(l).cuda() for l in levels]
        gs.update_appearance(envmap=dict(levels=lv, scale=scale, to_world=m))
        got = render(gpu, gs, integ, 4, A.PHIP_FLAG_NO_FUSED)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], kind
    assert_is_fresh(gpu, gs, new, (0, A.PHIP_FLAG_FUSED_ANY), direct=False)
    with pytest.raises(_ffi.PhipError) as e:
        gs.update_appearance(envmap=dict(levels=[np.zeros_like(l) for l in levels]))
    assert e.value.code == A.PHIP_ERR_INVALID and "completely black" in str(e.value)
    after = render(gpu, gs, integ, 4, A.PHIP_FLAG_NO_FUSED)
    assert same_bits(after[0], want[0]) and same_bits(after[1], want[1])


def test_constant_emitter_radiance(gpu, gauss):
    sb = sphere_box(gauss, "constant", 6, 4, 32, 32)
    gs = gpu.Scene(sb.desc())
    sb.emitters[0]["radiance"] = [0.1, 0.9, 0.4]; sb.emitters[0]["weight"] = 1.7
    gs.update_appearance(emitters=emitters_of(sb.desc()))
    assert_is_fresh(gpu, gs, sb, (0, A.PHIP_FLAG_NO_FUSED, A.PHIP_FLAG_FUSED_ANY))


def test_appearance_geometry_appearance_and_the_replicas(gpu, gauss):
    sb = two_light_box(gauss)
    gs = gpu.Scene(sb.desc())
    sb.materials[0].reflectance[:] = [0.1, 0.1, 0.9]
    gs.update_appearance(materials=materials_of(sb))
    sb.positions[6] = (sb.positions[6] + np.float32(15.0)).astype(np.float32)
    gs.update(positions=sb.flat_positions())
    m = sb.materials[4]; m.type = A.PHIP_BSDF_DIELECTRIC; m.eta[0] = 1.33; m.reflectance[:] = [1, 1, 1]; m.transmittance[:] = [1, 1, 1]
    sb.emitters[1]["radiance"] = [1.0, 9.0, 1.0]
    gs.update_appearance(materials=materials_of(sb), emitters=emitters_of(sb.desc()))
    assert_is_fresh(gpu, gs, sb, SMALL_PATHS)
    integ = gpu.PathHIP(maxDepth=5)
    kw = dict(flags=A.PHIP_FLAG_ALIAS_DEVICES, devices=[0, 0])
    stale = gpu.HDRFilm(gs.width, gs.height); assert integ.render(gs, stale, 4, **kw)              # the replica exists, of the scene as it is now
    sb.materials[0].reflectance[:] = [0.9, 0.1, 0.1]
    gs.update_appearance(materials=materials_of(sb))                                               # drops it
    fresh = gpu.Scene(sb.desc())
    a, b = gpu.HDRFilm(gs.width, gs.height), gpu.HDRFilm(gs.width, gs.height)
    assert integ.render(gs, a, 4, **kw) and integ.render(fresh, b, 4, **kw)
    assert same_bits(a.storage, b.storage) and not same_bits(a.storage, stale.storage)
    single = render(gpu, fresh, integ, 4)[0]
    # two devices' films summed by a kernel: the single-device frame up to the order of a pixel's float32 additions (a few ulp of its largest term)
    np.testing.assert_allclose(a.storage, single, rtol=1e-5, atol=1e-6)

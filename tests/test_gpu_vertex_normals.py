"""phip_vertex_normals_device on the GPU: the kernel's normals are the host call's bit for bit -- on every mesh of tests/normals_reference.py, at the vertex counts
round the block and wave sizes, with sentinels round the output --, the incidence lists of the creation serve new positions after phip_scene_rebuild and
phip_scene_update, and the loop the call exists for -- deform in torch, Scene.vertex_normals, Scene.update on device tensors, render -- gives the samples, the
film and the counters of a scene freshly created from the deformed positions with the host call's normals."""
import numpy as np
import pytest

from conftest import bits
from mitsuba_amd import _abi as A, scene as S
from test_gpu_parity import gpu, soup  # noqa: F401  (the fixture)
from test_gpu_scene_update import assert_same_renders
import normals_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def scene_of(gpu, gauss, meshes):
    """a scene of the (P, T) meshes, one shape each, under a constant environment"""
    sb = S.SceneBuilder()
    sb.constant((0.8, 0.8, 0.8))
    m = sb.diffuse((0.5, 0.5, 0.5))
    for P, T in meshes:
        sb.mesh(P, T, m)
    sb.perspective((0, 0, -30), (0, 0, 0), (0, 1, 0), 40.0)
    sb.hdrfilm(16, 16, gauss)
    return sb, gpu.Scene(sb.desc())


def flat(meshes):
    """the scene's vertex and index arrays of the meshes: the second mesh's indices offset by the first's vertex count"""
    P = np.concatenate([p for p, _ in meshes]).astype(np.float32)
    offs = np.cumsum([0] + [len(p) for p, _ in meshes])
    T = np.concatenate([np.asarray(t, np.uint32).reshape(-1, 3) + np.uint32(o) for (_, t), o in zip(meshes, offs)])
    return P, T


def device_normals(gs, P):
    """Scene.vertex_normals into the middle of a buffer of sentinels -> (normals, n_invalid); the sentinels before and after must stay"""
    import torch
    n = len(P)
    buf = torch.full((n + 2, 3), SENTINEL, device="cuda")
    out, info = gs.vertex_normals(torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda(), out=buf[1:n + 1], info=True)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all()
    assert out.data_ptr() == buf.data_ptr() + 12 and info.kernel_ms > 0
    return got[1:-1], int(info.n_invalid)


def assert_device_is_host(gs, P, T):
    want, want_invalid = S.vertex_normals_angle_weighted(P, T, return_invalid=True)
    got, invalid = device_normals(gs, P)
    assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:4]
    assert invalid == want_invalid
    return want_invalid


@pytest.mark.parametrize("name", list(R.meshes()))
def test_device_equals_host_on_the_host_suites_meshes(gpu, gauss, name):
    P, T = R.meshes()[name]
    if name == "two_ranges":                                        # as two shapes
        _, _, (nv0, nt0) = R.two_ranges()
        parts = [(P[:nv0], T[:nt0]), (P[nv0:], T[nt0:] - np.uint32(nv0))]
    else:
        parts = [(P, T)]
    sb, gs = scene_of(gpu, gauss, parts)
    fp, ft = flat(parts)
    assert (fp == P).all() and (ft == T).all()
    invalid = assert_device_is_host(gs, P, T)
    assert (bits(device_normals(gs, P)[0]) == bits(R.reference(name)[0])).all()          # ... and the restatement's, a second call on the cached lists
    if name == "degenerate":
        assert invalid == R.DEGENERATE_INVALID
    gs.close()


def strip(n, seed):
    """n vertices on a jittered helix, triangles (i, i + 1, i + 2): valence 1 to 3"""
    rng = np.random.default_rng(seed)
    a = 0.4 * np.arange(n)
    P = (np.stack([np.cos(a), 0.1 * a, np.sin(a)], -1) * 3 + rng.uniform(-0.2, 0.2, (n, 3))).astype(np.float32)
    T = np.stack([np.arange(n - 2), np.arange(n - 2) + 1, np.arange(n - 2) + 2], -1).astype(np.uint32) if n > 2 else np.zeros((0, 3), np.uint32)
    return P, T


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_grid_tail(gpu, gauss, n):
    """one vertex and no triangle; one short of a wave, a wave, one more; one more than a block"""
    P, T = strip(n, n)
    sb, gs = scene_of(gpu, gauss, [(P, T)])
    invalid = assert_device_is_host(gs, P, T)
    assert invalid == (1 if n == 1 else 0)
    gs.close()


@pytest.mark.parametrize("entry", ["rebuild", "update"])
def test_cached_lists_serve_new_positions_after_rebuild_and_update(gpu, gauss, entry):
    """the 4096-triangle soup as two shapes over one vertex array each (half of every shape's vertices belong to no triangle of it)"""
    rng = np.random.default_rng(17)
    P, T = soup(rng, 4096, size=0.3, extent=8.0)
    half = len(T) // 2
    parts = [(P, T[:half]), (P, T[half:])]
    sb, gs = scene_of(gpu, gauss, parts)
    fp, ft = flat(parts)
    assert assert_device_is_host(gs, fp, ft) == len(fp) // 2          # the lists are made here, on the creation's positions
    moved = (fp + (0.05 if entry == "update" else 1.2) * np.sin(fp[:, [1, 2, 0]] * (np.pi / 8.0) + np.array([0.3, 1.1, 2.0]))).astype(np.float32)
    getattr(gs, entry)(positions=moved)
    assert_device_is_host(gs, moved, ft)
    assert_device_is_host(gs, fp, ft)
    gs.close()


def angle_sphere_box(gauss):
    """the Cornell box with two tessellated spheres (S.cornell_spheres' places, ~1.1 k triangles) whose normals are normals="angle" """
    sb = S.SceneBuilder()
    S.cornell_box(32, 32, gauss, sb=sb)
    m0, m1 = sb.diffuse((0.7, 0.6, 0.3)), sb.twosided(sb.roughconductor(S.CU_ETA, S.CU_K, alpha=0.15))
    for centre, radius, m in (((185, 120, 170), 70.0, m0), ((370, 330, 350), 60.0, m1)):
        P, T, _ = S.sphere_mesh(centre, radius, 24, 12)
        sb.mesh(P, T, m, normals="angle")
    return sb


def test_deform_normals_update_render_equals_a_fresh_scene(gpu, gauss):
    import torch
    sb = angle_sphere_box(gauss)
    gs = gpu.Scene(sb.desc())
    assert gs.desc.n_triangles > 1000
    pos = torch.from_numpy(sb.flat_positions()).cuda()
    first = sum(len(p) for p in sb.positions[:-2])                  # the spheres are the last two shapes
    sph = pos[first:]
    pos[first:] = sph + 9.0 * torch.sin(sph[:, [1, 2, 0]] * 0.045 + torch.tensor([0.3, 1.1, 2.0], device="cuda"))
    nrm = gs.vertex_normals(pos)
    gs.update(positions=pos, normals=nrm)
    moved = pos.cpu().numpy()
    at = first
    for i in (len(sb.positions) - 2, len(sb.positions) - 1):
        n = len(sb.positions[i])
        sb.positions[i] = moved[at:at + n].copy()
        sb.normals[i] = S.vertex_normals_angle_weighted(sb.positions[i], sb.indices[i])
        assert (bits(nrm[at:at + n].cpu().numpy()) == bits(sb.normals[i])).all()
        at += n
    fresh = gpu.Scene(sb.desc())
    integ = gpu.PathHIP(maxDepth=5)
    film, smp, counters = assert_same_renders(gpu, gs, fresh, integ, 4, (0, A.PHIP_FLAG_NO_FUSED))
    assert np.isfinite(film).all() and film[..., :3].max() > 0 and counters[0] == 32 * 32 * 4
    gs.close(); fresh.close()

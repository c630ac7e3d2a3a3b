"""phip_trace_device without a GPU: its place in the ABI, and the surface records (phip_surface) as the host twin of k_surfaces builds them -- phip_debug_host_surfaces
runs the creation's own shading-record stage and fillSurface of dv_scene.h, the one statement the kernel evaluates -- against float64 numpy on the descriptor's
arrays.  The hits come from the oracle's sweep over all triangles, the structure-independent answer every ray cast of the library returns.

Tolerances: 1e-5 of the scene's extent for points, 1e-5 for unit vectors and texture coordinates -- two orders of magnitude above what the float32 sums, cross
products and normalisations of fillIntersection lose on these meshes (a few 2^-24 relative), far below a wrong vertex, a wrong weight or an unflipped normal.
The side of arrival, and with it the leaf BSDF, is decided by the sign of ns.d in float32: it is compared where |ns.d| > 1e-3 (random unit directions leave
about 0.1 % of the hits out; the tests assert that it is less than 1 %)."""
import ctypes as C
import os
import subprocess

import numpy as np

from mitsuba_amd import _abi as A, _ffi, scene as S
from test_gpu_parity import random_rays

HERE = os.path.dirname(os.path.abspath(__file__))
NO_HIT = 0xFFFFFFFF


def host_surfaces(phip, desc, rays, hits):
    """(n, 16) uint32: the words of the phip_surface of every (ray, hit) as the host twin makes them"""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8); h = np.ascontiguousarray(hits, np.float32).reshape(-1, 4)
    out = np.zeros((len(r), 16), np.uint32)
    rc = phip.phip_debug_host_surfaces(C.byref(desc), r.ctypes.data_as(C.POINTER(A.phip_ray)), h.ctypes.data_as(C.POINTER(A.phip_hit)), len(r),
                                       out.ctypes.data_as(C.POINTER(A.phip_surface)))
    assert rc == 0, phip.phip_last_error()
    return out


def fields(words):
    f = words.view(np.float32)
    return dict(p=f[:, 0:3], t=f[:, 3], ng=f[:, 4:7], prim=words[:, 7], ns=f[:, 8:11], flags=words[:, 11], uv=f[:, 12:14], material=words[:, 14], emitter=words[:, 15].view(np.int32))


def check_surfaces(phip, oracle, desc, rays, min_hits, min_back=0):
    """the host twin's records of the sweep's hits on `desc`, every field against float64 numpy; returns the records' fields (hits only) and the hit mask"""
    osc = oracle.OracleScene(desc)
    hits, _, _ = osc.trace(rays, True, False, bruteforce=True)
    osc.close()
    words = host_surfaces(phip, desc, rays, hits)
    hw = hits.view(np.uint32)
    hit = hw[:, 3] != NO_HIT
    assert hit.sum() >= min_hits and (~hit).sum() > 0, (hit.sum(), len(hit))
    # a miss: prim = PHIP_NO_HIT, every other word zero
    miss = words[~hit]
    assert (miss[:, 7] == NO_HIT).all() and (np.delete(miss, 7, axis=1) == 0).all()
    s = {k: v[hit] for k, v in fields(words).items()}
    prim = hw[hit, 3]; u = hits[hit, 1].astype(np.float64); v = hits[hit, 2].astype(np.float64); d = rays[hit, 4:7].astype(np.float64)
    assert (s["prim"] == prim).all() and (s["t"].view(np.uint32) == hw[hit, 0]).all()
    P = np.ctypeslib.as_array(desc.positions, shape=(desc.n_vertices, 3)).astype(np.float64)
    T = np.ctypeslib.as_array(desc.indices, shape=(desc.n_triangles, 3))
    shape_of = np.zeros(desc.n_triangles, np.int64)
    for i in range(desc.n_shapes):
        shape_of[desc.shapes[i].first_triangle:desc.shapes[i].first_triangle + desc.shapes[i].n_triangles] = i
    sh = shape_of[prim]
    extent = float((P.max(0) - P.min(0)).max())
    b = np.stack([1 - u - v, u, v], 1)
    p0, p1, p2 = P[T[prim, 0]], P[T[prim, 1]], P[T[prim, 2]]
    # p: the barycentric sum of the vertices, on the triangle
    want_p = b[:, :1] * p0 + b[:, 1:2] * p1 + b[:, 2:] * p2
    assert np.abs(s["p"] - want_p).max() <= 1e-5 * extent
    assert (b >= -1e-5).all() and (b <= 1 + 1e-5).all()
    e1, e2 = p1 - p0, p2 - p0
    face = np.cross(e1, e2); face /= np.linalg.norm(face, axis=1, keepdims=True)
    assert np.abs(np.einsum("ij,ij->i", s["p"] - p0, face)).max() <= 1e-5 * extent
    # ng: unit, perpendicular to both edges
    ng = s["ng"].astype(np.float64)
    assert np.abs(np.linalg.norm(ng, axis=1) - 1).max() <= 1e-5
    for e in (e1, e2):
        assert np.abs(np.einsum("ij,ij->i", ng, e / np.linalg.norm(e, axis=1, keepdims=True))).max() <= 1e-5
    # ns: the normalised interpolated vertex normal, ng on its side; the face normal itself on a flat-shaded mesh
    ns = s["ns"].astype(np.float64)
    has_n = np.array([desc.shapes[i].has_normals != 0 for i in range(desc.n_shapes)])[sh]
    if has_n.any():
        N = np.ctypeslib.as_array(desc.normals, shape=(desc.n_vertices, 3)).astype(np.float64)
        want_n = b[:, :1] * N[T[prim, 0]] + b[:, 1:2] * N[T[prim, 1]] + b[:, 2:] * N[T[prim, 2]]
        want_n /= np.linalg.norm(want_n, axis=1, keepdims=True)
        assert np.abs(ns - want_n)[has_n].max() <= 1e-5
        assert (np.einsum("ij,ij->i", ng, ns)[has_n] >= 0).all()
    assert (s["ns"].view(np.uint32) == s["ng"].view(np.uint32))[~has_n].all()
    assert (np.abs(np.einsum("ij,ij->i", ng, face)) >= 1 - 1e-5).all()
    # uv: the interpolated texture coordinates, (u, v) of the hit on a mesh without
    has_uv = np.array([desc.shapes[i].has_texcoords != 0 for i in range(desc.n_shapes)])[sh]
    if has_uv.any():
        UV = np.ctypeslib.as_array(desc.texcoords, shape=(desc.n_vertices, 2)).astype(np.float64)
        want_uv = b[:, :1] * UV[T[prim, 0]] + b[:, 1:2] * UV[T[prim, 1]] + b[:, 2:] * UV[T[prim, 2]]
        assert np.abs(s["uv"] - want_uv)[has_uv].max() <= 1e-5
    assert (s["uv"].view(np.uint32) == hw[hit, 1:3])[~has_uv].all()
    # emitter, and -- away from grazing arrival -- the side and the leaf BSDF of that side, from the descriptor
    assert (s["emitter"] == np.array([desc.shapes[i].emitter for i in range(desc.n_shapes)])[sh]).all()
    cos = np.einsum("ij,ij->i", ns, -d)
    sure = np.abs(cos) > 1e-3
    assert (~sure).mean() <= 0.01, (~sure).mean()
    back = cos <= 0
    assert ((s["flags"] & A.PHIP_SURFACE_BACK) != 0)[sure].tolist() == back[sure].tolist()
    assert (s["flags"] & ~np.uint32(A.PHIP_SURFACE_BACK) == 0).all()
    assert back[sure].sum() >= min_back
    mat = np.array([desc.shapes[i].material for i in range(desc.n_shapes)])[sh]
    two = np.array([desc.materials[i].type == A.PHIP_BSDF_TWOSIDED for i in range(desc.n_materials)])
    nested = np.array([[desc.materials[i].nested[0], desc.materials[i].nested[1]] for i in range(desc.n_materials)])
    want_mat = np.where(two[mat], nested[mat, back.astype(int)], mat)
    assert (s["material"][sure] == want_mat[sure]).all()
    return s, hit


def test_abi_of_phip_trace_device(phip, have_gpu):
    header = open(os.path.join(HERE, "..", "include", "phip.h")).read()
    assert "int  phip_trace_device(phip_scene *scene, const phip_ray *d_rays, size_t n," in header and "} phip_surface;" in header
    assert A.PHIP_ABI_VERSION == 7 and "#define PHIP_ABI_VERSION 7" in header                # declarations only: no struct of the ABI changed
    assert phip.phip_abi_sizeof(13) == 64 == C.sizeof(A.phip_surface)
    assert phip.phip_abi_sizeof(8) == 32 and phip.phip_abi_sizeof(9) == 16 and phip.phip_abi_sizeof(14) == 0
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB], capture_output=True, text=True).stdout
    assert " phip_trace_device" in out and "phip_debug_" not in out
    dbg = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_DEBUG], capture_output=True, text=True).stdout
    assert "phip_debug_host_surfaces" in dbg
    assert phip.phip_trace_device(None, None, 0, None, None, None, None, None) == A.PHIP_ERR_INVALID
    if not have_gpu:
        never_read = C.create_string_buffer(64)
        assert phip.phip_trace_device(C.cast(never_read, C.c_void_p), C.cast(never_read, C.c_void_p), 1, None, None, None, None, None) == A.PHIP_ERR_DEVICE      # no CPU fallback
        assert phip.phip_last_error()
    from mitsuba_amd.integrator import Scene
    assert Scene.rayIntersectDevice.__code__.co_varnames[:6] == ("self", "rays", "closest", "shadow", "surfaces", "stream")
    assert ("phip_raycast.hip", [], "phip_raycast.o") in _ffi.UNITS                          # a unit of its own


def test_surfaces_of_the_cornell_box(phip, oracle, gauss):
    """flat-shaded rectangles, one of them the area light: ns = ng = the face normal, uv = (u, v) of the hit, the emitter id on the light's two triangles"""
    desc = S.cornell_box(32, 32, gauss).desc()
    rays = random_rays(np.random.default_rng(11), 20000, -100, 650)          # some start outside the box and miss it
    s, hit = check_surfaces(phip, oracle, desc, rays, min_hits=10000, min_back=100)
    assert (s["emitter"] >= 0).sum() > 20 and (s["emitter"] == -1).sum() > 10000


def test_surfaces_of_a_sphere_with_vertex_normals_and_texture_coordinates(phip, oracle, gauss):
    """500 triangles with vertex normals and texture coordinates; rays start inside and outside, so both sides of arrival occur"""
    rng = np.random.default_rng(12)
    P, T, N = S.sphere_mesh((0.3, -0.2, 0.1), 1.5, 25, 11)
    assert len(T) == 500
    sb = S.SceneBuilder()
    sb.mesh(P, T, sb.diffuse((0.5, 0.6, 0.7)), normals=N, uvs=rng.uniform(-2, 3, (len(P), 2)))
    sb.perspective((0, 0, -6), (0, 0, 0), (0, 1, 0), 40.0)
    sb.hdrfilm(32, 32, gauss)
    desc = sb.desc()
    s, hit = check_surfaces(phip, oracle, desc, random_rays(rng, 20000, -2.5, 2.5, mint=0.0), min_hits=3000, min_back=1000)      # (about a fifth of the chords of the cube meet the sphere)
    assert (s["flags"] == 0).sum() >= 1000


def test_surfaces_of_a_twosided_quad_from_both_sides(phip, oracle, gauss):
    """a `twosided` adapter with two different nested models: the record names the model of the side the ray arrives on"""
    rng = np.random.default_rng(13)
    sb = S.SceneBuilder()
    front, back = sb.diffuse((0.8, 0.1, 0.1)), sb.diffuse((0.1, 0.1, 0.8))
    plain = sb.diffuse((0.5, 0.5, 0.5))
    sb.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), sb.twosided(front, back), facing=(0, 1, 0))
    sb.quad((-1, -3, -1), (1, -3, -1), (1, -3, 1), (-1, -3, 1), plain, facing=(0, 1, 0), radiance=(1, 1, 1))      # one-sided: its own material from either side
    sb.perspective((0, 5, -5), (0, 0, 0), (0, 1, 0), 40.0)
    sb.hdrfilm(32, 32, gauss)
    desc = sb.desc()
    rays = random_rays(rng, 8000, -1.5, 1.5, mint=0.0)
    rays[:, 1] = rng.uniform(-4.0, 1.5, len(rays))
    s, hit = check_surfaces(phip, oracle, desc, rays, min_hits=1000, min_back=300)
    seen = set(zip(s["material"].tolist(), (s["flags"] & 1).tolist()))
    assert {(front, 0), (back, 1), (plain, 0), (plain, 1)} <= seen, seen

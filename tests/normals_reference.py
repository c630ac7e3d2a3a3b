"""What tests/test_vertex_normals_host.py and tests/test_gpu_vertex_normals.py share: a numpy restatement of the reference's TriMesh::computeNormals
(trimesh.cpp:640-672, with unitAngle of core/util.h:309-314 and the vector operators of core/vector.h) in float32, every operation a single step, and the meshes
the two suites run on.  asin is np.float32(np.arcsin(np.float64(x))): the correctly rounded value, which is what pm_asinf returns."""
import numpy as np

f32 = np.float32
PI = f32(3.14159265358979323846)          # M_PI_FLT, constants.h:63


def _length(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])          # float32 scalars: every product and sum rounds once, left to right


def _div(v, s):
    recip = f32(1) / s                                                # TVector3::operator/ : one reciprocal, three products
    return np.array([v[0] * recip, v[1] * recip, v[2] * recip], f32)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def asin32(x):
    return f32(np.arcsin(np.float64(x)))


def unit_angle(u, v, taken=None):
    if u[0] * v[0] + u[1] * v[1] + u[2] * v[2] < 0:
        if taken is not None:
            taken[0] += 1
        return PI - f32(2) * asin32(f32(0.5) * _length(v + u))
    if taken is not None:
        taken[1] += 1
    return f32(2) * asin32(f32(0.5) * _length(v - u))


def reference_normals(P, T):
    """(normals, n_invalid, [corners through the dot < 0 branch, corners through the other])"""
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    N = np.zeros_like(P)
    taken = [0, 0]
    with np.errstate(all="ignore"):
        for tri in T:
            n = None
            for i in range(3):
                v0, v1, v2 = P[tri[i]], P[tri[(i + 1) % 3]], P[tri[(i + 2) % 3]]
                side_a, side_b = v1 - v0, v2 - v0
                if i == 0:
                    n = _cross(side_a, side_b)
                    length = _length(n)
                    if length == 0:
                        break
                    n = _div(n, length)
                angle = unit_angle(_div(side_a, _length(side_a)), _div(side_b, _length(side_b)), taken)
                N[tri[i]] += n * angle
        invalid = 0
        for i in range(len(N)):
            length = _length(N[i])
            if length != 0:
                N[i] = _div(N[i], length)
            else:
                invalid += 1
                N[i] = (1, 0, 0)
    return N, invalid, taken


def icosphere(subdivisions=2):
    """(P, T) of the unit icosphere: 20 * 4^subdivisions triangles, outward winding"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    V = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in V]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, G = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in F:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return np.asarray(V, f32), np.asarray(F, np.uint32)


def jittered_icosphere(jitter=0.08, seed=11):
    """320 triangles, 162 vertices, every vertex moved by up to `jitter` per axis: irregular enough that area and angle weighting differ visibly"""
    P, T = icosphere(2)
    rng = np.random.default_rng(seed)
    return (P + rng.uniform(-jitter, jitter, P.shape)).astype(f32), T


def fan(valence=65, seed=5):
    """`valence` triangles round vertex 0, a shallow jittered cone: one incidence list longer than a wave is wide"""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, valence, endpoint=False)
    rim = np.stack([np.cos(a), np.sin(a), -0.3 + 0.1 * rng.uniform(-1, 1, valence)], -1) * (1 + 0.2 * rng.uniform(-1, 1, (valence, 1)))
    P = np.concatenate([[[0, 0, 0.1]], rim]).astype(f32)
    T = np.stack([np.zeros(valence, np.int64), 1 + np.arange(valence), 1 + (np.arange(valence) + 1) % valence], -1).astype(np.uint32)
    return P, T


def obtuse():
    """three triangles round a nearly flat apex (corners of ~120 degrees there) and a sliver with a corner of ~170 degrees: unitAngle's dot < 0 branch"""
    P = np.array([[0, 0, 0.05], [1, 0, 0], [-0.5, 0.8660254, 0], [-0.5, -0.8660254, 0], [2, 0.1, 0.3], [0.4, 0.05, 0.2]], f32)
    T = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [5, 1, 4], [1, 5, 0]], np.uint32)
    return P, T


def degenerate():
    """a zero-area triangle (3, 4, 5: exactly on one line), a triangle that names a vertex twice (6, 6, 7) and an unreferenced vertex (8), beside two proper
    triangles that share an edge; vertex 3 belongs to a proper triangle and to the zero-area one.  Nothing contributes to 4, 5, 6, 7 and 8"""
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.25], [1, 1, 0], [2, 2, 0], [4, 4, 0], [5, 0, 1], [6, 1, 1], [7, 7, 7]], f32)
    T = np.array([[0, 1, 2], [3, 4, 5], [1, 3, 2], [6, 6, 7]], np.uint32)
    return P, T


DEGENERATE_INVALID = 5                   # vertices 4 .. 8 of degenerate()


def two_ranges():
    """two meshes in one index array, the second's indices offset by the first's vertex count: the layout of two shapes of a scene"""
    (P0, T0), (P1, T1) = jittered_icosphere(0.05, 3), fan(7, 9)
    return np.concatenate([P0, P1]).astype(f32), np.concatenate([T0, T1 + np.uint32(len(P0))]).astype(np.uint32), (len(P0), len(T0))


def single():
    return np.array([[0, 0, 0], [1, 0.5, 0], [0.25, 1, 0.5]], f32), np.array([[0, 1, 2]], np.uint32)


def meshes():
    """name -> (P, T) of every mesh of the issue's list"""
    P2, T2, _ = two_ranges()
    return {"single": single(), "fan65": fan(65), "icosphere": jittered_icosphere(), "obtuse": obtuse(), "degenerate": degenerate(), "two_ranges": (P2, T2)}


_REFERENCE = {}


def reference(name):
    """reference_normals of meshes()[name], computed once per process"""
    if name not in _REFERENCE:
        _REFERENCE[name] = reference_normals(*meshes()[name])
    return _REFERENCE[name]

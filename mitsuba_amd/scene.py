"""Host-side scene assembly for the `path_hip` back end.

`SceneBuilder` plays the role of the Mitsuba plugin shim's flattening step
(mitsuba_amd/plugin/path_hip.cpp walks Scene::getShapes()/getEmitters()/getSensor() and fills
the same phip_scene_desc): triangle meshes with a material and an optional area emitter, a
perspective sensor and an hdrfilm with a reconstruction filter.  Names follow the reference's
XML vocabulary (shape / bsdf / emitter / sensor / film / rfilter).

Benchmark scenes (BASELINE.json configs; the reference ships no Cornell/Sponza assets, so they
are generated deterministically here):
    cornell_box()      -- classic measured Cornell box, diffuse + quad area light   (C1, C2)
    atrium()           -- "Sponza-class" procedural atrium, ~260k triangles         (C3, C5)
    glass_room()       -- tiled room with tessellated glass objects, ~150k tris     (C4)
"""
import ctypes as C
import math
import numpy as np

from . import _abi as A


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def look_at(origin, target, up):
    """Transform::lookAt (src/libcore/transform.cpp:191-214): camera looks down +z, x = left."""
    p = np.asarray(origin, np.float64)
    t = np.asarray(target, np.float64)
    u = np.asarray(up, np.float64)
    d = t - p
    d /= np.linalg.norm(d)
    left = np.cross(u, d)
    left /= np.linalg.norm(left)
    new_up = np.cross(d, left)
    m = np.eye(4)
    m[:3, 0] = left
    m[:3, 1] = new_up
    m[:3, 2] = d
    m[:3, 3] = p
    return m.astype(np.float32)


def mip_pyramid(level0):
    """MIP levels of an (H, W, 3) image with the level sizes of TMIPMap (max(1, (n+1)/2) down to 1x1, mipmap.h:182-192);
    each level is an area-weighted box resampling of level 0 (a stand-in for the reference's 2-lobe Lanczos resampler)."""
    out = [np.ascontiguousarray(level0, np.float32)]
    h, w = out[0].shape[:2]
    src = out[0].astype(np.float64)

    def resample_axis(a, n_out, axis):
        n_in = a.shape[axis]
        edges = np.linspace(0, n_in, n_out + 1)
        res = []
        for i in range(n_out):
            lo, hi = edges[i], edges[i + 1]
            idx = np.arange(int(np.floor(lo)), int(np.ceil(hi)))
            wgt = np.minimum(idx + 1, hi) - np.maximum(idx, lo)
            sl = np.take(a, idx, axis=axis)
            shape = [1] * a.ndim; shape[axis] = len(idx)
            res.append((sl * wgt.reshape(shape)).sum(axis=axis) / (hi - lo))
        return np.stack(res, axis=axis)
    while w > 1 or h > 1:
        w, h = max(1, (w + 1) // 2), max(1, (h + 1) // 2)
        out.append(np.ascontiguousarray(resample_axis(resample_axis(src, h, 0), w, 1), np.float32))
    return out


WRAP_MODES = {"clamp": A.PHIP_WRAP_CLAMP, "repeat": A.PHIP_WRAP_REPEAT, "mirror": A.PHIP_WRAP_MIRROR, "zero": A.PHIP_WRAP_ZERO, "one": A.PHIP_WRAP_ONE}


def pyramid_sizes(w, h):
    """[(h, w)] of every level of a complete pyramid, level 0 first (mipmap.h:182-192)"""
    out = [(h, w)]
    while w > 1 or h > 1:
        w, h = max(1, (w + 1) // 2), max(1, (h + 1) // 2)
        out.append((h, w))
    return out


def mip_pyramid_lanczos(level0, wrap_u="repeat", wrap_v=None, max_value=1.0):
    """MIP levels of an (H, W, 3) image exactly as the reference's TMIPMap builds and stores them (phip_mip_pyramid: the two-lobe Lanczos resampler per axis, every
    level from the float32 level before it, clamped to [0, max_value], stored in half precision) -- level 0 included, which comes back clamped at 0 and rounded.
    wrap_u / wrap_v: "clamp", "repeat", "mirror", "zero", "one" or the PHIP_WRAP_* value; a texture takes its own wrap modes and max_value 1, an environment map
    repeat x clamp and infinity.  Runs on the host: no GPU is needed."""
    from . import _ffi
    t = np.ascontiguousarray(level0, dtype=np.float32)
    assert t.ndim == 3 and t.shape[2] == 3
    sizes = pyramid_sizes(t.shape[1], t.shape[0])
    out = [np.empty((h, w, 3), np.float32) for h, w in sizes]
    p = A.phip_pyramid_desc()
    p.width, p.height, p.n_levels = t.shape[1], t.shape[0], len(sizes)
    p.wrap_u = WRAP_MODES.get(wrap_u, wrap_u)
    p.wrap_v = p.wrap_u if wrap_v is None else WRAP_MODES.get(wrap_v, wrap_v)
    p.max_value = max_value
    p.d_level0 = t.ctypes.data
    for l, o in enumerate(out):
        p.d_levels[l] = o.ctypes.data
    rc = _ffi.lib().phip_mip_pyramid(C.byref(p))
    if rc != 0:
        raise _ffi.PhipError(rc, "phip_mip_pyramid")
    return out


def vertex_normals_angle_weighted(P, T, return_invalid=False):
    """Vertex normals of the mesh (P: (n, 3) positions, T: (m, 3) indices) exactly as the reference's TriMesh::computeNormals makes them for a mesh loaded without
    normals (phip_vertex_normals: every corner adds its triangle's unit normal times its angle, in triangle order; a vertex nothing contributes to gets (1, 0, 0)).
    Returns the (n, 3) float32 normals, with return_invalid=True also the number of vertices that got (1, 0, 0).  Runs on the host: no GPU is needed."""
    from . import _ffi
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    T = np.ascontiguousarray(T, dtype=np.uint32).reshape(-1, 3)
    N = np.empty_like(P)
    d = A.phip_normals_desc(n_vertices=len(P), n_triangles=len(T), indices=T.ctypes.data if len(T) else None, positions=P.ctypes.data, normals=N.ctypes.data)
    info = A.phip_normals_info()
    rc = _ffi.lib().phip_vertex_normals(C.byref(d), C.byref(info))
    if rc != 0:
        raise _ffi.PhipError(rc, "phip_vertex_normals")
    return (N, int(info.n_invalid)) if return_invalid else N


class SceneBuilder:
    def __init__(self):
        self.positions = []      # list of (n,3) float32
        self.normals = []        # list of (n,3) float32 or None
        self.indices = []        # list of (m,3) uint32 (local to the mesh)
        self.shapes = []         # dicts
        self.materials = []      # phip_material
        self.emitters = []       # dicts
        self.uvs = []            # list of (n,2) float32 or None
        self.textures = []       # dicts
        self.camera = None
        self.film = None
        self._keep = []

    # ---- bsdfs -------------------------------------------------------------------------
    def _add_material(self, m):
        self.materials.append(m)
        return len(self.materials) - 1

    def diffuse(self, reflectance=(0.5, 0.5, 0.5), texture=None):
        """`texture` = id returned by bitmap(): <texture type="bitmap" name="reflectance">"""
        m = A.phip_material()
        m.type = A.PHIP_BSDF_DIFFUSE
        m.reflectance[:] = _rgb(reflectance)
        m.reflectance_texture = 0 if texture is None else texture + 1
        return self._add_material(m)

    def bitmap(self, image, wrap="repeat", wrap_v=None, filter_type="ewa", max_anisotropy=20.0,
               uscale=1.0, vscale=1.0, uoffset=0.0, voffset=0.0, pyramid=True):
        """<texture type="bitmap">: `image` = (H, W, 3) float RGB in [0, 1] as the plugin stores MIP level 0; the pyramid
        comes from `mip_pyramid` (or pass the levels; pyramid="lanczos": the reference's own levels from `mip_pyramid_lanczos`, level 0 included) unless the filter
        is nearest / bilinear."""
        wraps = WRAP_MODES
        filters = {"nearest": A.PHIP_FILTER_NEAREST, "bilinear": A.PHIP_FILTER_BILINEAR, "trilinear": A.PHIP_FILTER_TRILINEAR, "ewa": A.PHIP_FILTER_EWA}
        t = np.ascontiguousarray(image, dtype=np.float32)
        assert t.ndim == 3 and t.shape[2] == 3
        need = filter_type in ("trilinear", "ewa")          # mipmap.h:182-192: nearest / bilinear keep a single level
        if isinstance(pyramid, str):
            assert pyramid == "lanczos", pyramid
            levels = mip_pyramid_lanczos(t, wrap, wrap_v or wrap, 1.0) if need else [t]
        else:
            levels = (mip_pyramid(t) if pyramid is True else [t] + [np.ascontiguousarray(l, np.float32) for l in pyramid[1:]]) if need else [t]
        self.textures.append({"levels": levels, "wrap_u": wraps[wrap], "wrap_v": wraps[wrap_v or wrap], "filter": filters[filter_type],
                              "aniso": float(max_anisotropy), "scale": (float(uscale), float(vscale)), "offset": (float(uoffset), float(voffset))})
        return len(self.textures) - 1

    def dielectric(self, int_ior=1.5046, ext_ior=1.000277, specular_reflectance=1.0, specular_transmittance=1.0, texture=None, transmittance_texture=None):
        """defaults: intIOR bk7, extIOR air (src/bsdfs/dielectric.cpp:149-152, ior.h); `transmittance_texture`: <texture name="specularTransmittance">"""
        m = A.phip_material()
        m.type = A.PHIP_BSDF_DIELECTRIC
        m.eta[0] = np.float32(np.float32(int_ior) / np.float32(ext_ior))
        m.reflectance[:] = _rgb(specular_reflectance)
        m.transmittance[:] = _rgb(specular_transmittance)
        m.reflectance_texture = 0 if texture is None else texture + 1      # <texture name="specularReflectance">
        m.transmittance_texture = 0 if transmittance_texture is None else transmittance_texture + 1
        return self._add_material(m)

    def roughconductor(self, eta, k, alpha=0.1, alpha_v=None, distribution="beckmann", sample_visible=True,
                       specular_reflectance=1.0, ext_eta=1.000277, texture=None, alpha_texture=None, alpha_v_texture=None):
        """eta/k are linear-RGB (the host converts data/ior/*.spd, roughconductor.cpp:176-190).  `alpha_texture`: <texture name="alpha">
        (or name="alphaU" when `alpha_v_texture`, <texture name="alphaV">, is given too); the roughness is the texture's RGB average."""
        m = A.phip_material()
        m.type = A.PHIP_BSDF_ROUGHCONDUCTOR
        e = np.float32(ext_eta)
        m.eta[:] = [float(np.float32(x) / e) for x in _rgb(eta)]
        m.k[:] = [float(np.float32(x) / e) for x in _rgb(k)]
        m.alpha_u = alpha
        m.alpha_v = alpha if alpha_v is None else alpha_v
        m.distribution = {"beckmann": A.PHIP_MF_BECKMANN, "ggx": A.PHIP_MF_GGX}[distribution]
        m.sample_visible = 1 if sample_visible else 0
        m.reflectance[:] = _rgb(specular_reflectance)
        m.reflectance_texture = 0 if texture is None else texture + 1      # <texture name="specularReflectance">
        m.alpha_u_texture = 0 if alpha_texture is None else alpha_texture + 1
        m.alpha_v_texture = m.alpha_u_texture if alpha_v_texture is None else alpha_v_texture + 1
        return self._add_material(m)

    def twosided(self, front, back=None):
        m = A.phip_material()
        m.type = A.PHIP_BSDF_TWOSIDED
        m.nested[0] = front
        m.nested[1] = front if back is None else back
        return self._add_material(m)

    # ---- shapes ------------------------------------------------------------------------
    def mesh(self, positions, triangles, material, normals=None, radiance=None, sampling_weight=1.0, uvs=None):
        positions = _f32(positions).reshape(-1, 3)
        triangles = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        if isinstance(normals, str):         # normals="angle": the reference's own for a mesh loaded without normals (vertex_normals_angle_weighted)
            assert normals == "angle", normals
            normals = vertex_normals_angle_weighted(positions, triangles)
        if normals is not None:
            normals = _f32(normals).reshape(-1, 3)
            assert normals.shape == positions.shape
        sid = len(self.shapes)
        emitter = -1
        if radiance is not None:
            emitter = len(self.emitters)
            self.emitters.append({"radiance": _rgb(radiance), "weight": sampling_weight, "shape": sid})
        if uvs is not None:
            uvs = _f32(uvs).reshape(-1, 2)
            assert len(uvs) == len(positions)
        self.uvs.append(uvs)
        self.positions.append(positions)
        self.normals.append(normals)
        self.indices.append(triangles)
        self.shapes.append({"material": material, "emitter": emitter})
        return sid

    def constant(self, radiance, sampling_weight=1.0):
        """<emitter type="constant">: the constant environment emitter (src/emitters/constant.cpp)."""
        self.emitters.append({"radiance": _rgb(radiance), "weight": sampling_weight, "shape": 0xFFFFFFFF,
                              "type": A.PHIP_EMITTER_CONSTANT})
        return len(self.emitters) - 1

    def envmap(self, texels, scale=1.0, to_world=None, sampling_weight=1.0, pyramid=False):
        """<emitter type="envmap">: lat-long radiance map (src/emitters/envmap.cpp); `texels` = (H, W, 3) float RGB
        (MIP level 0 as the reference stores it), `to_world` = 4x4 emitter-to-world (rotation).  `pyramid=True` adds
        the MIP levels the filtered background lookup needs (the Mitsuba shim passes the plugin's own Lanczos pyramid;
        this harness builds a box-filtered one with `mip_pyramid` -- product and oracle consume the same levels); pyramid="lanczos": the
        reference's own levels (`mip_pyramid_lanczos` with repeat x clamp and no upper bound), level 0 included."""
        t = np.ascontiguousarray(texels, dtype=np.float32)
        assert t.ndim == 3 and t.shape[2] == 3
        if isinstance(pyramid, str):
            assert pyramid == "lanczos", pyramid
            levels = mip_pyramid_lanczos(t, "repeat", "clamp", float("inf"))
            t = levels[0]
            pyramid = levels
        levels = mip_pyramid(t) if pyramid is True else ([t] + [np.ascontiguousarray(l, np.float32) for l in pyramid[1:]] if pyramid else [t])
        self._envmap = (t, float(scale), np.eye(4, dtype=np.float32) if to_world is None else np.asarray(to_world, np.float32).reshape(4, 4), levels)
        self.emitters.append({"radiance": (0.0, 0.0, 0.0), "weight": sampling_weight, "shape": 0xFFFFFFFF,
                              "type": A.PHIP_EMITTER_ENVMAP})
        return len(self.emitters) - 1

    def quad(self, p0, p1, p2, p3, material, facing=None, radiance=None, uvs=None):
        """Two triangles (0,1,2),(2,3,0) like Rectangle::createTriMesh (rectangle.cpp:170-203);
        if `facing` is given the winding is flipped so the face normal points that way.  uvs=True: the rectangle's
        own parameterisation (0,0) (1,0) (1,1) (0,1); or four (u, v) pairs."""
        P = _f32([p0, p1, p2, p3])
        if uvs is True:
            uvs = [(0, 0), (1, 0), (1, 1), (0, 1)]
        U = _f32(uvs) if uvs is not None else None
        n = np.cross(P[1] - P[0], P[2] - P[0])
        if facing is not None and np.dot(n, np.asarray(facing, np.float32)) < 0:
            P = P[::-1].copy()
            if U is not None:
                U = U[::-1].copy()
        return self.mesh(P, [[0, 1, 2], [2, 3, 0]], material, radiance=radiance, uvs=U)

    # ---- sensor / film ------------------------------------------------------------------
    def perspective(self, origin, target, up, fov_x_deg, near=1e-2, far=1e4):
        cam = A.phip_camera()
        cam.to_world[:] = look_at(origin, target, up).reshape(-1).tolist()
        cam.xfov_deg = fov_x_deg
        cam.near_clip = near
        cam.far_clip = far
        self.camera = cam

    def hdrfilm(self, width, height, filter_table, crop=None):
        """filter_table = (radius, [32 floats]) from a ReconstructionFilter provider."""
        f = A.phip_film()
        f.width, f.height = width, height
        if crop is None:
            crop = (0, 0, width, height)
        f.crop_offset_x, f.crop_offset_y, f.crop_width, f.crop_height = crop
        f.filter_radius = filter_table[0]
        f.filter_table[:] = list(filter_table[1])
        self.film = f

    # ---- flatten -----------------------------------------------------------------------
    def desc(self):
        d = A.phip_scene_desc()
        d.abi_version = A.PHIP_ABI_VERSION
        pos = np.concatenate(self.positions).astype(np.float32) if self.positions else np.zeros((0, 3), np.float32)
        any_normals = any(n is not None for n in self.normals)
        nrm = None
        if any_normals:
            nrm = np.concatenate([n if n is not None else np.zeros_like(p) for n, p in zip(self.normals, self.positions)]).astype(np.float32)
        idx, shapes = [], (A.phip_shape * max(1, len(self.shapes)))()
        v0 = t0 = 0
        for i, (p, t, s) in enumerate(zip(self.positions, self.indices, self.shapes)):
            idx.append(t + np.uint32(v0))
            sh = shapes[i]
            sh.first_vertex, sh.n_vertices = v0, len(p)
            sh.first_triangle, sh.n_triangles = t0, len(t)
            sh.material, sh.emitter = s["material"], s["emitter"]
            sh.has_normals = 1 if self.normals[i] is not None else 0
            sh.has_texcoords = 1 if self.uvs[i] is not None else 0
            v0 += len(p)
            t0 += len(t)
        idx = np.ascontiguousarray(np.concatenate(idx), dtype=np.uint32) if idx else np.zeros((0, 3), np.uint32)
        pos = np.ascontiguousarray(pos)
        mats = (A.phip_material * max(1, len(self.materials)))(*self.materials)
        ems = (A.phip_emitter * max(1, len(self.emitters)))()
        for i, e in enumerate(self.emitters):
            ems[i].radiance[:] = e["radiance"]
            ems[i].sampling_weight = e["weight"]
            ems[i].shape = e["shape"]
            ems[i].type = e.get("type", A.PHIP_EMITTER_AREA)
        d.n_vertices = len(pos)
        d.positions = pos.ctypes.data_as(C.POINTER(C.c_float))
        d.normals = nrm.ctypes.data_as(C.POINTER(C.c_float)) if nrm is not None else None
        d.n_triangles = len(idx)
        d.indices = idx.ctypes.data_as(C.POINTER(C.c_uint32))
        d.n_shapes, d.shapes = len(self.shapes), shapes
        d.n_materials, d.materials = len(self.materials), mats
        d.n_emitters, d.emitters = len(self.emitters), ems
        d.camera, d.film = self.camera, self.film
        tcs = None
        if any(u is not None for u in self.uvs):
            tcs = np.ascontiguousarray(np.concatenate([u if u is not None else np.zeros((len(p), 2), np.float32) for u, p in zip(self.uvs, self.positions)]), np.float32)
            d.texcoords = tcs.ctypes.data_as(C.POINTER(C.c_float))
        texs = (A.phip_texture * max(1, len(self.textures)))()
        for i, t in enumerate(self.textures):
            lv = t["levels"]
            texs[i].height, texs[i].width = lv[0].shape[0], lv[0].shape[1]
            texs[i].n_levels = len(lv)
            for j, l in enumerate(lv):
                texs[i].levels[j] = l.ctypes.data_as(C.POINTER(C.c_float))
            texs[i].wrap_u, texs[i].wrap_v, texs[i].filter_type, texs[i].max_anisotropy = t["wrap_u"], t["wrap_v"], t["filter"], t["aniso"]
            texs[i].uv_scale[:] = t["scale"]; texs[i].uv_offset[:] = t["offset"]
        d.n_textures, d.textures = len(self.textures), texs
        env = getattr(self, "_envmap", None)
        if env is not None:
            t, scale, m, levels = env
            d.envmap.n_levels = len(levels)
            for i, l in enumerate(levels):
                d.envmap.levels[i] = l.ctypes.data_as(C.POINTER(C.c_float))
            d.envmap.texels = t.ctypes.data_as(C.POINTER(C.c_float))
            d.envmap.height, d.envmap.width = t.shape[0], t.shape[1]
            d.envmap.scale = scale
            d.envmap.to_world[:] = [float(v) for v in m.reshape(-1)]
        d._keep = (pos, nrm, idx, shapes, mats, ems, env, tcs, texs, [t["levels"] for t in self.textures])   # keep the buffers alive with the struct
        return d

    # ---- a second frame of the same topology (Scene.update) ---------------------------------
    def flat_positions(self):
        """the vertex positions of every mesh in the order of desc(): move a mesh (`sb.positions[shape_id]`) or the camera (`perspective`), then pass this to
        Scene.update -- or build desc() again for the scene a fresh creation makes of the same arrays"""
        return np.ascontiguousarray(np.concatenate(self.positions), dtype=np.float32) if self.positions else np.zeros((0, 3), np.float32)

    def flat_normals(self):
        """the vertex normals in the order of desc() (zeros for meshes without), or None if no mesh has any"""
        if not any(n is not None for n in self.normals):
            return None
        return np.ascontiguousarray(np.concatenate([n if n is not None else np.zeros_like(p) for n, p in zip(self.normals, self.positions)]), dtype=np.float32)

    @property
    def n_triangles(self):
        return sum(len(t) for t in self.indices)


def _rgb(v):
    if np.isscalar(v):
        return [float(v)] * 3
    v = list(v)
    assert len(v) == 3
    return [float(x) for x in v]


# ==========================================================================================
#  C1 / C2: the Cornell box (classic measured data, units of mm)
# ==========================================================================================
def cornell_box(width, height, filter_table, light_scale=1.0, sb=None, short_bsdf=None, tall_bsdf=None, extra_blocks=0):
    """short_bsdf / tall_bsdf: callables sb -> material id for the two blocks (default: the white diffuse of the room);
    extra_blocks: further small white blocks on the floor in front of the two (10 triangles each)"""
    sb = sb or SceneBuilder()
    white = sb.diffuse((0.725, 0.71, 0.68))
    red = sb.diffuse((0.63, 0.065, 0.05))
    green = sb.diffuse((0.14, 0.45, 0.091))
    light_bsdf = sb.diffuse((0.78, 0.78, 0.78))

    # room (normals face inward)
    sb.quad((552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2), white, facing=(0, 1, 0))            # floor
    sb.quad((556.0, 548.8, 0), (556.0, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0), white, facing=(0, -1, 0))  # ceiling
    sb.quad((549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556.0, 548.8, 559.2), white, facing=(0, 0, -1))  # back
    sb.quad((0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2), green, facing=(1, 0, 0))             # right (x=0)
    sb.quad((552.8, 0, 0), (549.6, 0, 559.2), (556.0, 548.8, 559.2), (556.0, 548.8, 0), red, facing=(-1, 0, 0))    # left
    # area light just below the ceiling
    sb.quad((343.0, 548.7, 227.0), (343.0, 548.7, 332.0), (213.0, 548.7, 332.0), (213.0, 548.7, 227.0), light_bsdf,
            facing=(0, -1, 0), radiance=tuple(light_scale * c for c in (17.0, 12.0, 4.0)))

    def box(top, h, white=white):
        """top: 4 corner (x,z) pairs of the top face, counter-clockwise seen from above"""
        top = [np.array([x, h, z], np.float32) for x, z in top]
        bot = [np.array([p[0], 0.0, p[2]], np.float32) for p in top]
        c = sum(top) / 4.0
        cx = np.array([c[0], h / 2.0, c[2]], np.float32)
        sb.quad(top[0], top[1], top[2], top[3], white, facing=(0, 1, 0))
        for i in range(4):
            j = (i + 1) % 4
            mid = (top[i] + top[j] + bot[i] + bot[j]) / 4.0
            sb.quad(top[i], bot[i], bot[j], top[j], white, facing=mid - cx)

    box([(130.0, 65.0), (82.0, 225.0), (240.0, 272.0), (290.0, 114.0)], 165.0, short_bsdf(sb) if short_bsdf else white)     # short box
    box([(423.0, 247.0), (265.0, 296.0), (314.0, 456.0), (472.0, 406.0)], 330.0, tall_bsdf(sb) if tall_bsdf else white)   # tall box
    for i in range(extra_blocks):                                                    # (33..64-record scenes: VERDICT r4 item 3b)
        x0, z0, s_, h_ = 330.0 + 70.0 * (i % 3), 40.0 + 75.0 * (i // 3), 50.0, 60.0 + 25.0 * i
        box([(x0 + s_, z0), (x0, z0 + 0.3 * s_), (x0 + 0.3 * s_, z0 + 1.3 * s_), (x0 + 1.3 * s_, z0 + s_)], h_)

    sb.perspective(origin=(278.0, 273.0, -800.0), target=(278.0, 273.0, -799.0), up=(0, 1, 0),
                   fov_x_deg=39.3077, near=10.0, far=2800.0)
    sb.hdrfilm(width, height, filter_table)
    return sb


def cornell_mixed(width, height, filter_table, light_scale=1.0, sb=None):
    """The Cornell box of C2 with one block of rough copper (two-sided, Beckmann alpha 0.1) and one of glass (bk7): the same 32
    triangles, all three leaf BSDF models of the path -- the small scene that is NOT the benchmark."""
    return cornell_box(width, height, filter_table, light_scale, sb,
                       short_bsdf=lambda b: b.twosided(b.roughconductor(CU_ETA, CU_K, alpha=0.1)),
                       tall_bsdf=lambda b: b.dielectric())


def cornell_spheres(width, height, filter_table, nlon=24, nlat=12, materials=True, sb=None):
    """The Cornell box with a glass and a rough-copper sphere (`materials=False`: two diffuse spheres), tessellated nlon x nlat: 32 + 2 * 2 * nlon * (nlat - 1)
    triangles -- the mid-sized scenes between the LDS-resident boxes and the atrium (1 k / 4.5 k / 18 k triangles at 24 x 12 / 48 x 24 / 96 x 48): the wavefront
    kernels on a tree that lives in L2."""
    sb = cornell_box(width, height, filter_table, sb=sb)
    P, T, N = sphere_mesh((185, 120, 170), 70.0, nlon, nlat)
    sb.mesh(P, T, sb.dielectric(1.5, 1.0) if materials else sb.diffuse((0.6, 0.6, 0.6)), normals=N)
    P, T, N = sphere_mesh((370, 330, 350), 60.0, nlon, nlat)
    sb.mesh(P, T, sb.twosided(sb.roughconductor(CU_ETA, CU_K, alpha=0.15)) if materials else sb.diffuse((0.7, 0.5, 0.3)), normals=N)
    return sb


# ==========================================================================================
#  procedural meshes
# ==========================================================================================
def _grid_mesh(P, nu, nv, closed_u=False):
    """(nu x nv) vertex grid -> triangles; P has shape (nv, nu, 3)"""
    P = _f32(P).reshape(nv, nu, 3)
    idx = np.arange(nu * nv, dtype=np.uint32).reshape(nv, nu)
    cols = nu if closed_u else nu - 1
    i0 = idx[:-1, :cols]
    i1 = np.roll(idx, -1, axis=1)[:-1, :cols]
    i2 = np.roll(idx, -1, axis=1)[1:, :cols]
    i3 = idx[1:, :cols]
    tris = np.concatenate([np.stack([i0, i1, i2], -1).reshape(-1, 3), np.stack([i2, i3, i0], -1).reshape(-1, 3)])
    return P.reshape(-1, 3), tris.astype(np.uint32)


def _smooth_normals(P, T):
    """area-weighted vertex normals (only used to give generated meshes a shading normal)"""
    P64 = P.astype(np.float64)
    fn = np.cross(P64[T[:, 1]] - P64[T[:, 0]], P64[T[:, 2]] - P64[T[:, 0]])
    N = np.zeros_like(P64)
    for k in range(3):
        np.add.at(N, T[:, k], fn)
    ln = np.linalg.norm(N, axis=1, keepdims=True)
    N = np.where(ln > 0, N / np.maximum(ln, 1e-30), np.array([0.0, 1.0, 0.0]))
    return N.astype(np.float32)


def cylinder_mesh(center, radius, y0, y1, nseg, nring, flute=0.0, nflutes=12):
    th = np.linspace(0, 2 * np.pi, nseg, endpoint=False)
    ys = np.linspace(y0, y1, nring + 1)
    r = radius * (1.0 - flute * (0.5 + 0.5 * np.cos(nflutes * th)))
    P = np.zeros((nring + 1, nseg, 3))
    P[..., 0] = center[0] + r[None, :] * np.cos(th)[None, :]
    P[..., 2] = center[1] + r[None, :] * np.sin(th)[None, :]
    P[..., 1] = ys[:, None]
    return _grid_mesh(P, nseg, nring + 1, closed_u=True)


def sphere_mesh(center, radius, nlon, nlat):
    th = np.linspace(0, 2 * np.pi, nlon, endpoint=False)
    ph = np.linspace(0, np.pi, nlat + 1)[1:-1]
    P = np.zeros((nlat - 1, nlon, 3))
    P[..., 0] = np.sin(ph)[:, None] * np.cos(th)[None, :]
    P[..., 1] = np.cos(ph)[:, None]
    P[..., 2] = np.sin(ph)[:, None] * np.sin(th)[None, :]
    V, T = _grid_mesh(P, nlon, nlat - 1, closed_u=True)
    n = len(V)
    V = np.concatenate([V, [[0, 1, 0], [0, -1, 0]]]).astype(np.float32)
    top = np.stack([np.full(nlon, n), (np.arange(nlon) + 1) % nlon, np.arange(nlon)], -1)
    base = (nlat - 2) * nlon
    bot = np.stack([np.full(nlon, n + 1), base + np.arange(nlon), base + (np.arange(nlon) + 1) % nlon], -1)
    T = np.concatenate([T, top, bot]).astype(np.uint32)
    N = V.copy()
    return (V * radius + np.asarray(center, np.float32)).astype(np.float32), T, N.astype(np.float32)


def box_mesh(lo, hi):
    lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32)
    c = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], lo[2]],
                  [lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]], np.float32)
    q = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]   # outward facing
    T = []
    for a, b, cc, d in q:
        T += [[a, b, cc], [cc, d, a]]
    return c, np.array(T, np.uint32)


CU_ETA = (0.200438, 0.924033, 1.102212)     # copper, linear RGB (what the host derives from data/ior/Cu.eta.spd)
CU_K = (3.912949, 2.452848, 2.142188)


# ==========================================================================================
#  C3 / C5: "Sponza-class" procedural atrium, ~260k triangles
# ==========================================================================================
def atrium(width, height, filter_table, seed=1, detail=1.0, sb=None):
    """Two-storey colonnaded atrium: tessellated fluted columns, arches, a bumpy tiled floor and
    hanging cloth banners.  70 % of the objects are twosided diffuse (albedo ~ U[0.2,0.8]), 30 %
    roughconductor (Cu, beckmann alpha in {0.05, 0.1, 0.3}); one large ceiling area light plus a
    smaller 'skylight' quad.  detail scales the tessellation (1.0 -> ~260k triangles)."""
    rng = np.random.default_rng(seed)
    sb = sb or SceneBuilder()
    LX, LY, LZ = 36.0, 14.0, 16.0        # room size (x: long axis)

    def random_material():
        if rng.random() < 0.3:
            a = float(rng.choice([0.05, 0.1, 0.3]))
            return sb.twosided(sb.roughconductor(CU_ETA, CU_K, alpha=a))
        return sb.twosided(sb.diffuse(tuple(rng.uniform(0.2, 0.8, 3))))

    wall = sb.twosided(sb.diffuse((0.62, 0.58, 0.5)))
    # shell
    sb.quad((0, 0, 0), (LX, 0, 0), (LX, 0, LZ), (0, 0, LZ), wall, facing=(0, 1, 0))      # ground slab (under the tiles)
    sb.quad((0, LY, 0), (LX, LY, 0), (LX, LY, LZ), (0, LY, LZ), wall, facing=(0, -1, 0))
    sb.quad((0, 0, 0), (0, LY, 0), (0, LY, LZ), (0, 0, LZ), wall, facing=(1, 0, 0))
    sb.quad((LX, 0, 0), (LX, LY, 0), (LX, LY, LZ), (LX, 0, LZ), wall, facing=(-1, 0, 0))
    sb.quad((0, 0, 0), (LX, 0, 0), (LX, LY, 0), (0, LY, 0), wall, facing=(0, 0, 1))
    sb.quad((0, 0, LZ), (LX, 0, LZ), (LX, LY, LZ), (0, LY, LZ), wall, facing=(0, 0, -1))
    # lights
    sb.quad((8, LY - 0.05, 5.5), (28, LY - 0.05, 5.5), (28, LY - 0.05, 10.5), (8, LY - 0.05, 10.5), sb.diffuse((0.5, 0.5, 0.5)),
            facing=(0, -1, 0), radiance=(18.0, 16.5, 14.0))
    sb.quad((0.05, 8.0, 6.0), (0.05, 12.0, 6.0), (0.05, 12.0, 10.0), (0.05, 8.0, 10.0), sb.diffuse((0.5, 0.5, 0.5)),
            facing=(1, 0, 0), radiance=(6.0, 8.0, 12.0))

    # bumpy tiled floor: one mesh per 4x4 m tile
    n = max(2, int(round(24 * detail)))
    for ix in range(9):
        for iz in range(4):
            xs = np.linspace(ix * 4.0, ix * 4.0 + 3.9, n)
            zs = np.linspace(iz * 4.0, iz * 4.0 + 3.9, n)
            X, Z = np.meshgrid(xs, zs)
            Y = 0.02 + 0.015 * np.sin(3.1 * X + ix) * np.cos(2.7 * Z + iz) + 0.004 * rng.standard_normal(X.shape)
            P, T = _grid_mesh(np.stack([X, Y, Z], -1), n, n)
            T = T[:, [0, 2, 1]]            # face up
            sb.mesh(P, T, random_material(), normals=_smooth_normals(P, T))

    # two rows of fluted columns on two storeys + arches between them
    nseg = max(8, int(round(48 * detail))); nring = max(2, int(round(20 * detail)))
    xs_cols = np.linspace(3.0, LX - 3.0, 9)
    for storey, (y0, y1, rad) in enumerate([(0.0, 6.0, 0.45), (6.6, 11.5, 0.35)]):
        for zc in (3.5, LZ - 3.5):
            for xc in xs_cols:
                P, T = cylinder_mesh((xc, zc), rad, y0, y1, nseg, nring, flute=0.12, nflutes=12)
                sb.mesh(P, T, random_material(), normals=_smooth_normals(P, T))
            # arches: half tori between neighbouring columns
            na = max(6, int(round(28 * detail))); nt = max(6, int(round(14 * detail)))
            for xa, xb in zip(xs_cols[:-1], xs_cols[1:]):
                R = 0.5 * (xb - xa); cx = 0.5 * (xa + xb)
                u = np.linspace(0, np.pi, na + 1); v = np.linspace(0, 2 * np.pi, nt, endpoint=False)
                U, V = np.meshgrid(u, v, indexing="ij")
                r = 0.22
                X = cx + (R + r * np.cos(V)) * np.cos(U)
                Yc = y1 - R * 0.0 + (R + r * np.cos(V)) * np.sin(U) * 0.55
                Zc = zc + r * np.sin(V)
                P, T = _grid_mesh(np.stack([X, Yc, Zc], -1), nt, na + 1, closed_u=True)
                sb.mesh(P, T, random_material(), normals=_smooth_normals(P, T))
        # balcony slab of the storey.  Its end faces stop 3 cm short of the room shell: rounds 1-2 let them lie IN the wall planes, and
        # a ray that hit a wall behind a slab end found two triangles at exactly the same distance -- which of them an accelerator
        # reports is a property of its leaf order (the reference's kd-tree) or of a rule (path_hip: the highest index), so the generator's
        # own coincident panels, not the renderer, accounted for most of the 3.7e-4 that separated path_hip from Mitsuba on C3.
        g = 0.03
        for zlo, zhi in ((g, 4.2), (LZ - 4.2, LZ - g)):
            P, T = box_mesh((g, y1, zlo), (LX - g, y1 + 0.5, zhi))
            sb.mesh(P, T, wall)

    # hanging cloth banners (sinusoidal sheets)
    nc = max(8, int(round(96 * detail)))
    for i, xc in enumerate(np.linspace(6.0, LX - 6.0, 6)):
        u = np.linspace(-1.4, 1.4, nc); v = np.linspace(0.0, 5.5, nc)
        U, V = np.meshgrid(u, v)
        X = xc + 0.25 * np.sin(2.2 * V + i) * (V / 5.5)
        Y = 12.5 - V
        Z = LZ / 2 + U + 0.12 * np.sin(4.0 * U + 1.7 * V + i)
        P, T = _grid_mesh(np.stack([X, Y, Z], -1), nc, nc)
        sb.mesh(P, T, random_material(), normals=_smooth_normals(P, T))

    # clutter: spheres and boxes on the floor
    nl = max(8, int(round(40 * detail)))
    for i in range(14):
        c = (rng.uniform(4, LX - 4), 0.0, rng.uniform(5.5, LZ - 5.5))
        if i % 2 == 0:
            rad = rng.uniform(0.35, 0.8)
            P, T, N = sphere_mesh((c[0], rad + 0.05, c[2]), rad, nl, nl // 2)
            sb.mesh(P, T, random_material(), normals=N)
        else:
            s = rng.uniform(0.4, 0.9, 3)
            P, T = box_mesh((c[0] - s[0], 0.05, c[2] - s[2]), (c[0] + s[0], 0.05 + 2 * s[1], c[2] + s[2]))
            sb.mesh(P, T, random_material())

    sb.perspective(origin=(2.5, 4.2, LZ / 2 + 0.8), target=(LX - 4.0, 5.2, LZ / 2 - 0.4), up=(0, 1, 0), fov_x_deg=70.0, near=0.05, far=200.0)
    sb.hdrfilm(width, height, filter_table)
    return sb


# ==========================================================================================
#  C4: glass-heavy room, ~150k triangles
# ==========================================================================================
def glass_room(width, height, filter_table, seed=2, detail=1.0, sb=None):
    """Tiled box room with tessellated glass spheres and slabs (dielectric, intIOR 1.5) on a table,
    two quad area lights.  Long specular chains: NEE is skipped on the delta surfaces (path.cpp:174-175)."""
    rng = np.random.default_rng(seed)
    sb = sb or SceneBuilder()
    LX, LY, LZ = 8.0, 4.0, 6.0
    tiles = [sb.diffuse(c) for c in [(0.75, 0.75, 0.72), (0.35, 0.45, 0.6), (0.7, 0.55, 0.4)]]
    white = sb.diffuse((0.8, 0.8, 0.8))
    glass = sb.dielectric(1.5, 1.0)

    def tiled_wall(origin, du, dv, nu, nv, facing):
        o = np.asarray(origin, np.float32); du = np.asarray(du, np.float32); dv = np.asarray(dv, np.float32)
        for m in range(len(tiles)):
            Ps, Ts = [], []
            cnt = 0
            for i in range(nu):
                for j in range(nv):
                    if (i * 7 + j * 3 + (i * j) % 2) % len(tiles) != m:
                        continue
                    p0 = o + du * (i / nu) + dv * (j / nv); p1 = o + du * ((i + 1) / nu) + dv * (j / nv)
                    p2 = o + du * ((i + 1) / nu) + dv * ((j + 1) / nv); p3 = o + du * (i / nu) + dv * ((j + 1) / nv)
                    quad = np.stack([p0, p1, p2, p3])
                    nrm = np.cross(quad[1] - quad[0], quad[2] - quad[0])
                    if np.dot(nrm, facing) < 0:
                        quad = quad[::-1]
                    Ps.append(quad); Ts.append(np.array([[0, 1, 2], [2, 3, 0]], np.uint32) + 4 * cnt); cnt += 1
            if Ps:
                sb.mesh(np.concatenate(Ps), np.concatenate(Ts), tiles[m])

    nt = max(2, int(round(24 * detail)))
    tiled_wall((0, 0, 0), (LX, 0, 0), (0, 0, LZ), nt, nt, (0, 1, 0))
    tiled_wall((0, LY, 0), (LX, 0, 0), (0, 0, LZ), nt // 2, nt // 2, (0, -1, 0))
    tiled_wall((0, 0, 0), (0, LY, 0), (0, 0, LZ), nt // 2, nt, (1, 0, 0))
    tiled_wall((LX, 0, 0), (0, LY, 0), (0, 0, LZ), nt // 2, nt, (-1, 0, 0))
    tiled_wall((0, 0, LZ), (LX, 0, 0), (0, LY, 0), nt, nt // 2, (0, 0, -1))
    tiled_wall((0, 0, 0), (LX, 0, 0), (0, LY, 0), nt, nt // 2, (0, 0, 1))
    # lights
    sb.quad((2.0, LY - 0.02, 2.0), (3.6, LY - 0.02, 2.0), (3.6, LY - 0.02, 3.6), (2.0, LY - 0.02, 3.6), sb.diffuse((0.5, 0.5, 0.5)),
            facing=(0, -1, 0), radiance=(30.0, 28.0, 24.0))
    sb.quad((5.2, LY - 0.02, 3.0), (6.4, LY - 0.02, 3.0), (6.4, LY - 0.02, 4.4), (5.2, LY - 0.02, 4.4), sb.diffuse((0.5, 0.5, 0.5)),
            facing=(0, -1, 0), radiance=(14.0, 18.0, 26.0))
    # table
    P, T = box_mesh((1.5, 0.9, 1.5), (6.5, 1.0, 4.8)); sb.mesh(P, T, white)
    for x, z in [(1.7, 1.7), (6.3, 1.7), (1.7, 4.6), (6.3, 4.6)]:
        P, T = box_mesh((x - 0.06, 0.0, z - 0.06), (x + 0.06, 0.9, z + 0.06)); sb.mesh(P, T, white)
    # glass spheres on the table and floor
    nl = max(8, int(round(80 * detail)))
    for i in range(24):
        r = float(rng.uniform(0.12, 0.32))
        if i < 16:
            c = (rng.uniform(1.9, 6.1), 1.0 + r + 0.002, rng.uniform(1.9, 4.4))
        else:
            c = (rng.uniform(0.8, 7.2), r + 0.002, rng.uniform(0.6, 1.2) if i % 2 else rng.uniform(5.0, 5.6))
        P, T, N = sphere_mesh(c, r, nl, nl // 2)
        sb.mesh(P, T, glass, normals=N)
    # glass slabs
    for i in range(6):
        x = 2.0 + 0.75 * i
        P, T = box_mesh((x, 1.002, 2.6 + 0.1 * (i % 2)), (x + 0.08, 1.9 + 0.1 * i, 3.6 + 0.1 * (i % 2)))
        sb.mesh(P, T, glass)
    sb.perspective(origin=(0.9, 2.2, 0.5), target=(4.6, 1.2, 3.4), up=(0, 1, 0), fov_x_deg=65.0, near=0.02, far=100.0)
    sb.hdrfilm(width, height, filter_table)
    return sb

"""Host-side mirror of the reference's integrator plugin interface for the `path` hot path.

Names, parameter meaning and error behaviour follow the reference so that tests read like the
reference's own:

    PathHIP(props)           <-> MIPathTracer(const Properties &)           src/integrators/path/path.cpp:109-111
      maxDepth / rrDepth / strictNormals / hideEmitters                      src/librender/integrator.cpp:190-225
    PathHIP.render(scene)    <-> SamplingIntegrator::render(scene, queue, job, ...) -> bool   integrator.cpp:95-129
    PathHIP.cancel()         <-> SamplingIntegrator::cancel                  integrator.cpp:90-93
    DirectHIP(props)         <-> MIDirectIntegrator(const Properties &)      src/integrators/direct/direct.cpp:91-108
      shadingSamples / emitterSamples / bsdfSamples / strictNormals / hideEmitters
    Scene(desc)              <-> Scene::initialize (kd-tree build -> BVH build + upload)       scene.cpp:322-384
    HDRFilm.put / develop    <-> HDRFilm::put(const ImageBlock *) / develop  films/hdrfilm.cpp:391-393,427-475

Everything below the C ABI runs on the GPU; this module only marshals arguments.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from . import _ffi


def _ptr(t):
    """the address of a tensor for a descriptor; None (NULL) for an output not asked for or an input not given"""
    return t.data_ptr() if t is not None else None


def _stream_handle(stream):
    """the hipStream_t of a torch.cuda.Stream, or the raw handle (or None) as given"""
    return getattr(stream, "cuda_stream", stream)


def _check(rc, name):
    if rc != 0:
        raise _ffi.PhipError(rc, name)


class Properties(dict):
    """Minimal typed property bag (include/mitsuba/core/properties.h)."""

    def __init__(self, plugin_name="", **kw):
        super().__init__(**kw)
        self.plugin_name = plugin_name

    def getInteger(self, name, default):
        return int(self.get(name, default))

    def getBoolean(self, name, default):
        return bool(self.get(name, default))

    def getSize(self, name, default):
        v = int(self.get(name, default))
        if v < 0:
            raise RuntimeError("Size property '%s': expected a nonnegative value!" % name)     # properties.cpp getSize
        return v


class Scene:
    """Device-resident scene: flattened meshes + BVH + emitter tables (phip_scene)."""

    def __init__(self, desc, device=0):
        self._L = _ffi.lib()
        self.desc = desc
        self.device = device
        self._h = self._L.phip_scene_create(C.byref(desc), device)
        if not self._h:
            raise RuntimeError("phip_scene_create: " + _ffi.last_error())
        self.width, self.height = desc.film.crop_width, desc.film.crop_height
        self.block_size = 32          # Scene::getBlockSize default (mitsuba.cpp:144)

    def setBlockSize(self, bs):
        self.block_size = int(bs)

    def accel_info(self):
        info = A.phip_accel_info()
        _check(self._L.phip_scene_accel_info(self._h, C.byref(info)), "phip_scene_accel_info")
        return info

    def rayIntersect(self, rays, closest=True, shadow=False):
        """Batch version of ShapeKDTree::rayIntersect(ray, its) / (ray).  rays: (n,8) float32 = o, mint, d, maxt."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(r)
        hits = np.zeros((n, 4), np.float32) if closest else None
        occ = np.zeros(n, np.uint8) if shadow else None
        st = A.phip_stats()
        _check(self._L.phip_trace(self._h, r.ctypes.data_as(C.POINTER(A.phip_ray)), n,
                                  hits.ctypes.data_as(C.POINTER(A.phip_hit)) if closest else None,
                                  occ.ctypes.data_as(C.POINTER(C.c_uint8)) if shadow else None, C.byref(st)), "phip_trace")
        return hits, occ, st

    def rayIntersectDevice(self, rays, closest=True, shadow=False, surfaces=False, stream=None):
        """rayIntersect on device memory (phip_trace_device): rays is a contiguous float32 torch tensor of shape (n, 8) = o, mint, d, maxt on the scene's device, read in
        place; `stream` is the stream its producer ran on (a torch.cuda.Stream or a raw handle), the cast is ordered after it.  Returns (hits, occluded, surfaces, stats):
        torch tensors on the same device -- (n, 4) float32 (t, u, v, bits of prim), (n,) uint8, (n, 16) float32 (the words of phip_surface) -- or None where not asked for.
        stats.trace_kernel_ms is the ray kernel's HIP-event time, stats.shade_kernel_ms that of the surface records' kernel.
        The rays must be finite.  ValueError for a tensor of another dtype, layout or device; PhipError for what the library refuses (surfaces without closest)."""
        import torch
        rays = Scene._device_tensor(self, rays, "rays", 8)
        n = rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.float32, device=rays.device) if closest else None
        occ = torch.empty((n,), dtype=torch.uint8, device=rays.device) if shadow else None
        surf = torch.empty((n, 16), dtype=torch.float32, device=rays.device) if surfaces else None
        st = A.phip_stats()
        rc = self._L.phip_trace_device(self._h, _ptr(rays), n, _ptr(hits), _ptr(occ), _ptr(surf), _stream_handle(stream), C.byref(st))
        _check(rc, "phip_trace_device")
        return hits, occ, surf, st

    def _sensor_params(self, spp, seed, sample_offset, block_size, flags, stream):
        return A.default_render_params(spp=spp, seed=seed, sample_offset=sample_offset, block_size=block_size or self.block_size, device=self.device, flags=flags,
                                       stream=_stream_handle(stream))

    def camera_rays(self, spp, seed=0, sample_offset=0, pixels=None, keys=True, positions=False, stream=None):
        """The camera samples a render traces, on the device (phip_camera_rays_device): for every pixel of the crop window in row-major order -- or for the pixels
        of `pixels`, a contiguous int32 / uint32 tensor of crop-pixel indices (y * width + x) on the scene's device -- and k in [0, spp), sample sample_offset + k
        of the counter stream.  Returns (rays, keys, positions): torch tensors on the scene's device with one row per sample, pixel-major -- (n, 8) float32 = o, mint,
        d, maxt as rayIntersectDevice and PathHIP.radiance read them; (n, 2) int32 (pixel, sample), the `pairs` of PathHIP.radiance; (n, 2) float32, the sample's
        position on the film in crop coordinates -- or None where not asked for.  ValueError for a tensor of another dtype, layout or device; PhipError for what
        the library refuses (an index outside the crop window: nothing is written)."""
        import torch
        dev = torch.device("cuda", self.device)
        pixels = Scene._device_tensor(self, pixels, "pixels", dtype=(torch.int32, torch.uint32), rows="m", optional=True)
        m = self.width * self.height if pixels is None else pixels.shape[0]
        n = m * spp
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        k = torch.empty((n, 2), dtype=torch.int32, device=dev) if keys else None
        pos = torch.empty((n, 2), dtype=torch.float32, device=dev) if positions else None
        if n == 0:                                  # an empty list: nothing to ask the library for
            return rays, k, pos
        d = A.phip_camera_rays_desc(d_pixels=_ptr(pixels), m=m, d_rays=_ptr(rays), d_keys=_ptr(k), d_positions=_ptr(pos))
        p = self._sensor_params(spp, seed, sample_offset, None, 0, stream)
        _check(self._L.phip_camera_rays_device(self._h, C.byref(p), C.byref(d)), "phip_camera_rays_device")
        return rays, k, pos

    def film(self, values, spp, seed=0, sample_offset=0, signed=False, out=None, accumulate=False, block_size=None, flags=0, stream=None):
        """ImageBlock::put on the caller's per-sample values (phip_film_device): values is a contiguous float32 torch tensor of height * width * spp x 4 entries in
        [y][x][k] order (camera_rays' order) on the scene's device; the result is the (height, width, 5) float32 film -- four filtered sums and the weight -- a
        render would leave had its samples carried these values, at the samples' own positions.  signed: reject only non-finite samples (normals, signed
        fields), not negative ones.  out: the film tensor to write (accumulate=True: to add to).  Returns (film, stats)."""
        import torch
        n = self.width * self.height * spp
        if not hasattr(values, "data_ptr") or values.dtype != torch.float32 or not values.is_contiguous() or values.numel() != 4 * n or values.shape[-1] != 4:
            raise ValueError("values: expected a contiguous float32 tensor of height * width * spp x 4 values")
        if not values.is_cuda or (values.device.index or 0) != self.device:
            raise ValueError("values: the tensor is not on the scene's device")
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs the film to add to (out=)")
            out = torch.empty((self.height, self.width, 5), dtype=torch.float32, device=values.device)
        elif not hasattr(out, "data_ptr") or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (self.height, self.width, 5) or out.device != values.device:
            raise ValueError("out: expected a contiguous float32 tensor of shape (height, width, 5) on the values' device")
        d = A.phip_film_desc(d_values=values.data_ptr(), d_out=out.data_ptr(), flags=A.PHIP_FILM_SIGNED if signed else 0, reserved=0)
        st = A.phip_stats()
        p = self._sensor_params(spp, seed, sample_offset, block_size, flags | (A.PHIP_FLAG_ACCUMULATE if accumulate else 0), stream)
        _check(self._L.phip_film_device(self._h, C.byref(p), C.byref(d), C.byref(st)), "phip_film_device")
        return out, st

    def _device_tensor(self, t, name, cols=None, dtype=None, rows=None, optional=False):
        """a contiguous tensor on the scene's device, as the calls on device memory read and write them: of shape (n, cols), or (n,) without `cols`; of `dtype`, one
        torch dtype or a tuple of those accepted (default float32).  rows: the row count it must have, or the letter the refusal has for a free one (default n)"""
        import torch
        if t is None and optional:
            return None
        dtypes = dtype if isinstance(dtype, tuple) else (dtype or torch.float32,)
        shape = (lambda: t.dim() == 1) if cols is None else (lambda: t.dim() == 2 and t.shape[1] == cols)
        if not hasattr(t, "data_ptr") or t.dtype not in dtypes or not t.is_contiguous() or not shape() or (isinstance(rows, int) and t.shape[0] != rows):
            raise ValueError("%s: expected a contiguous %s tensor of shape (%s%s" % (name, " or ".join(str(d).replace("torch.", "") for d in dtypes),
                                                                                      "n" if rows is None else rows, ",)" if cols is None else ", %d)" % cols))
        if not t.is_cuda or (t.device.index or 0) != self.device:
            raise ValueError("%s: the tensor is not on the scene's device" % name)
        return t

    def bsdf(self, rays, hits, wo=None, samples=None, local=False, wi_local=False, stream=None):
        """BSDF::eval / pdf / sample at the hits of a ray cast (phip_bsdf_device).  rays (n, 8) and hits (n, 4) are what rayIntersectDevice read and returned.
        wo: (n, 4) float32, xyz = the outgoing direction -> eval, (n, 4) = the BSDF's value (solid-angle measure, cosine included) and its pdf.
        samples: (n, 2) float32 in [0, 1) -> sampled, (n, 12) float32: the words of phip_bsdf_sample -- wo, pdf, weight = value / pdf, eta, flags (view as int32:
        PHIP_BSDF_SAMPLED_VALID | _DELTA), three reserved words; a failed sample is all zero.  local: wo is given, and the sampled direction returned, in the shading
        frame instead of world space.  wi_local: also return wi in the shading frame, (n, 4).  Returns (eval, sampled, wi_local), None where not asked for.
        A miss is all zero.  ValueError for a tensor of another dtype, layout or device; PhipError for what the library refuses (no output asked for)."""
        import torch
        rays = self._device_tensor(rays, "rays", 8)
        n = rays.shape[0]
        hits = self._device_tensor(hits, "hits", 4, rows=n)
        wo = self._device_tensor(wo, "wo", 4, rows=n, optional=True)
        samples = self._device_tensor(samples, "samples", 2, rows=n, optional=True)
        ev = torch.empty((n, 4), dtype=torch.float32, device=rays.device) if wo is not None else None
        sampled = torch.empty((n, 12), dtype=torch.float32, device=rays.device) if samples is not None else None
        wi = torch.empty((n, 4), dtype=torch.float32, device=rays.device) if wi_local else None
        d = A.phip_bsdf_desc(d_rays=_ptr(rays), d_hits=_ptr(hits), n=n, d_wo=_ptr(wo), d_samples=_ptr(samples), d_eval=_ptr(ev), d_sampled=_ptr(sampled), d_wi_local=_ptr(wi),
                             flags=A.PHIP_BSDF_LOCAL if local else 0, reserved=0, stream=_stream_handle(stream))
        _check(self._L.phip_bsdf_device(self._h, C.byref(d)), "phip_bsdf_device")
        return ev, sampled, wi

    def emitter_sample(self, ref, ref_n, samples, shadow_rays=False, stream=None):
        """Scene::sampleEmitterDirect without its visibility test (phip_emitter_sample_device).  ref: (n, 4) float32, xyz = the reference points; ref_n: (n, 4), their
        normals, or None (points on no surface); samples: (n, 2) in [0, 1).  Returns (sampled, rays): sampled (n, 12) float32, the words of phip_emitter_sample -- d,
        dist, value = radiance / pdf, pdf, emitter (view as int32; -1: no sample, all else 0), three reserved words; rays (n, 8), the shadow rays to hand to
        rayIntersectDevice(shadow=True) -- the empty interval where there is no sample --, or None."""
        import torch
        ref = self._device_tensor(ref, "ref", 4)
        n = ref.shape[0]
        ref_n = self._device_tensor(ref_n, "ref_n", 4, rows=n, optional=True)
        samples = self._device_tensor(samples, "samples", 2, rows=n)
        sampled = torch.empty((n, 12), dtype=torch.float32, device=ref.device)
        rays = torch.empty((n, 8), dtype=torch.float32, device=ref.device) if shadow_rays else None
        d = A.phip_emitter_sample_desc(d_ref=_ptr(ref), d_ref_n=_ptr(ref_n), d_samples=_ptr(samples), n=n, d_sampled=_ptr(sampled), d_shadow_rays=_ptr(rays),
                                       stream=_stream_handle(stream))
        _check(self._L.phip_emitter_sample_device(self._h, C.byref(d)), "phip_emitter_sample_device")
        return sampled, rays

    def emitter_eval(self, rays, hits, ref_n=None, emitter=False, stream=None):
        """The emitted radiance a ray meets and the density with which emitter sampling would have produced it (phip_emitter_eval_device): rays (n, 8), hits (n, 4)
        as for bsdf; ref_n (n, 4): the normals at the rays' origins, or None (zero).  Returns (eval, emitter): (n, 4) float32 = Le(-d) at a hit on an area emitter,
        the environment's radiance at a miss, else 0, and pdfEmitterDirect in the solid-angle measure; (n,) int32 emitter ids (-1: none) if emitter=True, else None."""
        import torch
        rays = self._device_tensor(rays, "rays", 8)
        n = rays.shape[0]
        hits = self._device_tensor(hits, "hits", 4, rows=n)
        ref_n = self._device_tensor(ref_n, "ref_n", 4, rows=n, optional=True)
        ev = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
        em = torch.empty((n,), dtype=torch.int32, device=rays.device) if emitter else None
        d = A.phip_emitter_eval_desc(d_rays=_ptr(rays), d_hits=_ptr(hits), d_ref_n=_ptr(ref_n), n=n, d_eval=_ptr(ev), d_emitter=_ptr(em), stream=_stream_handle(stream))
        _check(self._L.phip_emitter_eval_device(self._h, C.byref(d)), "phip_emitter_eval_device")
        return ev, em

    def replicate(self, devices):
        """Copies the device scene to further GPUs ahead of a multi-device render (phip_scene_replicate)."""
        arr = (C.c_int32 * len(devices))(*devices)
        _check(self._L.phip_scene_replicate(self._h, arr, len(devices)), "phip_scene_replicate")

    def update(self, positions=None, normals=None, camera=None, stream=None):
        """New vertex positions / normals / camera on the scene as created: a refit of the acceleration structure, not a rebuild (phip_scene_update).
        positions, normals: numpy arrays (host memory), or float32 contiguous torch tensors on the scene's device, whose data_ptr() the library reads in place
        (`stream`: the stream their producer ran on -- a torch.cuda.Stream or a raw handle; the update is ordered after it); shape n_vertices x 3 of the scene as
        created.  camera: a phip_camera.  Returns the phip_update_info (update_ms, kernel_ms, sah_cost, n_degenerate); PhipError on a refusal, the scene unchanged."""
        return self._new_vertices("phip_scene_update", positions, normals, camera, stream)

    def rebuild(self, positions=None, normals=None, camera=None, stream=None):
        """Scene.update with a new topology of the acceleration structure, built on the device from the positions where they are (phip_scene_rebuild): the remedy for
        a tree that refits have made slow (compare the sah_cost an update returns with accel_info().sah_cost of the creation).  Same arguments, same return value; with
        no arguments the tree is rebuilt on the scene's current vertices.  accel_info() may report other node, leaf and record counts afterwards."""
        return self._new_vertices("phip_scene_rebuild", positions, normals, camera, stream)

    def _new_vertices(self, entry, positions, normals, camera, stream):
        n = self.desc.n_vertices
        u = A.phip_update_desc()
        keep, on_device = [], []
        for name, a in (("positions", positions), ("normals", normals)):
            if a is None:
                continue
            if isinstance(a, np.ndarray) or not hasattr(a, "data_ptr"):
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.size != 3 * n:
                    raise ValueError("%s: expected %d x 3 values" % (name, n))
                setattr(u, name, a.ctypes.data)
                on_device.append(False)
            else:
                import torch
                if a.dtype != torch.float32 or not a.is_contiguous() or tuple(a.shape) != (n, 3):
                    raise ValueError("%s: expected a contiguous float32 tensor of shape (%d, 3)" % (name, n))
                if not a.is_cuda or (a.device.index or 0) != self.device:
                    raise ValueError("%s: the tensor is not on the scene's device" % name)
                setattr(u, name, a.data_ptr())
                on_device.append(True)
            keep.append(a)
        if len(set(on_device)) > 1:
            raise ValueError("positions and normals must both be host arrays or both be device tensors")
        u.device_pointers = 1 if on_device and on_device[0] else 0
        if stream is not None:
            u.stream = _stream_handle(stream)
        if camera is not None:
            u.camera = C.pointer(camera)
        info = A.phip_update_info()
        _check(getattr(self._L, entry)(self._h, C.byref(u), C.byref(info)), entry)
        if camera is not None:
            self.desc.camera = camera
        return info

    def vertex_normals(self, positions, out=None, stream=None, info=False):
        """The vertex normals of the scene's meshes at new positions as the reference's TriMesh::computeNormals makes them, on the scene's device
        (phip_vertex_normals_device; the host call of the same bits: scene.vertex_normals_angle_weighted).  positions: a contiguous (n_vertices, 3) float32 tensor
        on the scene's device; out: a tensor of the same kind to write into, or None (allocated); stream: the stream the positions' producer ran on.  Returns the
        normals -- what Scene.update(positions, normals) takes next --, with info=True also the phip_normals_info (n_invalid, kernel_ms)."""
        import torch
        n = self.desc.n_vertices
        positions = self._device_tensor(positions, "positions", 3, rows=n)
        out = torch.empty((n, 3), dtype=torch.float32, device=positions.device) if out is None else self._device_tensor(out, "out", 3, rows=n)
        d = A.phip_normals_desc(n_vertices=n, n_triangles=self.desc.n_triangles, indices=None, positions=_ptr(positions), normals=_ptr(out), stream=_stream_handle(stream))
        inf = A.phip_normals_info()
        _check(self._L.phip_vertex_normals_device(self._h, C.byref(d), C.byref(inf)), "phip_vertex_normals_device")
        return (out, inf) if info else out

    def mip_pyramid(self, level0, wrap_u="repeat", wrap_v=None, max_value=1.0, out=None, stream=None):
        """The MIP pyramid of a texture or an environment map as the reference's TMIPMap builds and stores it, on the scene's device (phip_mip_pyramid_device; the
        host call of the same bits: scene.mip_pyramid_lanczos).  level0: a contiguous (h, w, 3) float32 tensor on the scene's device.  wrap_u / wrap_v: "clamp",
        "repeat", "mirror", "zero", "one" or the PHIP_WRAP_* value (wrap_v defaults to wrap_u); max_value: 1 for a texture, infinity for an environment map
        (which takes repeat x clamp).  out: None, or one tensor per level to write into -- out[0] may be None (level 0 is not written) or level0 itself (rounded in
        place); without `out` every level is allocated, level 0 included.  stream: the stream level0's producer ran on.  Returns the list of levels, level 0
        first (None where out[0] was None): what update_appearance takes as "levels"."""
        import torch
        from .scene import WRAP_MODES, pyramid_sizes
        if not hasattr(level0, "data_ptr") or level0.dim() != 3 or level0.shape[2] != 3 or not level0.is_contiguous():
            raise ValueError("level0: expected a contiguous float32 tensor of shape (h, w, 3)")
        level0 = self._device_tensor(level0.view(-1), "level0").view(level0.shape)
        sizes = pyramid_sizes(level0.shape[1], level0.shape[0])
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.float32, device=level0.device) for h, w in sizes]
        if len(out) != len(sizes):
            raise ValueError("out: expected %d levels" % len(sizes))
        p = A.phip_pyramid_desc()
        p.width, p.height, p.n_levels = level0.shape[1], level0.shape[0], len(sizes)
        p.wrap_u = WRAP_MODES.get(wrap_u, wrap_u)
        p.wrap_v = p.wrap_u if wrap_v is None else WRAP_MODES.get(wrap_v, wrap_v)
        p.max_value = max_value
        p.d_level0 = _ptr(level0)
        for l, ((h, w), o) in enumerate(zip(sizes, out)):
            if o is None and l == 0:
                continue
            if o is None or o.numel() != 3 * h * w:
                raise ValueError("out[%d]: expected %d x %d x 3 values" % (l, h, w))
            p.d_levels[l] = _ptr(self._device_tensor(o.view(-1), "out[%d]" % l))
        p.stream = _stream_handle(stream)
        _check(self._L.phip_mip_pyramid_device(self._h, C.byref(p)), "phip_mip_pyramid_device")
        return list(out)

    def _levels_of(self, entry, n_levels, wrap_u, wrap_v, max_value, stream):
        """the "levels" of a texture or envmap dict of update_appearance: as given, or built from its "image" -- a device tensor on the device, an array on the host"""
        if "image" not in entry:
            return entry["levels"]
        from .scene import mip_pyramid_lanczos
        image = entry["image"]
        levels = self.mip_pyramid(image, wrap_u, wrap_v, max_value, stream=stream) if hasattr(image, "data_ptr") else mip_pyramid_lanczos(image, wrap_u, wrap_v, max_value)
        return levels[:max(1, n_levels)]

    def update_appearance(self, materials=None, emitters=None, textures=None, envmap=None, stream=None):
        """New materials, emitter radiances / sampling weights, texture contents and / or a new environment map on the scene as created, in place
        (phip_scene_update_appearance): afterwards the scene is the one a fresh creation with this look would have given.
        materials, emitters: sequences of phip_material / phip_emitter, one per material / emitter of the scene (emitter types and shapes stay).
        textures: one entry per texture of the scene -- None leaves it alone; else a dict as SceneBuilder keeps it: "levels" (the pyramid, (h, w, 3) float32 each,
        sizes as created) and optionally "wrap_u", "wrap_v", "filter", "aniso", "scale", "offset" (default: the creation's).
        envmap: a dict with "levels" (level 0 first), and optionally "scale" and "to_world" (4 x 4; default: the creation's).
        In place of "levels" a texture or envmap dict may carry "image", level 0 alone: the levels the scene was created with are then built as the reference
        builds them (mip_pyramid on the device for a tensor, scene.mip_pyramid_lanczos for an array) -- a texture with its own wrap modes and the bound 1, the
        environment map with repeat x clamp and no bound -- and passed on; a tensor never leaves the device.
        Texel arrays are numpy arrays (host memory) or contiguous float32 torch tensors on the scene's device, read in place (`stream`: the stream their producer
        ran on); a mix of both is refused.  Returns the phip_appearance_info as a dict; PhipError on a refusal, the scene unchanged."""
        d = self.desc
        a = A.phip_appearance_desc()
        keep, on_device = [], []

        def texels(x, h, w, what):
            if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
                x = np.ascontiguousarray(x, dtype=np.float32)
                if x.size != 3 * h * w:
                    raise ValueError("%s: expected %d x %d x 3 values" % (what, h, w))
                keep.append(x); on_device.append(False)
                return C.cast(x.ctypes.data, C.POINTER(C.c_float))
            import torch
            if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != 3 * h * w:
                raise ValueError("%s: expected a contiguous float32 tensor of %d x %d x 3 values" % (what, h, w))
            if not x.is_cuda or (x.device.index or 0) != self.device:
                raise ValueError("%s: the tensor is not on the scene's device" % what)
            keep.append(x); on_device.append(True)
            return C.cast(x.data_ptr(), C.POINTER(C.c_float))

        def level_sizes(w, h, n):
            out = [(h, w)]
            while len(out) < n:
                w, h = max(1, (w + 1) // 2), max(1, (h + 1) // 2)
                out.append((h, w))
            return out

        if materials is not None:
            arr = (A.phip_material * max(1, len(materials)))(*materials)
            a.n_materials, a.materials = len(materials), arr
            keep.append(arr)
        if emitters is not None:
            arr = (A.phip_emitter * max(1, len(emitters)))(*emitters)
            a.n_emitters, a.emitters = len(emitters), arr
            keep.append(arr)
        if textures is not None:
            arr = (A.phip_texture * max(1, len(textures)))()
            for i, t in enumerate(textures):
                if t is None or i >= d.n_textures:
                    continue                                      # width 0: this texture stays (a wrong count is the library's to refuse)
                old = d.textures[i]
                levels = self._levels_of(t, old.n_levels, t.get("wrap_u", old.wrap_u), t.get("wrap_v", old.wrap_v), 1.0, stream)
                arr[i].width, arr[i].height, arr[i].n_levels = old.width, old.height, len(levels)
                for l, (h, w) in enumerate(level_sizes(old.width, old.height, min(len(levels), A.PHIP_MIP_MAX_LEVELS))):
                    arr[i].levels[l] = texels(levels[l], h, w, "textures[%d] level %d" % (i, l))
                arr[i].wrap_u, arr[i].wrap_v = t.get("wrap_u", old.wrap_u), t.get("wrap_v", old.wrap_v)
                arr[i].filter_type, arr[i].max_anisotropy = t.get("filter", old.filter_type), t.get("aniso", old.max_anisotropy)
                arr[i].uv_scale[:] = t.get("scale", tuple(old.uv_scale)); arr[i].uv_offset[:] = t.get("offset", tuple(old.uv_offset))
            a.n_textures, a.textures = len(textures), arr
            keep.append(arr)
        if envmap is not None:
            e = A.phip_envmap()
            old = d.envmap
            levels = self._levels_of(envmap, old.n_levels, A.PHIP_WRAP_REPEAT, A.PHIP_WRAP_CLAMP, float("inf"), stream)
            e.width, e.height, e.n_levels = old.width, old.height, len(levels)
            for l, (h, w) in enumerate(level_sizes(old.width, old.height, min(len(levels), A.PHIP_ENVMAP_MAX_LEVELS))):
                e.levels[l] = texels(levels[l], h, w, "envmap level %d" % l)
            e.texels = e.levels[0]
            e.scale = envmap.get("scale", old.scale)
            e.to_world[:] = [float(v) for v in np.asarray(envmap["to_world"], np.float32).reshape(-1)] if "to_world" in envmap else list(old.to_world)
            a.envmap = C.pointer(e)
            keep.append(e)
        if len(set(on_device)) > 1:
            raise ValueError("texel arrays must all be host arrays or all be device tensors")
        a.device_pointers = 1 if on_device and on_device[0] else 0
        if stream is not None:
            a.stream = _stream_handle(stream)
        info = A.phip_appearance_info()
        rc = self._L.phip_scene_update_appearance(self._h, C.byref(a), C.byref(info))
        del keep                                                  # (held until the call has returned)
        _check(rc, "phip_scene_update_appearance")
        return info.as_dict()

    def film_to_host(self, d_ptr, host_ptr):
        """a device-resident frame (render_device's output, e.g. after an RCCL reduce) to host memory, as phip_render delivers it"""
        _check(self._L.phip_film_to_host(self._h, C.c_void_p(d_ptr), C.c_void_p(host_ptr)), "phip_film_to_host")

    def close(self):
        if getattr(self, "_h", None):
            self._L.phip_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HDRFilm:
    """Crop-sized (R,G,B,alpha,weight) float32 accumulation buffer, like HDRFilm's m_storage."""

    def __init__(self, width, height):
        self.storage = np.zeros((height, width, 5), np.float32)

    def clear(self):
        self.storage[...] = 0

    def put(self, block):
        self.storage += block

    def develop(self):
        h, w, _ = self.storage.shape
        out = np.zeros((h, w, 3), np.float32)
        _ffi.lib().phip_develop(_ffi.fptr(self.storage), h * w, _ffi.fptr(out))
        return out


class PinnedFilm(HDRFilm):
    """HDRFilm whose storage is page-locked (phip_host_alloc): PathHIP.render_into(scene, film.ptr, spp) receives the frame in one
    asynchronous device-to-host copy instead of the staged copy pageable memory needs."""

    def __init__(self, width, height):
        n = width * height * 5
        self._p = _ffi.lib().phip_host_alloc(n * 4)
        if not self._p:
            raise RuntimeError("phip_host_alloc: " + _ffi.last_error())
        self.ptr = self._p
        self.storage = np.ctypeslib.as_array(C.cast(C.c_void_p(self._p), C.POINTER(C.c_float)), shape=(height, width, 5))
        self.storage[...] = 0

    def close(self):
        if getattr(self, "_p", None):
            self.storage = None
            _ffi.lib().phip_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PathHIP:
    """`path_hip` integrator: MIPathTracer semantics, MI355X execution."""
    INTEGRATOR = A.PHIP_INTEGRATOR_PATH

    def __init__(self, props=None, **kw):
        props = Properties("path_hip", **(dict(props or {}) | kw))
        self.m_rrDepth = props.getInteger("rrDepth", 5)
        self.m_maxDepth = props.getInteger("maxDepth", -1)
        self.m_strictNormals = props.getBoolean("strictNormals", False)
        self.m_hideEmitters = props.getBoolean("hideEmitters", False)
        # integrator.cpp:219-224
        if self.m_rrDepth <= 0:
            raise RuntimeError("'rrDepth' must be set to a value greater than zero!")
        if self.m_maxDepth <= 0 and self.m_maxDepth != -1:
            raise RuntimeError("'maxDepth' must be set to -1 (infinite) or a value greater than zero!")
        self.stats = None
        self._scene = None

    def params(self, scene, spp, seed=0, shard_index=0, shard_count=1, flags=0, stream=None, **extra):
        """extra: devices=[...] (multi-GPU inside the call), sample_offset / sample_total (progressive passes), progress=callable"""
        p = A.default_render_params(spp=spp, max_depth=self.m_maxDepth, rr_depth=self.m_rrDepth,
                                    strict_normals=int(self.m_strictNormals), hide_emitters=int(self.m_hideEmitters),
                                    block_size=scene.block_size, seed=seed, shard_index=shard_index,
                                    shard_count=shard_count, device=scene.device, flags=flags, stream=stream, **extra)
        p.integrator = self.INTEGRATOR
        return p

    def _call(self, entry, scene, p, out):
        """One render entry point: keeps the call's statistics; False if cancelled, PhipError (Log(EError, ...) throws in the reference) on any other failure."""
        self._scene = scene
        st = A.phip_stats()
        rc = getattr(_ffi.lib(), entry)(scene._h, C.byref(p), out, C.byref(st))
        self.stats = st
        if rc == A.PHIP_ERR_CANCELLED:
            return False
        _check(rc, entry)
        return True

    def render(self, scene, film, spp, seed=0, shard_index=0, shard_count=1, flags=0, **extra):
        """Renders into `film` (film.put of one full-frame block).  Returns True on success,
        False if cancelled (SamplingIntegrator::render returns proc->getReturnStatus() == ESuccess)."""
        block = np.zeros((scene.height, scene.width, 5), np.float32)
        ok = self._call("phip_render", scene, self.params(scene, spp, seed, shard_index, shard_count, flags, **extra), _ffi.fptr(block))
        if ok:
            film.put(block)
        return ok

    def render_into(self, scene, host_ptr, spp, seed=0, shard_index=0, shard_count=1, flags=0, **extra):
        """phip_render into the caller's host memory (height x width x 5 float32 at address `host_ptr`): what the Mitsuba shim does with
        the film's bitmap.  Pinned memory (PinnedFilm below, torch pin_memory) gets the film in one asynchronous copy."""
        return self._call("phip_render", scene, self.params(scene, spp, seed, shard_index, shard_count, flags, **extra),
                          C.cast(C.c_void_p(host_ptr), C.POINTER(C.c_float)))

    def render_device(self, scene, d_out_ptr, spp, seed=0, shard_index=0, shard_count=1, flags=0, stream=None, **extra):
        """Renders this shard's blocks into device memory (e.g. a torch tensor) for an RCCL reduce."""
        return self._call("phip_render_device", scene, self.params(scene, spp, seed, shard_index, shard_count, flags, stream, **extra), C.c_void_p(d_out_ptr))

    def radiance(self, scene, rays, spp, seed=0, stream_ids=None, first_stream=0, flags=0, stream=None, pairs=None, **extra):
        """SamplingIntegrator::Li along the caller's rays (phip_radiance_device): rays is a contiguous float32 torch tensor of shape (n, 8) = o, mint, d, maxt on the
        scene's device, read in place; the result is an (n, 4) float32 tensor of (R, G, B, alpha) on the same device, the mean of spp samples per ray.  Ray i draws
        the counter stream of "pixel" stream_ids[i] (a contiguous int32 / uint32 tensor of n keys on the same device) or first_stream + i; extra: sample_offset,
        sample_total.  pairs (in place of stream_ids): a contiguous int32 / uint32 tensor of shape (n, 2) of (key, sample) -- Scene.camera_rays' keys --, sample k of
        ray i then draws the stream of (key, sample + k), and sample_offset must be 0: the camera samples of a whole render are one call at spp = 1.
        `stream` is the stream the rays' producer ran on (a torch.cuda.Stream or a raw handle).  The call's statistics are kept in self.stats.
        ValueError for a tensor of another dtype, layout or device; PhipError for what the library refuses; None if the call was cancelled."""
        import torch
        rays = Scene._device_tensor(scene, rays, "rays", 8)
        n = rays.shape[0]
        if stream_ids is not None:
            if not hasattr(stream_ids, "data_ptr") or stream_ids.dtype not in (torch.int32, torch.uint32) or not stream_ids.is_contiguous() or tuple(stream_ids.shape) != (n,):
                raise ValueError("stream_ids: expected a contiguous int32 or uint32 tensor of shape (n,)")
            if stream_ids.device != rays.device:
                raise ValueError("stream_ids: the tensor is not on the rays' device")
        if pairs is not None:
            if stream_ids is not None:
                raise ValueError("pairs and stream_ids are two layouts of one argument: pass one of them")
            if not hasattr(pairs, "data_ptr") or pairs.dtype not in (torch.int32, torch.uint32) or not pairs.is_contiguous() or tuple(pairs.shape) != (n, 2):
                raise ValueError("pairs: expected a contiguous int32 or uint32 tensor of shape (n, 2)")
            if pairs.device != rays.device:
                raise ValueError("pairs: the tensor is not on the rays' device")
            stream_ids = pairs
        out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
        p = self.params(scene, spp, seed, flags=flags, stream=_stream_handle(stream), **extra)
        d = A.phip_radiance_desc(d_rays=rays.data_ptr() if n else None, n=n, d_stream=stream_ids.data_ptr() if stream_ids is not None and n else None,
                                 first_stream=first_stream, reserved=A.PHIP_RADIANCE_STREAM_PAIRS if pairs is not None else 0, d_out=out.data_ptr() if n else None)
        return out if self._call("phip_radiance_device", scene, p, C.byref(d)) else None

    def samples(self, scene, spp):
        """Per-sample (R,G,B,alpha) of the last render made with PHIP_FLAG_SAMPLE_BUFFER: [y][x][sample]."""
        out = np.zeros((scene.height, scene.width, spp, 4), np.float32)
        _check(_ffi.lib().phip_get_samples(scene._h, _ffi.fptr(out), scene.height * scene.width * spp), "phip_get_samples")
        return out

    def cancel(self):
        if self._scene is not None:
            _ffi.lib().phip_cancel(self._scene._h)


class DirectHIP(PathHIP):
    """`direct_hip` integrator: MIDirectIntegrator semantics (direct.cpp:149-312) on the same kernels."""
    INTEGRATOR = A.PHIP_INTEGRATOR_DIRECT

    def __init__(self, props=None, **kw):
        props = Properties("direct_hip", **(dict(props or {}) | kw))
        # direct.cpp:94-107
        shadingSamples = props.getSize("shadingSamples", 1)
        self.m_emitterSamples = props.getSize("emitterSamples", shadingSamples)
        self.m_bsdfSamples = props.getSize("bsdfSamples", shadingSamples)
        self.m_strictNormals = props.getBoolean("strictNormals", False)
        self.m_hideEmitters = props.getBoolean("hideEmitters", False)
        if self.m_emitterSamples + self.m_bsdfSamples <= 0:
            raise RuntimeError("Assertion 'm_emitterSamples + m_bsdfSamples > 0' failed")
        self.m_rrDepth, self.m_maxDepth = 5, -1          # not parameters of this integrator
        self.stats = None
        self._scene = None

    def params(self, scene, spp, seed=0, shard_index=0, shard_count=1, flags=0, stream=None, **extra):
        p = super().params(scene, spp, seed, shard_index, shard_count, flags, stream, **extra)
        p.emitter_samples = self.m_emitterSamples
        p.bsdf_samples = self.m_bsdfSamples
        return p


class VolPathSimpleHIP(PathHIP):
    """`volpath_simple_hip` integrator: SimpleVolumetricPathTracer (src/integrators/path/volpath_simple.cpp:88-318) on a scene without participating media --
    the `path` loop without multiple importance sampling, same parameters (MonteCarloIntegrator: maxDepth, rrDepth, strictNormals, hideEmitters).  The scene
    description has no media; the Mitsuba plugin shim (mitsuba_amd/plugin/volpath_simple_hip.cpp) refuses a scene that has any."""
    INTEGRATOR = A.PHIP_INTEGRATOR_VOLPATH_SIMPLE

#!/usr/bin/env python3
"""phip_radiance_device on the procedural atrium's own primary rays against phip_render_device with PHIP_FLAG_NO_FUSED on the same samples, in one process on one
GPU.  One JSON line is appended to profiles/radiance_device.jsonl (DESIGN.md 3.15 quotes it).

    python tools/gpu_radiance.py [--mode radiance|render|both|parts] [--out profiles/radiance_device.jsonl] [--width 1920] [--height 1080] [--spp 4] [--reps 5] [--warmup 2]
                                 [--rays-file rays.npy] [--make-rays]

The rays are the camera rays of samples 0 .. spp - 1 of every pixel, made on the host by the twins of the device's stream and camera (phip_debug_host_ctr_block,
phip_debug_host_camera_ray) and keyed by their pixel index.  Making them is a Python loop over every pixel and sample and needs no GPU: --make-rays writes them to
--rays-file and exits, so that a job can do it in a step of its own; a later run loads the file.  Three lines, each quantity as [min, median, max] ms over --reps
repetitions after --warmup -- wall clock, and the HIP-event times of the vertex kernel, the ray kernel and the film pass / k_radiance_out (PHIP_FLAG_KERNEL_TIMING):
  render_device_no_fused     phip_render_device with PHIP_FLAG_NO_FUSED, spp samples per pixel
  radiance_device_per_sample the SAME samples: spp calls of phip_radiance_device with one sample each, call k on the camera rays of sample k at sample_offset k (a
                             repetition's figure is the sum over its spp calls, which are spp passes with a pool of a quarter of the ids each)
  radiance_device            one call with spp samples per ray on the camera rays of sample 0: the same streams, but the spp samples of a pixel share their first
                             segment, so their first hits are more coherent than the render's (a caller's usual call: a ray and its spp)
--mode render runs at a commit that has no phip_radiance_device.
--mode parts needs no ray file: the camera samples are made on the device by phip_camera_rays_device (the same bits, tests/test_gpu_camera_film.py).
Its lines, beside render_device_no_fused and radiance_device_per_sample measured again in the same process on the device-made rays:
  camera_rays_device         phip_camera_rays_device making the width x height x spp samples with their keys (wall clock only: one kernel and a synchronisation)
  radiance_device_pairs      ONE call of phip_radiance_device at spp = 1 with PHIP_RADIANCE_STREAM_PAIRS on those samples: the render's samples, one pool
  film_device                phip_film_device putting that call's output on the film: its kernel's HIP-event time stands beside the render's film_kernel_ms"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402  (before the library touches the GPU: tests/conftest.py)

if torch.cuda.is_available():     # (--make-rays runs without a GPU)
    torch.cuda.init()
from mitsuba_amd import _abi as A, _ffi, scene as S  # noqa: E402
from mitsuba_amd import integrator as I  # noqa: E402


def camera_rays(desc, w, h, spp):
    """(spp, h * w, 8) float32: the camera ray of sample k of every pixel, in pixel order"""
    L = _ffi.lib()
    rays = np.zeros((spp, h * w, 8), np.float32)
    buf = (C.c_float * 4)(); ray = A.phip_ray()
    for k in range(spp):
        for y in range(h):
            for x in range(w):
                L.phip_debug_host_ctr_block(y * w + x, k, 0, 0, buf)
                L.phip_debug_host_camera_ray(C.byref(desc.camera), C.byref(desc.film), np.float32(x) + buf[0], np.float32(y) + buf[1], C.byref(ray))
                rays[k, y * w + x] = list(ray.o) + [ray.mint] + list(ray.d) + [ray.maxt]
    return rays


def spread(v):
    return [float(np.min(v)), float(np.median(v)), float(np.max(v))]


def measure(calls, integ, reps, warmup):
    """calls: the calls of one repetition; its figures are their sums"""
    keys = ("shade_kernel_ms", "trace_kernel_ms", "film_kernel_ms")
    q = dict(wall_ms=[], shade_kernel_ms=[], trace_kernel_ms=[], film_kernel_ms=[])
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        wall = 0.0; acc = dict.fromkeys(keys + ("samples", "closest_rays", "iterations"), 0)
        for call in calls:
            t0 = time.perf_counter(); call(); wall += (time.perf_counter() - t0) * 1e3
            for k in acc:
                acc[k] += getattr(integ.stats, k)
        if i >= warmup:
            q["wall_ms"].append(wall)
            for k in keys:
                q[k].append(acc[k])
    out = {k: spread(v) for k, v in q.items()}
    out.update(samples=int(acc["samples"]), closest_rays=int(acc["closest_rays"]), iterations=int(acc["iterations"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="both", choices=("radiance", "render", "both", "parts"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "radiance_device.jsonl"))
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080); ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rays-file", default=None); ap.add_argument("--make-rays", action="store_true")
    args = ap.parse_args()
    w, h = args.width, args.height
    desc = S.atrium(w, h, _ffi.gaussian_filter(0.5)).desc()
    if args.make_rays:
        np.save(args.rays_file, camera_rays(desc, w, h, args.spp))
        return
    gs = I.Scene(desc)
    integ = I.PathHIP()
    build = _ffi.lib().phip_build_id().decode()
    line = dict(scene="atrium", triangles=int(desc.n_triangles), width=w, height=h, spp=args.spp, reps=args.reps, warmup=args.warmup, build=build, device=torch.cuda.get_device_name(0))
    if args.mode in ("render", "both", "parts"):
        film = torch.empty((h, w, 5), dtype=torch.float32, device="cuda")
        flags = A.PHIP_FLAG_NO_FUSED | A.PHIP_FLAG_KERNEL_TIMING
        line["render_device_no_fused"] = measure([lambda: integ.render_device(gs, film.data_ptr(), args.spp, flags=flags)], integ, args.reps, args.warmup)
    if args.mode in ("radiance", "both"):
        rays = np.load(args.rays_file) if args.rays_file and os.path.exists(args.rays_file) else camera_rays(desc, w, h, args.spp)
        assert rays.shape == (args.spp, h * w, 8), rays.shape
        t = [torch.from_numpy(r).cuda() for r in rays]
        per_sample = [(lambda k=k: integ.radiance(gs, t[k], 1, flags=A.PHIP_FLAG_KERNEL_TIMING, sample_offset=k, sample_total=args.spp)) for k in range(args.spp)]
        line["radiance_device_per_sample"] = measure(per_sample, integ, args.reps, args.warmup)
        line["radiance_device"] = measure([lambda: integ.radiance(gs, t[0], args.spp, flags=A.PHIP_FLAG_KERNEL_TIMING)], integ, args.reps, args.warmup)
    if args.mode == "parts":
        T = A.PHIP_FLAG_KERNEL_TIMING
        made = {}
        def make():
            made["rays"], made["keys"], _ = gs.camera_rays(args.spp)
            integ.stats = A.phip_stats()                    # (the call has no statistics: wall clock only)
        line["camera_rays_device"] = measure([make], integ, args.reps, args.warmup)
        rays, keys = made["rays"], made["keys"]
        t = [rays.view(h * w, args.spp, 8)[:, k].contiguous() for k in range(args.spp)]
        per_sample = [(lambda k=k: integ.radiance(gs, t[k], 1, flags=T, sample_offset=k, sample_total=args.spp)) for k in range(args.spp)]
        line["radiance_device_per_sample"] = measure(per_sample, integ, args.reps, args.warmup)
        del t
        got = {}
        def pairs():
            got["L"] = integ.radiance(gs, rays, 1, flags=T, pairs=keys, sample_total=args.spp)
        line["radiance_device_pairs"] = measure([pairs], integ, args.reps, args.warmup)
        out_film = torch.empty((h, w, 5), dtype=torch.float32, device="cuda")
        def put():
            _, integ.stats = gs.film(got["L"], args.spp, out=out_film, flags=T)
        line["film_device"] = measure([put], integ, args.reps, args.warmup)
    print(json.dumps(line))
    with open(args.out, "a") as out:
        out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

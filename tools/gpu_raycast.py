#!/usr/bin/env python3
"""phip_trace (host pointers, k_raycast_w: one ray per lane) against phip_trace_device (device pointers, k_raycast_p: persistent waves with refill) on the same rays,
in one process on one GPU, on the procedural atrium of mitsuba_amd/scene.py.  One JSON line is appended to profiles/raycast_device.jsonl (DESIGN.md 3.14 quotes it).

    python tools/gpu_raycast.py [--out profiles/raycast_device.jsonl] [--rays 4194304] [--reps 5] [--warmup 2]

Two ray sets of --rays rays each: `primary`, the rays of a pinhole camera at the scene's sensor through the pixel centres of a square image, in 8 x 8 tiles (coherent),
and `random`, uniform origins in the scene box with uniform directions (incoherent).  Per set, --reps repetitions after --warmup, each quantity as [min, median, max] ms:
  host_kernel_ms    phip_stats.trace_kernel_ms of phip_trace (HIP events around k_raycast_w, summed over its 4 M-ray chunks)
  device_kernel_ms  phip_stats.trace_kernel_ms of phip_trace_device (HIP events around k_raycast_p)
  host_wall_ms / device_wall_ms   wall clock of the two calls, closest hit + any hit (the host call copies rays up and results down and allocates its buffers)
  surfaces_ms       phip_stats.shade_kernel_ms of phip_trace_device with surfaces: k_surfaces alone
and `identical`: hits and occlusion of the two paths are the same bits."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402  (before the library touches the GPU: tests/conftest.py)

torch.cuda.init()
from mitsuba_amd import _ffi, scene as S  # noqa: E402
from mitsuba_amd import integrator as I  # noqa: E402


def primary_rays(cam, n):
    """pinhole rays through the pixel centres of a side x side image (side^2 >= n, the first n in 8 x 8 tiles)"""
    side = (int(np.ceil(np.sqrt(n))) + 7) // 8 * 8
    M = np.array(list(cam.to_world), np.float64).reshape(4, 4)
    t = np.tan(np.radians(cam.xfov_deg) / 2)
    y, x = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    tile = lambda a: a.reshape(side // 8, 8, side // 8, 8).transpose(0, 2, 1, 3).reshape(-1)[:n]
    x, y = tile(x), tile(y)
    d = np.stack([(1 - 2 * (x + 0.5) / side) * t, (1 - 2 * (y + 0.5) / side) * t, np.ones(n)], 1) @ M[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = M[:3, 3]; rays[:, 3] = 1e-4; rays[:, 4:7] = d; rays[:, 7] = np.inf
    return rays


def random_rays(rng, n, lo, hi):
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = np.inf
    return rays


def spread(v):
    return [float(np.min(v)), float(np.median(v)), float(np.max(v))]


def measure(gs, rays, reps, warmup):
    t = torch.from_numpy(rays).cuda()
    q = dict(host_kernel_ms=[], device_kernel_ms=[], host_wall_ms=[], device_wall_ms=[], surfaces_ms=[])
    for i in range(warmup + reps):
        t0 = time.perf_counter(); hh, ho, hst = gs.rayIntersect(rays, True, True); host_wall = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        t0 = time.perf_counter(); dh, do, _, dst = gs.rayIntersectDevice(t, True, True); dev_wall = (time.perf_counter() - t0) * 1e3
        _, _, _, sst = gs.rayIntersectDevice(t, True, False, True)
        if i >= warmup:
            q["host_kernel_ms"].append(hst.trace_kernel_ms); q["device_kernel_ms"].append(dst.trace_kernel_ms)
            q["host_wall_ms"].append(host_wall); q["device_wall_ms"].append(dev_wall); q["surfaces_ms"].append(sst.shade_kernel_ms)
    same = bool((dh.cpu().numpy().view(np.uint32) == hh.view(np.uint32)).all() and (do.cpu().numpy() == ho).all())
    out = {k: spread(v) for k, v in q.items()}
    out.update(identical=same, hit_share=float((hh.view(np.uint32)[:, 3] != 0xFFFFFFFF).mean()),
               host_node_visits_per_ray=hst.closest_node_visits / len(rays), device_node_visits_per_ray=dst.closest_node_visits / len(rays))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "raycast_device.jsonl"))
    ap.add_argument("--rays", type=int, default=1 << 22); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    sb = S.atrium(64, 64, _ffi.gaussian_filter(0.5))
    desc = sb.desc()
    gs = I.Scene(desc)
    P = np.concatenate(sb.positions)
    line = dict(scene="atrium", triangles=int(desc.n_triangles), rays=args.rays, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    line["primary"] = measure(gs, primary_rays(desc.camera, args.rays), args.reps, args.warmup)
    line["random"] = measure(gs, random_rays(np.random.default_rng(1), args.rays, P.min(axis=0), P.max(axis=0)), args.reps, args.warmup)
    print(json.dumps(line))
    with open(args.out, "a") as out:
        out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

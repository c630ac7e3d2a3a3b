#!/usr/bin/env python3
"""Times of phip_vertex_normals_device on one GPU, on the atrium's mesh (251 k triangles): the device call in HIP-event time (the kernel alone, as
phip_normals_info.kernel_ms states it, and the whole call between two events on its stream), against the route a caller has without it -- the host call
phip_vertex_normals on the positions in host memory plus the upload of its result, by the host's clock.

    python tools/gpu_normals.py [--out profiles/normals_device.jsonl]

Five repetitions after two warm-ups: min / median / max.  The first device call, which builds the scene's incidence lists, is timed once by the host's clock and
reported on its own.  The device's normals are checked against the host call's, bit for bit, before anything is written.  One JSON line per measurement is appended
to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

WARMUP, REPS = 2, 5


def summary(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_device.jsonl"))
    args = ap.parse_args()
    import torch
    from mitsuba_amd import _ffi, scene as S
    from mitsuba_amd.integrator import Scene
    _ffi.build()
    sb = S.atrium(64, 64, _ffi.gaussian_filter(0.5))
    desc = sb.desc()
    gs = Scene(desc)
    P = sb.flat_positions()
    T = np.ctypeslib.as_array(desc.indices, shape=(desc.n_triangles, 3)).copy()
    valence = np.bincount(T.reshape(-1), minlength=len(P))
    case = dict(case="atrium", n_vertices=int(len(P)), n_triangles=int(len(T)), max_valence=int(valence.max()), mean_valence=round(float(valence.mean()), 3))
    pos = torch.from_numpy(P).cuda()
    out = torch.empty_like(pos)
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gs.vertex_normals(pos, out=out, stream=stream)
    first_ms = 1e3 * (time.perf_counter() - t0)
    want, want_invalid = S.vertex_normals_angle_weighted(P, T, return_invalid=True)
    same = bool((out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all())
    if not same:
        raise RuntimeError("the device's normals are not the host call's")
    kernel, call = [], []
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _, info = gs.vertex_normals(pos, out=out, stream=stream, info=True)
        b.record(stream)
        b.synchronize()
        assert info.n_invalid == want_invalid
        if i >= WARMUP:
            kernel.append(info.kernel_ms); call.append(a.elapsed_time(b))
    host = []
    for i in range(WARMUP + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = S.vertex_normals_angle_weighted(P, T)
        out.copy_(torch.from_numpy(n))
        torch.cuda.synchronize()
        if i >= WARMUP:
            host.append(1e3 * (time.perf_counter() - t0))
    rows = [dict(what="device_call_kernel", **case, **summary(kernel)), dict(what="device_call_events", **case, **summary(call)),
            dict(what="host_call_and_upload", **case, **summary(host)),
            dict(what="first_device_call_with_incidence_lists", **case, min_ms=round(first_ms, 4), median_ms=round(first_ms, 4), max_ms=round(first_ms, 4))]
    gs.close()
    stamp = time.strftime("%Y-%m-%d")
    with open(args.out, "a") as f:
        for row in rows:
            row = dict(date=stamp, build_id=_ffi.built_id(), warmup=WARMUP, reps=REPS, bit_identical=same, n_invalid=want_invalid, **row)
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times of phip_mip_pyramid_device on one GPU: the pyramid of a 2048 x 1024 environment map and of a 1024 x 1024 texture, with the single-block
tail kernel and with the tail forced through the two-pass kernels, and Scene.update_appearance from an "image" tensor against the same call from host-made levels
(the host call's own time included).

    python tools/gpu_pyramid.py [--out profiles/pyramid_device.jsonl]

The pyramid is timed with HIP events on the stream the call runs on; update_appearance with the host's clock around the call and a device synchronisation, since its
host-levels form is mostly host work.  Five repetitions after two warm-ups: min / median / max.  The library without the tail is the product's sources with
-DPYRAMID_TAIL=0 (_ffi.TEST_VARIANTS["notail"]); it is measured in a child process of its own, which loads it through PHIP_LIB.  One JSON line per measurement is
appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

WARMUP, REPS = 2, 5
CASES = {"envmap_2048x1024": (2048, 1024, "repeat", "clamp", float("inf")), "texture_1024x1024": (1024, 1024, "repeat", "repeat", 1.0)}


def summary(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4)}


def time_pyramids(tag):
    import torch
    from mitsuba_amd import _ffi, scene as S
    from mitsuba_amd.integrator import Scene
    gs = Scene(S.cornell_box(16, 16, _ffi.gaussian_filter(0.5)).desc())
    rows = []
    for name, (w, h, wu, wv, maxv) in CASES.items():
        level0 = torch.rand((h, w, 3), device="cuda") * (4.0 if maxv != 1.0 else 1.0)
        out = [torch.empty((lh, lw, 3), device="cuda") for lh, lw in S.pyramid_sizes(w, h)]
        stream = torch.cuda.current_stream()
        ms = []
        for i in range(WARMUP + REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            gs.mip_pyramid(level0, wu, wv, maxv, out=out, stream=stream)
            b.record(stream)
            b.synchronize()
            if i >= WARMUP:
                ms.append(a.elapsed_time(b))
        rows.append(dict(what="mip_pyramid", case=name, library=tag, levels=len(out), **summary(ms)))
    gs.close()
    return rows


def time_update_appearance():
    import torch
    from mitsuba_amd import _ffi, scene as S
    from mitsuba_amd.integrator import Scene
    gauss = _ffi.gaussian_filter(0.5)
    rng = np.random.default_rng(1)
    rows = []
    for name, (w, h, wu, wv, maxv) in CASES.items():
        img = rng.uniform(0.05, 0.95, (h, w, 3)).astype(np.float32)
        sb = S.SceneBuilder()
        if maxv == 1.0:
            t = sb.bitmap(img, wrap=wu, wrap_v=wv, pyramid="lanczos")
            S.cornell_box(32, 32, gauss, sb=sb)
            sb.quad((100, 1, 100), (300, 1, 100), (300, 1, 300), (100, 1, 300), sb.diffuse(texture=t), facing=(0, 1, 0), uvs=True)
        else:
            sb.envmap(img, pyramid="lanczos")
            S.cornell_box(32, 32, gauss, sb=sb)
        gs = Scene(sb.desc())
        new = rng.uniform(0.05, 0.95, (h, w, 3)).astype(np.float32)
        dev = torch.from_numpy(new).cuda()

        def from_image():
            entry = dict(image=dev)
            gs.update_appearance(**({"textures": [entry]} if maxv == 1.0 else {"envmap": entry}))

        def from_host_levels():
            entry = dict(levels=S.mip_pyramid_lanczos(new, wu, wv, maxv))
            gs.update_appearance(**({"textures": [entry]} if maxv == 1.0 else {"envmap": entry}))
        for what, call in (("update_appearance_image", from_image), ("update_appearance_host_levels", from_host_levels)):
            ms = []
            for i in range(WARMUP + REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if i >= WARMUP:
                    ms.append(1e3 * (time.perf_counter() - t0))
            rows.append(dict(what=what, case=name, library="tail", **summary(ms)))
        gs.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_device.jsonl"))
    ap.add_argument("--child", default=None, help="internal: measure the pyramids with the library PHIP_LIB names and print the rows")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(time_pyramids(args.child)))
        return
    from mitsuba_amd import _ffi
    _ffi.build()
    notail = _ffi.build_test_variant("notail")
    rows = time_pyramids("tail")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "notail"], env=dict(os.environ, PHIP_LIB=notail), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the child with %s failed (%d):\n%s%s" % (notail, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    rows += json.loads(r.stdout.strip().splitlines()[-1])
    rows += time_update_appearance()
    stamp = time.strftime("%Y-%m-%d")
    with open(args.out, "a") as f:
        for row in rows:
            row = dict(date=stamp, build_id=_ffi.built_id(), warmup=WARMUP, reps=REPS, **row)
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    main()

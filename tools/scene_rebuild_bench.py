#!/usr/bin/env python3
"""phip_scene_rebuild against phip_scene_create of the same positions, in one process on one GPU: what a topology change costs on either way, and what a frame costs on
the tree either way makes.  One JSON line per (scene, displacement) is appended to profiles/scene_rebuild.jsonl (DESIGN.md 3.13 quotes them).

    python tools/scene_rebuild_bench.py [--out profiles/scene_rebuild.jsonl] [--width 1920 --height 1080 --spp 64 --max-depth 8] [--scenes atrium glass_room]

Per line: create_ms (wall clock of phip_scene_create on the displaced positions; build_ms = its host builder alone), rebuild_first_ms / rebuild_ms (wall clock of the
first phip_scene_rebuild of a scene, which allocates its scratch, and of the second; rebuild_kernel_ms = the device work of the second), sah_cost of the created, the
rebuilt and the merely refitted tree, frame_created_ms / frame_rebuilt_ms (phip_stats.render_ms, median of 3 after one warm-up frame), and break_even_frames: from how many
frames per topology change on creating the scene again is the cheaper call (null: never -- the rebuilt tree's frame is not slower)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mitsuba_amd import _ffi, scene as S
from mitsuba_amd import integrator as I


def displaced(sb, amplitude):
    """a smooth displacement field of the given amplitude on every mesh that is not a light"""
    P = np.concatenate(sb.positions)
    lo, hi = P.min(axis=0), P.max(axis=0)
    k = 2.0 * np.pi * 3.0 / (hi - lo).max()
    out = []
    for i, p in enumerate(sb.positions):
        if amplitude == 0.0 or sb.shapes[i]["emitter"] >= 0:
            out.append(p.copy())
        else:
            out.append((p + amplitude * np.sin(p[:, [1, 2, 0]].astype(np.float64) * k + np.array([0.3, 1.1, 2.0]))).astype(np.float32))
    return out


def frame_ms(integ, gs, spp):
    film = I.HDRFilm(gs.width, gs.height)
    times = []
    for i in range(4):
        assert integ.render(gs, film, spp)
        times.append(float(integ.stats.render_ms))
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "scene_rebuild.jsonl"))
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64); ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--scenes", nargs="+", default=["atrium", "glass_room"])
    ap.add_argument("--displacements", nargs="+", type=float, default=[0.0, 0.02], help="fractions of the scene's largest extent")
    args = ap.parse_args()
    gauss = _ffi.gaussian_filter(0.5)
    integ = I.PathHIP(maxDepth=args.max_depth)
    with open(args.out, "a") as out:
        for name in args.scenes:
            for frac in args.displacements:
                sb = getattr(S, name)(args.width, args.height, gauss)
                desc_a = sb.desc()
                extent = float((np.concatenate(sb.positions).max(axis=0) - np.concatenate(sb.positions).min(axis=0)).max())
                sb.positions = displaced(sb, frac * extent)
                Pb, Nb = sb.flat_positions(), sb.flat_normals()
                desc_b = sb.desc()
                t0 = time.perf_counter(); created = I.Scene(desc_b); create_ms = (time.perf_counter() - t0) * 1e3
                ci = created.accel_info()
                rebuilt = I.Scene(desc_a)
                first = rebuilt.rebuild(positions=Pb, normals=Nb)
                second = rebuilt.rebuild(positions=Pb, normals=Nb)
                ri = rebuilt.accel_info()
                refitted = I.Scene(desc_a)
                refit = refitted.update(positions=Pb, normals=Nb)
                del refitted
                fc, fr = frame_ms(integ, created, args.spp), frame_ms(integ, rebuilt, args.spp)
                line = dict(scene=name, triangles=int(desc_b.n_triangles), width=args.width, height=args.height, spp=args.spp, max_depth=args.max_depth,
                            displacement_fraction=frac, displacement=frac * extent,
                            create_ms=create_ms, build_ms=float(ci.build_ms), rebuild_first_ms=float(first.update_ms), rebuild_ms=float(second.update_ms),
                            rebuild_kernel_ms=float(second.kernel_ms), refit_ms=float(refit.update_ms),
                            sah_cost_created=float(ci.sah_cost), sah_cost_rebuilt=float(ri.sah_cost), sah_cost_refitted=float(refit.sah_cost),
                            nodes_created=int(ci.n_nodes), nodes_rebuilt=int(ri.n_nodes), depth_created=int(ci.max_depth), depth_rebuilt=int(ri.max_depth),
                            records_created=int(ci.n_triangle_refs), records_rebuilt=int(ri.n_triangle_refs),
                            frame_created_ms=fc, frame_rebuilt_ms=fr,
                            break_even_frames=((create_ms - second.update_ms) / (fr - fc) if fr > fc else None))
                print(json.dumps(line)); out.write(json.dumps(line) + "\n"); out.flush()
                del created, rebuilt


if __name__ == "__main__":
    main()

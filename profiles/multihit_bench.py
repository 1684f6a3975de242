"""All-hits ray query throughput (include/shader_ray_multihit.h), one JSON line on stdout.

Scenes: the bunny-class scene and the 1M-triangle OBJ.  Rays, 2^20 of each per scene:
  through  from a sphere around the scene aimed at points in its box (every ray crosses the box), in Morton order of the origin
  random   tests/test_gpu_ray_query.py's random rays (origins in twice the box, inside and on the mesh; mixed tmax)
Per scene and ray set:
  (i)   the first K crossings for K = 1, 4, 8, with counts (the walk that skips nothing) and without (the pruned walk)
  (ii)  trace_rays' closest hit (kernel id 0, no iteration cap) on the same rays: the yardstick
  (iii) what a caller did before: K successive trace_rays calls, each re-started from the previous hit (time only: its
        answers are not comparable at coincident surfaces)
Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
The counters per ray are those of the walk that skips nothing (one blocking counting run) and of the closest-hit walk.
Usage: python profiles/multihit_bench.py [--trials 15] [--warmup 5] [--no-million]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

F = np.float32


def through_rays(positions, n, seed):
    """origins on a sphere of 1.5 box diagonals around the box centre, aimed at uniform points of the box; tmax 1e7"""
    rng = np.random.default_rng(seed)
    v = positions.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    centre, radius = (lo + hi) / 2, 1.5 * np.linalg.norm(hi - lo)
    s = rng.normal(size=(n, 3))
    o = centre + radius * s / np.linalg.norm(s, axis=1, keepdims=True)
    d = lo + (hi - lo) * rng.random((n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F), np.full(n, F(1e7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch
    import ray_query_ref as R
    from __graft_entry__ import load_package
    from point_query_bench import morton_order
    from test_gpu_ray_query import random_rays

    pkg = load_package()
    stream = torch.cuda.current_stream()
    n = 1 << 20

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        times = []
        for _ in range(args.trials):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times)), float(min(times)), float(max(times))

    def entry(ms, lo, hi):
        return {"ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "Mrays_s": round(n / ms / 1e3, 1)}

    def case(scene, o, d, tmax):
        rays = pkg.tracer.make_rays(o, d, tmax)
        d_rays = torch.from_numpy(rays.view(F).reshape(-1, 8).copy()).cuda()
        d_hits = torch.empty((n, 8, 4), dtype=torch.int32, device="cuda")
        d_counts = torch.empty(n, dtype=torch.int32, device="cuda")
        out = {}
        for k in (1, 4, 8):
            for with_counts in (True, False):
                out[f"first_{k}" + ("_with_counts" if with_counts else "")] = entry(*median_ms(lambda: scene.trace_all_hits_into(
                    d_rays.data_ptr(), n, d_hits.data_ptr(), d_counts.data_ptr() if with_counts else 0, k, stream.cuda_stream)))
        out["counts_only"] = entry(*median_ms(lambda: scene.trace_all_hits_into(d_rays.data_ptr(), n, 0, d_counts.data_ptr(), 0,
                                                                               stream.cuda_stream)))
        d_one = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        out["trace_rays_closest"] = entry(*median_ms(lambda: scene.trace_rays_into(d_rays.data_ptr(), n, d_one.data_ptr(),
                                                                                  stream.cuda_stream, max_bvh_iterations=0)))
        work = torch.empty_like(d_rays)

        def retrace(k):
            work.copy_(d_rays)
            for _ in range(k):
                scene.trace_rays_into(work.data_ptr(), n, d_one.data_ptr(), stream.cuda_stream, max_bvh_iterations=0)
                hit = d_one[:, 3].view(torch.int32) >= 0
                t = torch.where(hit, d_one[:, 0], torch.zeros_like(d_one[:, 0]))
                work[:, 0:3] += work[:, 4:7] * t[:, None]                       # re-start from the hit point
                work[:, 3] = torch.where(hit, work[:, 3] - t, torch.zeros_like(t))   # a miss ends the ray (tmax 0: no walk)

        for k in (4, 8):
            out[f"retrace_{k}_calls"] = entry(*median_ms(lambda: retrace(k)))
        _, counts, c = scene.trace_all_hits(rays, max_hits=0, counters=True)
        _, cc = scene.trace_rays(rays, max_bvh_iterations=0, counters=True)
        out["per_ray"] = {"crossings": round(float(counts.mean()), 3), "crossings_max": int(counts.max()),
                          "unpruned_node_visits": round(c["node_visits"] / n, 2), "unpruned_leaf_visits": round(c["leaf_visits"] / n, 2),
                          "unpruned_triangle_tests": round(c["triangle_tests"] / n, 2),
                          "closest_node_visits": round(cc["node_visits"] / n, 2), "closest_leaf_visits": round(cc["leaf_visits"] / n, 2),
                          "closest_triangle_tests": round(cc["triangle_tests"] / n, 2)}
        return out

    out = {"trials": args.trials, "warmup": args.warmup, "rays": n, "device": torch.cuda.get_device_name(0)}
    scenes = [("bunny", pkg.scenes.bunny_trisrc)] + ([] if args.no_million else [("million", pkg.scenes.million_obj)])
    for name, path in scenes:
        world = pkg.World(path())
        arrays = R.SceneArrays(world.arrays())
        scene = pkg.Scene(world.flatten())
        scene.set_kernel(0)
        o, d, tmax = through_rays(arrays.positions, n, seed=2026)
        order = morton_order(o)
        out[name] = {"triangles": len(arrays.positions),
                     "through": case(scene, o[order], d[order], tmax[order]),
                     "random": case(scene, *random_rays(arrays, n, seed=2027))}
        scene.close()
        world.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

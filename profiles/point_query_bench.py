"""Closest-point query throughput (include/shader_ray_point.h), one JSON line on stdout.

  (a) the bunny-class scene, 2^20 points near the surface (within a hundredth of the scene's extent), in Morton order
  (b) the same points shuffled
  (c) the bunny-class scene, 2^20 points uniform in the scene's box
  (d) the 1M-triangle OBJ, 2^20 points near its surface, in Morton order
  (e) for scale: a chunked torch brute force on the GPU (plain fp32 torch operations, every point against every triangle)
      of 2^12 near points on the bunny-class scene

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
The counters (mean node visits, i.e. box bounds evaluated, and triangle tests per point) come from one blocking counting
run of the same points.
Usage: python profiles/point_query_bench.py [--trials 15] [--warmup 5] [--no-million]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

F = np.float32


def near_points(positions, n, seed):
    """points on the surface (uniform over the triangles' area) moved along the normal by up to extent/100 either way"""
    rng = np.random.default_rng(seed)
    tri = positions.reshape(-1, 3, 3).astype(np.float64)
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.linalg.norm(cross, axis=1)
    k = rng.choice(len(tri), n, p=area / area.sum())
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    p = tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])
    nrm = cross[k] / np.maximum(area[k], 1e-30)[:, None]
    extent = float(np.linalg.norm(tri.reshape(-1, 3).max(0) - tri.reshape(-1, 3).min(0)))
    return (p + nrm * ((rng.random(n) * 2 - 1) * extent / 100)[:, None]).astype(F)


def morton_order(p):
    """the permutation that sorts points by the 30-bit Morton code of their position in their bounding box"""
    lo, hi = p.min(0), p.max(0)
    q = np.clip(((p - lo) / np.maximum(hi - lo, 1e-30) * 1023).astype(np.int64), 0, 1023)
    code = np.zeros(len(p), np.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return np.argsort(code, kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch
    import point_query_ref as R
    from __graft_entry__ import load_package

    pkg = load_package()
    stream = torch.cuda.current_stream()

    def median_ms(fn, trials=None, warmup=None):
        for _ in range(args.warmup if warmup is None else warmup):
            fn()
        times = []
        for _ in range(args.trials if trials is None else trials):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times)), float(min(times)), float(max(times))

    def case(scene, pts):
        points = pkg.tracer.make_points(pts)
        d_pts = torch.from_numpy(points.view(F).reshape(-1, 4).copy()).cuda()
        d_out = torch.empty((len(pts), 8), dtype=torch.int32, device="cuda")
        ms, lo, hi = median_ms(lambda: scene.closest_points_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), stream.cuda_stream))
        _, c = scene.closest_points(points, counters=True)
        return {"points": len(pts), "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                "Mpoints_s": round(len(pts) / ms / 1e3, 1), "node_visits_per_point": round(c["node_visits"] / len(pts), 2),
                "leaf_visits_per_point": round(c["leaf_visits"] / len(pts), 2),
                "triangle_tests_per_point": round(c["triangle_tests"] / len(pts), 2)}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    world = pkg.World(pkg.scenes.bunny_trisrc())
    pos = np.asarray(world.arrays()["vertex_positions"], F)
    scene = pkg.Scene(world.flatten())
    out["bunny_triangles"] = len(pos) // 9
    n = 1 << 20
    near = near_points(pos, n, seed=2026)
    near = near[morton_order(near)]
    out["a_bunny_near_morton"] = case(scene, near)
    out["b_bunny_near_shuffled"] = case(scene, near[np.random.default_rng(1).permutation(n)])
    verts = pos.reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    uniform = (lo + (hi - lo) * np.random.default_rng(3).random((n, 3))).astype(F)
    out["c_bunny_uniform_box"] = case(scene, uniform)

    # (e) plain fp32 torch, chunked over points: every point against every triangle (the restatement's arithmetic)
    class Fp32Torch(R.TorchOps):
        def add(self, a, b):
            return a + b

        def sub(self, a, b):
            return a - b

        def mul(self, a, b):
            return a * b

        def div(self, a, b):
            return a / b

    small = pkg.tracer.make_points(near[np.random.default_rng(5).permutation(n)[:1 << 12]])
    ops = Fp32Torch("cuda")
    ms, lo_ms, hi_ms = median_ms(lambda: R._closest(ops, pos, small, 256, 1 << 24), trials=3, warmup=1)
    out["e_torch_brute_force_bunny"] = {"points": len(small), "ms": round(ms, 2), "ms_min_max": [round(lo_ms, 2), round(hi_ms, 2)],
                                        "Mpoints_s": round(len(small) / ms / 1e3, 4),
                                        "triangle_tests_per_point": out["bunny_triangles"]}
    scene.close()
    world.close()

    if not args.no_million:
        world = pkg.World(pkg.scenes.million_obj())
        pos = np.asarray(world.arrays()["vertex_positions"], F)
        scene = pkg.Scene(world.flatten())
        near = near_points(pos, n, seed=2027)
        out["million_triangles"] = len(pos) // 9
        out["d_million_near_morton"] = case(scene, near[morton_order(near)])
        scene.close()
        world.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

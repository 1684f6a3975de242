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
import numpy as np

import bench_harness as H
from bench_workloads import morton_order, near_points

F = np.float32


def main():
    ap = H.parser()
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch
    import point_query_ref as R

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    median_ms = H.median_timer(args)

    def case(scene, pts):
        points = pkg.tracer.make_points(pts)
        d_pts = H.upload(points, 4)
        d_out = torch.empty((len(pts), 8), dtype=torch.int32, device="cuda")
        t = median_ms(lambda: scene.closest_points_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), stream.cuda_stream))
        _, c = scene.closest_points(points, counters=True)
        return H.entry(t, "Mpoints_s", len(pts), places=1, trials=False, points=len(pts)) | {
            "node_visits_per_point": round(c["node_visits"] / len(pts), 2),
            "leaf_visits_per_point": round(c["leaf_visits"] / len(pts), 2),
            "triangle_tests_per_point": round(c["triangle_tests"] / len(pts), 2)}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    with H.bunny_scene(pkg) as (world, scene, pos):
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
        ms, lo_ms, hi_ms, _ = median_ms(lambda: R._closest(ops, pos, small, 256, 1 << 24), trials=3, warmup=1)
        out["e_torch_brute_force_bunny"] = {"points": len(small), "ms": round(ms, 2), "ms_min_max": [round(lo_ms, 2), round(hi_ms, 2)],
                                            "Mpoints_s": round(len(small) / ms / 1e3, 4),
                                            "triangle_tests_per_point": out["bunny_triangles"]}

    if not args.no_million:
        with H.million_scene(pkg) as (world, scene, pos):
            near = near_points(pos, n, seed=2027)
            out["million_triangles"] = len(pos) // 9
            out["d_million_near_morton"] = case(scene, near[morton_order(near)])
    H.emit(out, args)


if __name__ == "__main__":
    main()

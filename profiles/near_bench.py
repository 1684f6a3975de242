"""Within-radius query throughput (include/shader_ray_near.h), one JSON line on stdout.

Scenes: the bunny-class scene and the 1M-triangle OBJ; 2^20 points near the surface (point_query_bench.py's, in Morton order).
Radii: 1 %, 5 % and 20 % of the scene's extent, and +inf for the pruned forms.  Forms: K = 1, 4, 8, 64 pruned (no counts) and
with counts, and counts only (K = 0).

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
A counting walk at a wide radius tests thousands of triangles a point, so the forms with counts run on the first 2^m points,
m the largest with (triangle tests per point) * 2^m <= --max-tests (at least 2^12 points; the entry says how many); a form
whose first launch takes over half a second is timed over 3 launches.  The mean and maximum of n and the counters per point
(node visits, i.e. box bounds evaluated, leaf visits, triangle tests, of the walk that prunes only by max_dist2) come from
one blocking counting run of 2^12 of the points.

In the same run, on the same points:
  closest_vs_k1   K = 1 pruned at +inf against shray_closest_points_device, alternating, with the ratio
  torch_vs_k8     K = 8 with counts at the 5 % radius on 2^12 points against the restatement's arithmetic in plain fp32 torch
                  on the GPU (every point against every triangle, tests/near_ref.py)
  --ab A.so B.so  two builds of the library (the stack's two entry forms, near/near.hip SHRAY_NEAR_NAME_STACK) alternating

Usage: python profiles/near_bench.py [--trials 15] [--warmup 5] [--no-million] [--max-tests 2e9] [--ab A.so B.so]"""
import ctypes as C
import os

import numpy as np

import bench_harness as H
from bench_workloads import morton_order, near_points

F = np.float32
KS = (1, 4, 8, 64)
RADII = (0.01, 0.05, 0.20)


def main():
    ap = H.parser()
    ap.add_argument("--no-million", action="store_true")
    ap.add_argument("--max-tests", type=float, default=2e9)
    ap.add_argument("--ab", nargs=2, metavar="LIB")
    args = ap.parse_args()
    import torch
    import near_ref as NR
    import point_query_ref as R

    pkg = H.load_package()
    N = pkg._native
    stream = torch.cuda.current_stream()
    shipped = N.load_near()

    clock = H.event_clock(stream)
    median_ms = H.median_timer(args, slow_ms=500.0, clock=clock)

    def entry(points, t):
        return H.entry(t, "Mpoints_s", points, points=points)

    def launcher(lib, scene, d_pts, count, k, counts, d_out, d_cnt):
        np_ = pkg.tracer.near_params(k)
        out_ptr = C.c_void_p(d_out.data_ptr() if k else None)
        cnt_ptr = C.c_void_p(d_cnt.data_ptr() if counts else None)

        def launch():
            N.check(lib.shray_near_triangles_device(scene._handle, C.byref(np_), C.c_void_p(d_pts.data_ptr()), count, out_ptr, cnt_ptr,
                                                    C.c_void_p(stream.cuda_stream)))
        return launch

    def device(points):
        return H.upload(points, 4)

    def scene_cases(scene, pos, pts):
        n = len(pts)
        extent = float(np.linalg.norm(pos.reshape(-1, 3).max(0) - pos.reshape(-1, 3).min(0)))
        d_out = torch.empty((n, 64, 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        sample = np.random.default_rng(5).permutation(n)[:1 << 12]
        res = {}
        for radius in RADII + (np.inf,):
            points = pkg.tracer.make_points(pts, F((radius * extent) ** 2) if np.isfinite(radius) else None)
            d_pts = device(points)
            row = {}
            if np.isfinite(radius):
                _, cnt, c = scene.triangles_within(points[sample], max_near=0, counters=True)
                per = {k: round(c[k] / len(sample), 2) for k in ("node_visits", "leaf_visits", "triangle_tests")}
                row["n_mean"], row["n_max"], row["per_point"] = round(float(cnt.mean()), 2), int(cnt.max()), per
                m = n
                while m > (1 << 12) and per["triangle_tests"] * m > args.max_tests:
                    m //= 2
            for k in KS:
                row[f"K{k}_pruned"] = entry(n, median_ms(launcher(shipped, scene, d_pts, n, k, False, d_out, d_cnt)))
            if np.isfinite(radius):
                for k in KS + (0,):
                    name = f"K{k}_counts" if k else "counts_only"
                    row[name] = entry(m, median_ms(launcher(shipped, scene, d_pts, m, k, True, d_out, d_cnt)))
            res["inf" if not np.isfinite(radius) else f"r{int(round(radius * 100))}pct"] = row
        return res, extent

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    with H.bunny_scene(pkg) as (world, scene, pos):
        out["bunny_triangles"] = len(pos) // 9
        n = 1 << 20
        near = near_points(pos, n, seed=2026)
        near = near[morton_order(near)]
        out["bunny"], extent = scene_cases(scene, pos, near)

        # K = 1 pruned against the closest-point query, the same points, alternating
        points = pkg.tracer.make_points(near)
        d_pts = device(points)
        d_one = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        k1 = launcher(shipped, scene, d_pts, n, 1, False, d_one, None)

        def closest():
            scene.closest_points_into(d_pts.data_ptr(), n, d_one.data_ptr(), stream.cuda_stream)

        ab = H.alternating(closest, k1, trials=args.trials, clock=clock)
        a, b = ab["ms"]
        out["closest_vs_k1"] = {"points": n, "closest_points_ms": round(a, 4), "K1_pruned_ms": round(b, 4), "ratio_K1_over_closest": round(b / a, 4),
                                "closest_points_ms_first_second_half": [round(x, 4) for x in ab["a_first_second_half"]]}

        # K = 8 with counts at the 5 % radius on 2^12 points against plain fp32 torch, every point against every triangle
        class Fp32Torch(R.TorchOps):
            def add(self, a, b):
                return a + b

            def sub(self, a, b):
                return a - b

            def mul(self, a, b):
                return a * b

            def div(self, a, b):
                return a / b

        small = pkg.tracer.make_points(near[np.random.default_rng(5).permutation(n)[:1 << 12]], F((0.05 * extent) ** 2))
        d_small = device(small)
        ours = median_ms(launcher(shipped, scene, d_small, len(small), 8, True, d_one.view(-1)[: len(small) * 64].view(-1, 8, 8),
                                                      torch.empty(len(small), dtype=torch.int32, device="cuda")))
        ops = Fp32Torch("cuda")
        brute = median_ms(lambda: NR._near(ops, pos, small, 8, 512, 1 << 24), trials=3, warmup=1)
        out["torch_vs_k8"] = {"K8_counts": entry(len(small), ours), "torch_brute_force": entry(len(small), brute),
                              "speedup": round(brute.ms / ours.ms, 1)}

        if args.ab:
            libs = [N._bind(C.CDLL(os.path.abspath(p)), N.NEAR_SYMBOLS) for p in args.ab]
            d_out = torch.empty((n, 8, 8), dtype=torch.int32, device="cuda")
            d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
            ab = {"libraries": [os.path.basename(p) for p in args.ab]}
            for label, md, k, counts in (("K1_pruned_inf", None, 1, False), ("K8_pruned_inf", None, 8, False),
                                         ("K8_pruned_r5pct", F((0.05 * extent) ** 2), 8, False), ("K8_counts_r1pct", F((0.01 * extent) ** 2), 8, True)):
                d_p = device(pkg.tracer.make_points(near, md))
                fns = [launcher(lib, scene, d_p, n, k, counts, d_out, d_cnt) for lib in libs]
                pair = H.alternating(fns[0], fns[1], trials=args.trials, clock=clock)
                ab[label] = {"ms": [round(x, 4) for x in pair["ms"]], "ms_min": [round(x, 4) for x in pair["ms_min"]]}
            out["stack_entry_ab"] = ab

    if not args.no_million:
        with H.million_scene(pkg) as (world, scene, pos):
            near = near_points(pos, n, seed=2027)
            out["million_triangles"] = len(pos) // 9
            out["million"], _ = scene_cases(scene, pos, near[morton_order(near)])
    H.emit(out, args)


if __name__ == "__main__":
    main()

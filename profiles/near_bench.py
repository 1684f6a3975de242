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
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

F = np.float32
KS = (1, 4, 8, 64)
RADII = (0.01, 0.05, 0.20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-million", action="store_true")
    ap.add_argument("--max-tests", type=float, default=2e9)
    ap.add_argument("--ab", nargs=2, metavar="LIB")
    args = ap.parse_args()
    import torch
    import near_ref as NR
    import point_query_ref as R
    from __graft_entry__ import load_package
    from point_query_bench import morton_order, near_points

    pkg = load_package()
    N = pkg._native
    stream = torch.cuda.current_stream()
    shipped = N.load_near()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def median_ms(fn, trials=None, warmup=None):
        trials, warmup = args.trials if trials is None else trials, args.warmup if warmup is None else warmup
        if timed(fn) > 500.0:
            trials, warmup = 3, 0
        for _ in range(warmup):
            fn()
        times = [timed(fn) for _ in range(trials)]
        return float(np.median(times)), float(min(times)), float(max(times)), trials

    def entry(points, ms, lo, hi, trials):
        return {"points": points, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "trials": trials,
                "Mpoints_s": round(points / ms / 1e3, 4)}

    def launcher(lib, scene, d_pts, count, k, counts, d_out, d_cnt):
        np_ = pkg.tracer.near_params(k)
        out_ptr = C.c_void_p(d_out.data_ptr() if k else None)
        cnt_ptr = C.c_void_p(d_cnt.data_ptr() if counts else None)

        def launch():
            N.check(lib.shray_near_triangles_device(scene._handle, C.byref(np_), C.c_void_p(d_pts.data_ptr()), count, out_ptr, cnt_ptr,
                                                    C.c_void_p(stream.cuda_stream)))
        return launch

    def device(points):
        return torch.from_numpy(points.view(F).reshape(-1, 4).copy()).cuda()

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
                row[f"K{k}_pruned"] = entry(n, *median_ms(launcher(shipped, scene, d_pts, n, k, False, d_out, d_cnt)))
            if np.isfinite(radius):
                for k in KS + (0,):
                    name = f"K{k}_counts" if k else "counts_only"
                    row[name] = entry(m, *median_ms(launcher(shipped, scene, d_pts, m, k, True, d_out, d_cnt)))
            res["inf" if not np.isfinite(radius) else f"r{int(round(radius * 100))}pct"] = row
        return res, extent

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    world = pkg.World(pkg.scenes.bunny_trisrc())
    pos = np.asarray(world.arrays()["vertex_positions"], F)
    scene = pkg.Scene(world.flatten())
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

    for fn in (k1, closest) * 3:
        fn()
    pairs = [(timed(closest), timed(k1)) for _ in range(args.trials)]
    a, b = float(np.median([p[0] for p in pairs])), float(np.median([p[1] for p in pairs]))
    half = len(pairs) // 2   # the spread of the yardstick itself: its first and second half of the launches
    a2, b2 = float(np.median([p[0] for p in pairs[:half]])), float(np.median([p[0] for p in pairs[half:]]))
    out["closest_vs_k1"] = {"points": n, "closest_points_ms": round(a, 4), "K1_pruned_ms": round(b, 4), "ratio_K1_over_closest": round(b / a, 4),
                            "closest_points_ms_first_second_half": [round(a2, 4), round(b2, 4)]}

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
    ms, lo_ms, hi_ms, trials = median_ms(launcher(shipped, scene, d_small, len(small), 8, True, d_one.view(-1)[: len(small) * 64].view(-1, 8, 8),
                                                  torch.empty(len(small), dtype=torch.int32, device="cuda")))
    ops = Fp32Torch("cuda")
    t_ms, t_lo, t_hi, t_trials = median_ms(lambda: NR._near(ops, pos, small, 8, 512, 1 << 24), trials=3, warmup=1)
    out["torch_vs_k8"] = {"K8_counts": entry(len(small), ms, lo_ms, hi_ms, trials), "torch_brute_force": entry(len(small), t_ms, t_lo, t_hi, t_trials),
                          "speedup": round(t_ms / ms, 1)}

    if args.ab:
        libs = [N._bind(C.CDLL(os.path.abspath(p)), N.NEAR_SYMBOLS) for p in args.ab]
        d_out = torch.empty((n, 8, 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        ab = {"libraries": [os.path.basename(p) for p in args.ab]}
        for label, md, k, counts in (("K1_pruned_inf", None, 1, False), ("K8_pruned_inf", None, 8, False),
                                     ("K8_pruned_r5pct", F((0.05 * extent) ** 2), 8, False), ("K8_counts_r1pct", F((0.01 * extent) ** 2), 8, True)):
            d_p = device(pkg.tracer.make_points(near, md))
            fns = [launcher(lib, scene, d_p, n, k, counts, d_out, d_cnt) for lib in libs]
            for fn in fns * 3:
                fn()
            pairs = [(timed(fns[0]), timed(fns[1])) for _ in range(args.trials)]
            ab[label] = {"ms": [round(float(np.median([p[j] for p in pairs])), 4) for j in range(2)],
                         "ms_min": [round(float(min(p[j] for p in pairs)), 4) for j in range(2)]}
        out["stack_entry_ab"] = ab
    scene.close()
    world.close()

    if not args.no_million:
        world = pkg.World(pkg.scenes.million_obj())
        pos = np.asarray(world.arrays()["vertex_positions"], F)
        scene = pkg.Scene(world.flatten())
        near = near_points(pos, n, seed=2027)
        out["million_triangles"] = len(pos) // 9
        out["million"], _ = scene_cases(scene, pos, near[morton_order(near)])
        scene.close()
        world.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Instanced closest-point query throughput (include/shader_ray_instance_point.h), one JSON line on stdout.

Rows, each on the device path with near-surface points (a random triangle's centroid plus 1 % of the scene's extent of noise,
mapped into a random instance):
  a_identity     the bunny-class scene under one identity instance, 2^20 points, against Scene.closest_points on the same
                 points: the cost of the layer
  b_bunny_8x8    profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid, 2^20 points
  b_rigid_8x8    the same grid with rotations only, and beside it the loop a caller would write today for rigid maps: 64
                 Scene.closest_points calls on the points moved by world_to_object in torch, merged on the device by dist2
                 (the lower instance on a tie), with how often the two name the same instance and triangle
  c_lobed_4096   4,096 copies of lobed_528 on a 16 x 16 x 16 grid, 2^20 points

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.  The walk counters per point (node visits, i.e. image-box bounds evaluated, leaf
visits, triangle tests, and instance walks begun) come from one blocking counting run over 2^12 of the same points; row a's
are Scene.closest_points' own, so the other rows' against them say what the looser image boxes and the top level cost.

Usage: python profiles/instance_point_bench.py [--trials 15] [--warmup 5] [--points 1048576]"""
import sys

import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms, near_surface_points

F = np.float32
SAMPLE = 1 << 12


def main():
    ap = H.parser()
    ap.add_argument("--points", type=int, default=1 << 20)
    args = ap.parse_args()
    import torch

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = args.points
    median_ms = H.median_timer(args, slow_ms=2000.0)

    def entry(points, t):
        return H.entry(t, "Mpoints_s", points, points=points)

    def per_point(c, count):
        return {key: round(c[key] / count, 2) for key in ("node_visits", "leaf_visits", "triangle_tests", "traversals")}

    def set_row(s, pts):
        d_pts = torch.from_numpy(pts).cuda()
        d_out = torch.empty((len(pts), 8), dtype=torch.int32, device="cuda")
        d_inst = torch.empty(len(pts), dtype=torch.int32, device="cuda")
        r = entry(len(pts), median_ms(lambda: s.closest_points_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), d_inst.data_ptr(),
                                                                    stream.cuda_stream)))
        r["instances"] = s.count
        r["hit_fraction"] = round(float((d_inst >= 0).float().mean()), 4)
        _, _, c = s.closest_points(pts[:SAMPLE], counters=True)
        r["per_point"] = per_point(c, min(SAMPLE, len(pts)))
        print(f"  {s.count} instances: {r['ms']} ms, {r['per_point']}", file=sys.stderr, flush=True)
        return r, d_pts, d_out, d_inst

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(2026)

    # (a) -----------------------------------------------------------------------------------------------------------------
    with H.bunny_scene(pkg) as (world, bunny, positions):
        eye = np.eye(3, 4, dtype=F)[None]
        one = pkg.tracer.InstanceSet([bunny], eye)
        pts = near_surface_points(positions, eye, n, rng)
        row, d_pts, d_out, _ = set_row(one, pts)
        d_plain = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        plain = entry(n, median_ms(lambda: bunny.closest_points_into(d_pts.data_ptr(), n, d_plain.data_ptr(), stream.cuda_stream)))
        _, c = bunny.closest_points(pts[:SAMPLE], counters=True)
        plain["per_point"] = per_point(c, min(SAMPLE, n))
        out["a_identity"] = {"triangles": len(positions) // 9, "instance": row, "scene": plain, "instance_over_scene": round(row["ms"] / plain["ms"], 3),
                             "same_bytes": bool(torch.equal(d_out, d_plain))}
        one.close()

        # (b) -----------------------------------------------------------------------------------------------------------------
        extent = float(np.ptp(positions.reshape(-1, 3).astype(np.float64), axis=0).max())
        M = grid_transforms((8, 8), 1.5 * extent, np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        out["b_bunny_8x8"] = set_row(grid, near_surface_points(positions, M, n, rng))[0]
        grid.close()

        M = grid_transforms((8, 8), 1.5 * extent, np.random.default_rng(2026), scale=(1.0, 1.0))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        row, d_pts, d_out, d_inst = set_row(grid, near_surface_points(positions, M, n, rng))
        d_W = torch.from_numpy(grid.world_to_object()).cuda()
        moved = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        best = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        best_inst = torch.empty(n, dtype=torch.int32, device="cuda")

        def caller_loop():
            """what a caller writes today for rigid maps: per instance the points into object space, the plain query, the nearer kept"""
            best[:, 3] = torch.tensor(float("inf")).view(torch.int32).item()
            best[:, 6] = -1
            best_inst.fill_(-1)
            for i in range(64):
                moved[:, :3] = d_pts[:, :3] @ d_W[i, :, :3].T + d_W[i, :, 3]
                moved[:, 3] = d_pts[:, 3]
                bunny.closest_points_into(moved.data_ptr(), n, rec.data_ptr(), stream.cuda_stream)
                nearer = (rec[:, 6] >= 0) & (rec[:, 3].view(torch.float32) < best[:, 3].view(torch.float32))
                best[nearer] = rec[nearer]
                best_inst[nearer] = i

        loop = entry(n, median_ms(caller_loop))
        agree = (best_inst == d_inst) & (best[:, 6] == d_out[:, 6])
        out["b_rigid_8x8"] = {"set": row, "caller_loop": loop, "loop_over_set": round(loop["ms"] / row["ms"], 2),
                              "same_instance_and_triangle": round(float(agree.float().mean()), 6)}
        grid.close()
    del d_pts, d_out, d_inst, moved, rec, best, best_inst, d_plain

    # (c) -----------------------------------------------------------------------------------------------------------------
    with H.lobed_scene(pkg) as (world, lobed, positions):
        extent = float(np.ptp(positions.reshape(-1, 3).astype(np.float64), axis=0).max())
        M = grid_transforms((16, 16, 16), 1.5 * extent, np.random.default_rng(2027))
        grid = pkg.tracer.InstanceSet([lobed] * 4096, M)
        out["c_lobed_4096"] = set_row(grid, near_surface_points(positions, M, n, rng))[0]
        grid.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

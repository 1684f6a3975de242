"""Instanced winding number query cost (include/shader_ray_instance_winding.h), one JSON line on stdout.

profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid, 2^20 near-surface world points (a
random triangle's centroid plus 1 % of the scene's extent of noise, mapped into a random instance) in Morton order, on the
device path:
  instanced            InstanceSet.winding_number_into at beta = 2, with the containing instances: one launch over the set
  caller_loop          what it replaces, in the same run: per instance, the points mapped to object space by torch,
                       Scene.winding_number_into on the member, and the signed accumulation (64 launch pairs, the points
                       read and written once per instance)
  loop_over_instanced  the ratio
  exact                the exact mode (beta = +inf) on 2^14 of the points
  unsigned             InstanceSet.closest_points_into alone
  winding_signed       InstanceSet.winding_signed_distance_into with the caller's record and instance buffers
  winding_signed_over_unsigned  the ratio: what the sign costs on top of the distance
and how far the loop's values are from the one launch's (torch maps the points with its own operation order, so they are
compared, not expected to be equal bit for bit).

Every time is the median of --trials runs after --warmup runs, bracketed by HIP events on the current torch stream.
Usage: python profiles/instance_winding_bench.py [--trials 15] [--warmup 5] [--points 1048576]"""
import math

import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms, morton_order, near_surface_points

F = np.float32
EXACT_POINTS = 1 << 14


def main():
    ap = H.parser()
    ap.add_argument("--points", type=int, default=1 << 20)
    args = ap.parse_args()
    import torch

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = args.points
    median_ms = H.median_timer(args)

    def row(fn, points=n):
        return H.entry(median_ms(fn), "Mpoints_s", points, places=1, trials=False, points=points)

    with H.bunny_scene(pkg) as (world, bunny, positions):
        extent = float(np.ptp(positions.reshape(-1, 3).astype(np.float64), axis=0).max())
        M = grid_transforms((8, 8), 1.5 * extent, np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        pts = near_surface_points(positions, M, n, np.random.default_rng(2026))
        pts = pts[morton_order(pts[:, :3])]
        d_pts = torch.from_numpy(pts).cuda()
        d_w = torch.empty(n, dtype=torch.float32, device="cuda")
        d_in = torch.empty(n, dtype=torch.int32, device="cuda")
        d_rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
        d_sd = torch.empty(n, dtype=torch.float32, device="cuda")
        grid.winding_number_into(d_pts.data_ptr(), 1, d_w.data_ptr(), 0, 2.0, stream.cuda_stream)   # derive once, outside the timings

        out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "instances": grid.count,
               "triangles": len(positions) // 9, "beta": 2.0}
        out["instanced"] = row(lambda: grid.winding_number_into(d_pts.data_ptr(), n, d_w.data_ptr(), d_in.data_ptr(), 2.0, stream.cuda_stream))
        one_launch = d_w.clone()

        # the caller's loop
        W = torch.from_numpy(grid.world_to_object()).cuda()
        s = grid.orientations()
        d_obj = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        d_obj[:, 3] = math.inf
        d_term = torch.empty(n, dtype=torch.float32, device="cuda")
        d_acc = torch.empty(n, dtype=torch.float32, device="cuda")

        def loop():
            d_acc.zero_()
            for i in range(grid.count):
                d_obj[:, :3] = d_pts[:, :3] @ W[i, :, :3].T + W[i, :, 3]
                bunny.winding_number_into(d_obj.data_ptr(), n, d_term.data_ptr(), 2.0, stream.cuda_stream)
                d_acc.add_(d_term, alpha=float(s[i]))

        out["caller_loop"] = row(loop)
        out["loop_over_instanced"] = round(out["caller_loop"]["ms"] / out["instanced"]["ms"], 4)
        out["loop_max_abs_difference"] = float((d_acc - one_launch).abs().max())
        out["inside_fraction"] = round(float((one_launch > 0.5).float().mean()), 4)
        out["contained_fraction"] = round(float((d_in >= 0).float().mean()), 4)

        m = min(n, EXACT_POINTS)
        out["exact"] = row(lambda: grid.winding_number_into(d_pts.data_ptr(), m, d_w.data_ptr(), d_in.data_ptr(), math.inf, stream.cuda_stream), m)
        out["unsigned"] = row(lambda: grid.closest_points_into(d_pts.data_ptr(), n, d_rec.data_ptr(), d_inst.data_ptr(), stream.cuda_stream))
        out["winding_signed"] = row(lambda: grid.winding_signed_distance_into(d_pts.data_ptr(), n, d_sd.data_ptr(), d_rec.data_ptr(),
                                                                              d_inst.data_ptr(), 2.0, stream.cuda_stream))
        out["winding_signed_over_unsigned"] = round(out["winding_signed"]["ms"] / out["unsigned"]["ms"], 4)
        out["negative_fraction"] = round(float((d_sd < 0).float().mean()), 4)
        grid.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

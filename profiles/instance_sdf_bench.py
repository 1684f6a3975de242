"""Instanced signed distance query cost (include/shader_ray_instance_sdf.h), one JSON line on stdout.

profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid, 2^20 near-surface world points (a
random triangle's centroid plus 1 % of the scene's extent of noise, mapped into a random instance) in Morton order, on the
device path:
  unsigned             InstanceSet.closest_points_into: stage 1 alone
  signed               InstanceSet.signed_distance_into with the caller's record and instance buffers
  signed_no_buffers    the same with neither (stage 1 into stream-ordered scratch, a chunk at a time)
  signed_over_unsigned the ratio: what the sign costs on top of the distance
and, from one blocking counting run over 2^12 of the same points, the sign walks' counters per hit beside those of cold walks
(+inf radius) of the same object points on the member scene: what the seed saves; and the same pair for 2^12 points away from
every surface (between the copies and up to two grid sizes around the grid).

Every time is the median of --trials runs after --warmup runs, bracketed by HIP events on the current torch stream.
Usage: python profiles/instance_sdf_bench.py [--trials 15] [--warmup 5] [--points 1048576]"""
import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms, morton_order, near_surface_points

F = np.float32
SAMPLE = 1 << 12


def main():
    ap = H.parser()
    ap.add_argument("--points", type=int, default=1 << 20)
    args = ap.parse_args()
    import torch
    import instance_ref

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = args.points
    median_ms = H.median_timer(args)

    def row(fn):
        return H.entry(median_ms(fn), "Mpoints_s", n, places=1, trials=False, points=n)

    with H.bunny_scene(pkg) as (world, bunny, positions):
        extent = float(np.ptp(positions.reshape(-1, 3).astype(np.float64), axis=0).max())
        M = grid_transforms((8, 8), 1.5 * extent, np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        pts = near_surface_points(positions, M, n, np.random.default_rng(2026))
        pts = pts[morton_order(pts[:, :3])]
        d_pts = torch.from_numpy(pts).cuda()
        d_rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
        d_sd = torch.empty(n, dtype=torch.float32, device="cuda")
        grid.signed_distance_into(d_pts.data_ptr(), 1, d_sd.data_ptr(), 0, 0, stream.cuda_stream)   # derive once, outside the timings

        out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "instances": grid.count,
               "triangles": len(positions) // 9, "closed": grid.closed()}
        out["unsigned"] = row(lambda: grid.closest_points_into(d_pts.data_ptr(), n, d_rec.data_ptr(), d_inst.data_ptr(), stream.cuda_stream))
        out["signed"] = row(lambda: grid.signed_distance_into(d_pts.data_ptr(), n, d_sd.data_ptr(), d_rec.data_ptr(), d_inst.data_ptr(),
                                                              stream.cuda_stream))
        kept = d_sd.clone()
        out["signed_no_buffers"] = row(lambda: grid.signed_distance_into(d_pts.data_ptr(), n, d_sd.data_ptr(), 0, 0, stream.cuda_stream))
        out["signed_over_unsigned"] = round(out["signed"]["ms"] / out["unsigned"]["ms"], 4)
        out["same_values_without_buffers"] = bool(torch.equal(kept.view(torch.int32), d_sd.view(torch.int32)))
        out["hit_fraction"] = round(float((d_inst >= 0).float().mean()), 4)
        out["inside_fraction"] = round(float((kept < 0).float().mean()), 4)

        # the seed: the sign walks' counters against cold walks of the same object points
        W = grid.world_to_object()
        keys = ("node_visits", "leaf_visits", "triangle_tests")

        def walks(sample, name):
            _, _, inst, c = grid.signed_distance(sample, closest=True, counters=True)
            hits = max(1, int((inst >= 0).sum()))
            p_o = np.concatenate([instance_ref.object_vectors(W[i], sample[inst == i, :3], True) for i in sorted(set(inst[inst >= 0].tolist()))])
            _, cold = bunny.closest_points(pkg.tracer.make_points(p_o), counters=True)
            out[f"sign_walk_per_hit{name}"] = {k: round(c[k] / hits, 2) for k in keys}
            out[f"cold_walk_per_hit{name}"] = {k: round(cold[k] / hits, 2) for k in keys}

        walks(pts[:: max(1, n // SAMPLE)][:SAMPLE], "")
        # and for points away from every surface: between the copies and around the grid, up to two grid sizes out
        rng = np.random.default_rng(7)
        lo, hi = pts[:, :3].min(0).astype(np.float64), pts[:, :3].max(0).astype(np.float64)
        away = np.full((SAMPLE, 4), np.inf, F)
        away[:, :3] = (lo + hi) / 2 + (rng.random((SAMPLE, 3)) * 2 - 1) * (hi - lo).max() * rng.choice([0.5, 1.0, 2.0], (SAMPLE, 1))
        walks(away, "_away")
        grid.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

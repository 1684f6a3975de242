"""Instanced within-radius query throughput (include/shader_ray_instance_near.h), one JSON line on stdout.

Rows, each on the device path with near-surface points (a random triangle's centroid plus 1 % of the scene's extent of noise,
mapped into a random instance) and radii of 2 % and 10 % of the unscaled scene's extent:
  a_identity     the bunny-class scene under one identity instance against Scene.triangles_within on the same points: the
                 cost of the layer (and whether the two wrote the same bytes)
  b_bunny_8x8    profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid
Both at K = 1, 8 and 64, with and without counts (without: the walk prunes by the K-th best).

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.  The walk counters per point (image-box bounds evaluated, leaf visits, triangle tests,
instance walks begun) come from one blocking counting run over 2^12 of the same points, and with them the mean near count.

Usage: python profiles/instance_near_bench.py [--trials 15] [--warmup 5] [--points 262144] [--out FILE]"""
import sys

import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms, near_surface_points

F = np.float32
SAMPLE = 1 << 12
KS = (1, 8, 64)
RADII = (0.02, 0.10)


def main():
    ap = H.parser()
    ap.add_argument("--points", type=int, default=1 << 18)
    args = ap.parse_args()
    import torch

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = args.points
    median_ms = H.median_timer(args, slow_ms=1000.0)

    def time_cell(fn):
        return H.entry(median_ms(fn), "Mpoints_s", n)

    def rows(s, plain, pts, extent, what):
        """per radius and K, with and without counts: the set's time and, with `plain` (a Scene), Scene.triangles_within's"""
        out = {}
        d_pts = torch.from_numpy(pts).cuda()
        for frac in RADII:
            d_pts[:, 3] = float(F(frac * extent) ** 2)
            host = pts[:SAMPLE].copy()
            host[:, 3] = F(frac * extent) ** 2
            _, _, cnt, c = s.triangles_within(host, max_near=0, counters=True)
            per = {key: round(c[key] / len(host), 2) for key in ("node_visits", "leaf_visits", "triangle_tests", "traversals")}
            per["near"] = round(float(cnt.mean()), 2)
            cell = {"per_point": per}
            for k in KS:
                d_out = torch.empty((n, k, 8), dtype=torch.int32, device="cuda")
                d_inst = torch.empty((n, k), dtype=torch.int32, device="cuda")
                d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
                for counts in (True, False):
                    r = time_cell(lambda: s.triangles_within_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_inst.data_ptr(),
                                                                  d_cnt.data_ptr() if counts else 0, k, stream.cuda_stream))
                    if plain is not None:
                        d_plain = torch.empty((n, k, 8), dtype=torch.int32, device="cuda")
                        p = time_cell(lambda: plain.triangles_within_into(d_pts.data_ptr(), n, d_plain.data_ptr(),
                                                                          d_cnt.data_ptr() if counts else 0, k, stream.cuda_stream))
                        r = {"instance": r, "scene": p, "instance_over_scene": round(r["ms"] / p["ms"], 3),
                             "same_bytes": bool(torch.equal(d_out, d_plain))}
                        del d_plain
                    cell[f"K{k}_{'counts' if counts else 'pruned'}"] = r
                    print(f"  {what}, radius {frac}, K = {k}, counts = {counts}: {r}", file=sys.stderr, flush=True)
                del d_out, d_inst, d_cnt
            out[f"radius_{frac}"] = cell
        return out

    out = {"trials": args.trials, "warmup": args.warmup, "points": n, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(2026)
    with H.bunny_scene(pkg) as (world, bunny, positions):
        extent = float(np.ptp(positions.reshape(-1, 3).astype(np.float64), axis=0).max())
        out["triangles"] = len(positions) // 9

        eye = np.eye(3, 4, dtype=F)[None]
        one = pkg.tracer.InstanceSet([bunny], eye)
        out["a_identity"] = rows(one, bunny, near_surface_points(positions, eye, n, rng), extent, "one identity instance")
        one.close()

        M = grid_transforms((8, 8), 1.5 * extent, np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        out["b_bunny_8x8"] = rows(grid, None, near_surface_points(positions, M, n, rng), extent, "64 copies")
        grid.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

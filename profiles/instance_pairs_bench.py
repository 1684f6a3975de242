"""Instance-pair collision matrix throughput (include/shader_ray_instance_pairs.h), one JSON line on stdout and in
profiles/instance_pairs_bench.json (--out).

Sets:
  a_bunny_8x8        profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid, 1.5 extents apart
  b_bunny_8x8_close  the same 64 maps with the grid pulled together to 0.45 extents, so that neighbours overlap
  c_tiny_301         the 301 instances of three tiny scenes of tests/test_gpu_instance_point.py (one workgroup per row)
Per set, each on the device path into buffers allocated once:
  any, any_upper     SHRAY_PAIRS_ANY, and with SHRAY_PAIRS_UPPER
  first_only         keys without counts (the form that skips by a cell's key)
  counts             keys and counts (the form that skips nothing)
  loop_any           what the library offered before: n launches of the instance form with SHRAY_INTERSECT_ANY |
                     SHRAY_INTERSECT_SKIP_OWN_INSTANCE, one per instance, into one int32 buffer, and the per-instance reduction
                     of it (which instance collides at all -- the loop cannot say with whom); `rows_equal` says whether the
                     matrix's rows reduce to the same booleans
  any_over_loop      the ratio of the medians, with the ratios of the extremes
  wall_ms            one blocking InstanceSet.collision_matrix() and one InstanceSet.instances_colliding(), host clock
  per_query_triangle the four counters of the counting form per query triangle, and the set cells

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.

Usage: python profiles/instance_pairs_bench.py [--trials 15] [--warmup 5] [--out FILE]"""
import os
import sys
import time

import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms

F = np.float32


def main():
    args = H.parser(out=os.path.join(H.ROOT, "profiles", "instance_pairs_bench.json")).parse_args()
    import torch

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    median_ms = H.median_timer(args, slow_ms=500.0)

    def time_cell(fn):
        return H.entry(median_ms(fn))

    def rows(s, what):
        n = s.count
        triangles = [s.triangle_count(i) for i in range(n)]
        starts = np.concatenate([[0], np.cumsum(triangles)]).astype(np.int64)
        first = torch.empty(n * n, dtype=torch.int64, device="cuda")
        counts = torch.empty(n * n, dtype=torch.int64, device="cuda")
        flags = torch.empty(int(starts[-1]), dtype=torch.int32, device="cuda")
        segment = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.as_tensor(triangles, device="cuda"))
        res = {"instances": n, "query_triangles": int(starts[-1])}
        sp = stream.cuda_stream
        res["any"] = time_cell(lambda: s.collision_pairs_into(0, counts.data_ptr(), any_only=True, stream_ptr=sp))
        matrix = counts.cpu().numpy().reshape(n, n) != 0
        res["any_upper"] = time_cell(lambda: s.collision_pairs_into(0, counts.data_ptr(), any_only=True, upper=True, stream_ptr=sp))
        res["first_only"] = time_cell(lambda: s.collision_pairs_into(first.data_ptr(), 0, stream_ptr=sp))
        res["counts"] = time_cell(lambda: s.collision_pairs_into(first.data_ptr(), counts.data_ptr(), stream_ptr=sp))
        full = counts.cpu().numpy().reshape(n, n)
        assert np.array_equal(full > 0, matrix)
        colliding = torch.zeros(n, dtype=torch.int32, device="cuda")

        def loop():
            for i in range(n):
                s.instance_intersections_into(i, 0, triangles[i], 0, 0, flags.data_ptr() + 4 * int(starts[i]), 0, True, False, True, sp)
            colliding.zero_()
            colliding.index_add_(0, segment, flags)
            return colliding.cpu()

        res["loop_any"] = time_cell(loop)
        res["rows_equal"] = bool(np.array_equal(loop().numpy() > 0, matrix.any(1)))
        a, b = res["any"], res["loop_any"]
        res["any_over_loop"] = {"ratio": round(a["ms"] / b["ms"], 4),
                                "range": [round(a["ms_min_max"][0] / b["ms_min_max"][1], 4), round(a["ms_min_max"][1] / b["ms_min_max"][0], 4)]}
        t0 = time.perf_counter()
        s.collision_matrix()
        t1 = time.perf_counter()
        s.instances_colliding()
        t2 = time.perf_counter()
        res["wall_ms"] = {"collision_matrix": round(1e3 * (t1 - t0), 3), "instances_colliding": round(1e3 * (t2 - t1), 3)}
        tally = s.collision_pairs(counters=True)[3]
        res["per_query_triangle"] = {k: round(tally[k] / max(tally["samples"], 1), 3) for k in ("node_visits", "leaf_visits", "triangle_tests",
                                                                                                "traversals")}
        res["set_cells"], res["colliding_instances"], res["pairs_total"] = int(matrix.sum()), int(matrix.any(1).sum()), int(full.sum())
        print(f"  {what}: {res}", file=sys.stderr, flush=True)
        return res

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    with H.bunny_scene(pkg) as (world, bunny, pos):
        extent = float(np.ptp(pos.reshape(-1, 3).astype(np.float64), axis=0).max())
        out["triangles"] = len(pos) // 9
        M = grid_transforms((8, 8), 1.5 * extent, np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        out["a_bunny_8x8"] = rows(grid, "64 copies, 1.5 extents apart")
        close = M.copy()
        close[:, :, 3] *= F(0.45 / 1.5)
        grid.update(close)
        out["b_bunny_8x8_close"] = rows(grid, "64 copies, 0.45 extents apart")
        grid.close()

    import test_gpu_instance_point as G
    names, maps, _ = G.the_set(pkg, "301 tiny instances")
    tiny = pkg.tracer.InstanceSet([G.member(pkg, x)[1] for x in names], maps)
    out["c_tiny_301"] = rows(tiny, "301 tiny instances")
    tiny.close()
    for _, sc in G._members.values():
        sc.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

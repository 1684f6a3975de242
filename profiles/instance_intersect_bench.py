"""Instanced triangle-intersection query throughput (include/shader_ray_instance_intersect.h), one JSON line on stdout.

Rows, each on the device path:
  a_identity          the bunny-class scene under one identity instance against Scene.intersecting_triangles on the same 2^18
                      queries: the cost of the layer (and whether the two wrote the same indices and counts)
  b_bunny_8x8         profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid, 2^18 queries
  c_collision_sweep   the instance form with SHRAY_INTERSECT_ANY | SHRAY_INTERSECT_SKIP_OWN_INSTANCE over every instance of an
                      8 x 8 grid of copies spaced at 0.45 of the scene's widest extent, so that neighbours interpenetrate: one
                      launch per instance, every triangle of every instance a query (InstanceSet.instances_colliding's work)
Rows a and b on two kinds of queries: "moved" (triangles of a moved copy of the scene, profiles/intersect_bench.py's, placed by
the map of a random instance: most miss, and most of what passes the vertex boxes is rejected by a later axis) and "slicers"
(random triangles of 2 % to 20 % of the unscaled scene's diagonal about points of the placed surfaces), in three forms each:
counts only (K = 0), K = 8 with counts, and SHRAY_INTERSECT_ANY.

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.  The walk counters per query (image-box tests, leaf visits, triangle tests, instance
walks begun) come from one blocking counting run over 2^12 of the same queries, and with them the mean count.

Usage: python profiles/instance_intersect_bench.py [--trials 15] [--warmup 5] [--queries 262144] [--out FILE]"""
import sys

import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms

F = np.float32
SAMPLE = 1 << 12
FORMS = (("counts_only", 0, False), ("K8_counts", 8, False), ("any", 0, True))
TALLIES = ("node_visits", "leaf_visits", "triangle_tests", "traversals")


def main():
    ap = H.parser()
    ap.add_argument("--queries", type=int, default=1 << 18)
    args = ap.parse_args()
    import torch
    import intersect_cases as TC

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = args.queries
    median_ms = H.median_timer(args, slow_ms=1000.0)

    def time_cell(fn, items):
        return H.entry(median_ms(fn), "Mqueries_s", items)

    def as_tensor(corners):
        return H.upload(pkg.tracer.make_triangles(corners), 12)

    def cells(s, plain, d_q, what):
        """per form: the set's time and, with `plain` (a Scene), Scene.intersecting_triangles' on the same queries"""
        cell = {}
        sample = d_q[torch.from_numpy(np.random.default_rng(5).permutation(len(d_q))[:SAMPLE]).cuda()].cpu().numpy()
        for name, any_only in (("counting", False), ("any", True)):
            _, _, cnt, c = s.intersecting_triangles(sample, max_triangles=0, counters=True, any_only=any_only)
            cell[f"per_query_{name}"] = {key: round(c[key] / len(sample), 2) for key in TALLIES}
            if not any_only:
                cell["n_mean"], cell["n_max"], cell["met"] = round(float(cnt.mean()), 2), int(cnt.max()), round(float((cnt > 0).mean()), 4)
        d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_inst = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        for name, k, any_only in FORMS:
            r = time_cell(lambda: s.intersecting_triangles_into(d_q.data_ptr(), n, d_out.data_ptr() if k else 0, d_inst.data_ptr() if k else 0,
                                                                d_cnt.data_ptr(), k, any_only, False, stream.cuda_stream), n)
            if plain is not None:
                d_plain = torch.empty((n, 8), dtype=torch.int32, device="cuda")
                d_plain_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
                p = time_cell(lambda: plain.intersecting_triangles_into(d_q.data_ptr(), n, d_plain.data_ptr() if k else 0,
                                                                        d_plain_cnt.data_ptr(), k, any_only, False, stream.cuda_stream), n)
                r = {"instance": r, "scene": p, "instance_over_scene": round(r["ms"] / p["ms"], 3),
                     "same_answer": bool(torch.equal(d_cnt, d_plain_cnt)) and (k == 0 or bool(torch.equal(d_out, d_plain)))}
                del d_plain, d_plain_cnt
            cell[name] = r
            print(f"  {what}, {name}: {r}", file=sys.stderr, flush=True)
        return cell

    def queries_of(positions, maps, extent, rng):
        """(moved-copy triangles, slicers) as [n, 12] tensors, for the scene's positions placed by `maps`"""
        tris = positions.reshape(-1, 3, 3)
        A = np.asarray(maps, np.float64)
        place = lambda corners, i: np.einsum("nrc,nkc->nkr", A[i][:, :, :3], corners.astype(np.float64)) + A[i][:, None, :, 3]
        moved = TC.moved_copy(tris, seed=2027)
        t, i = rng.integers(0, len(tris), n), rng.integers(0, len(maps), n)
        d_moved = as_tensor(place(moved[t], i))
        t, i = rng.integers(0, len(tris), n), rng.integers(0, len(maps), n)
        w = rng.random((n, 3))
        w /= w.sum(1, keepdims=True)
        on = place((tris[t] * w[:, :, None]).sum(1)[:, None, :], i)
        size = (0.02 + 0.18 * rng.random((n, 1, 1))) * extent
        d_slicers = as_tensor(on + 0.5 * size * rng.normal(size=(n, 3, 3)))
        return d_moved, d_slicers

    out = {"trials": args.trials, "warmup": args.warmup, "queries": n, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(2026)
    with H.bunny_scene(pkg) as (world, bunny, positions):
        verts = positions.reshape(-1, 3).astype(np.float64)
        extent = float(np.linalg.norm(verts.max(0) - verts.min(0)))
        triangles = len(positions) // 9
        out["triangles"] = triangles

        eye = np.eye(3, 4, dtype=F)[None]
        one = pkg.tracer.InstanceSet([bunny], eye)
        d_moved, d_slicers = queries_of(positions, eye, extent, rng)
        out["a_identity"] = {"moved": cells(one, bunny, d_moved, "one identity instance, moved copies"),
                             "slicers": cells(one, bunny, d_slicers, "one identity instance, slicers")}
        one.close()

        widest = float(np.ptp(verts, axis=0).max())
        M = grid_transforms((8, 8), 1.5 * widest, np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        d_moved, d_slicers = queries_of(positions, M, extent, rng)
        out["b_bunny_8x8"] = {"moved": cells(grid, None, d_moved, "64 copies, moved copies"),
                              "slicers": cells(grid, None, d_slicers, "64 copies, slicers")}
        grid.close()
        del d_moved, d_slicers

        M = grid_transforms((8, 8), 0.45 * widest, np.random.default_rng(2026))
        close = pkg.tracer.InstanceSet([bunny] * 64, M)
        d_cnt = torch.empty((64, triangles), dtype=torch.int32, device="cuda")

        def sweep():
            for i in range(64):
                close.instance_intersections_into(i, 0, triangles, 0, 0, d_cnt[i].data_ptr(), 0, True, False, True, stream.cuda_stream)

        r = time_cell(sweep, 64 * triangles)
        met = d_cnt.cpu().numpy() != 0
        r.update({"launches": 64, "queries": 64 * triangles, "spacing_over_widest_extent": 0.45, "instances_colliding": int(met.any(1).sum()),
                  "triangles_colliding": round(float(met.mean()), 4)})
        part = close.instance_intersections(27, max_triangles=0, first=0, count=SAMPLE)[2]
        r["instance_27_first_4096"] = {"n_mean": round(float(part.mean()), 2), "n_max": int(part.max()), "met": round(float((part > 0).mean()), 4)}
        out["c_collision_sweep"] = r
        print(f"  collision sweep: {r}", file=sys.stderr, flush=True)
        close.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

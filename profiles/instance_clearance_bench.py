"""Instanced triangle-distance query throughput (include/shader_ray_instance_clearance.h), one JSON line on stdout and in
profiles/instance_clearance_bench.json (--out).

Rows, each on the device path, with profiles/clearance_bench.py's queries: 2^18 query triangles near the surface (a scene
triangle shrunk and lifted off by up to 1 % of the diagonal) and 2^18 far ones (2 to 10 diagonals away), each mapped into a
random instance:
  a_identity     the bunny-class scene under one identity instance against Scene.triangle_distances on the same queries: the
                 cost of the layer, and whether the two wrote the same bytes
  b_bunny_8x8    profiles/instance_bench.py's 64 rotated and scaled bunny-class copies on an 8 x 8 grid
Per set:
  near_K1            max_dist2 = +inf, K = 1, no counts: the nearest triangle of any instance and its witnesses (the form that
                     prunes)
  near_K8_tol        max_dist2 = (2 % of the diagonal)^2, K = 8 with counts
  near_any_tol       the tolerance query (SHRAY_CLEARANCE_ANY) at the same max_dist2
  far_K1, far_any_tol   the far queries: +inf with K = 1, and the tolerance query (nothing is in reach)
  own_K1_skip        the instance form over every triangle of one instance: on the identity set without
                     SKIP_OWN_INSTANCE and with SKIP_SHARED (Scene.self_clearance's row), on the grid with SKIP_OWN_INSTANCE:
                     the nearest triangle of another instance, +inf, K = 1, no counts
  own_any_tol        the instance form's tolerance query: on the identity set SKIP_SHARED at (0.5 %)^2, on the grid
                     SKIP_OWN_INSTANCE at (2 %)^2

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.  Where max_dist2 is finite, n mean and the four walk counters per query (image-box
bounds evaluated, leaf visits, triangle tests, instance walks begun) come from one blocking counting run over 2^10 of the same
queries.

Usage: python profiles/instance_clearance_bench.py [--trials 15] [--warmup 5] [--queries 262144] [--out FILE]"""
import os
import sys

import numpy as np

import bench_harness as H
from bench_workloads import grid_transforms

F = np.float32
SAMPLE = 1 << 10


def main():
    ap = H.parser(out=os.path.join(H.ROOT, "profiles", "instance_clearance_bench.json"))
    ap.add_argument("--queries", type=int, default=1 << 18)
    args = ap.parse_args()
    import torch
    import intersect_cases as IC
    import intersect_ref as IR

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = args.queries
    median_ms = H.median_timer(args, slow_ms=500.0)

    def time_cell(fn, count):
        return H.entry(median_ms(fn), "Mqueries_s", count, queries=count)

    dev = lambda q: H.upload(IR.make_triangles(q), 12)   # noqa: E731

    def item_row(s, plain, queries, d_queries, k, md, counts, any_only, what):
        d_out = torch.empty((n, max(k, 1), 12), dtype=torch.int32, device="cuda")
        d_inst = torch.empty((n, max(k, 1)), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        r = time_cell(lambda: s.triangle_distances_into(d_queries.data_ptr(), n, d_out.data_ptr() if k else 0, d_inst.data_ptr() if k else 0,
                                                        d_cnt.data_ptr() if counts else 0, md, k, any_only, False, stream.cuda_stream), n)
        r["max_dist2"] = float(md)
        if counts:
            full = d_cnt.cpu().numpy()
            r["n_mean"], r["n_max"] = round(float(full.mean()), 3), int(full.max())
        if np.isfinite(md):
            c = s.triangle_distances(queries[:SAMPLE], md, max_pairs=k, counters=True, any_only=any_only)[-1]
            r["per_query"] = {key: round(c[key] / SAMPLE, 2) for key in ("node_visits", "leaf_visits", "triangle_tests", "traversals")}
        if plain is not None:
            d_plain = torch.empty((n, max(k, 1), 12), dtype=torch.int32, device="cuda")
            d_plain_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
            p = time_cell(lambda: plain.triangle_distances_into(d_queries.data_ptr(), n, d_plain.data_ptr() if k else 0,
                                                                d_plain_cnt.data_ptr() if counts else 0, md, k, any_only, False,
                                                                stream.cuda_stream), n)
            same = (not k or bool(torch.equal(d_out, d_plain))) and (not counts or bool(torch.equal(d_cnt, d_plain_cnt)))
            r = {"instance": r, "scene": p, "instance_over_scene": round(r["ms"] / p["ms"], 3), "same_bytes": same}
        print(f"  {what}: K = {k}, max_dist2 = {md}, counts = {counts}, any = {any_only}: {r}", file=sys.stderr, flush=True)
        return r

    def own_row(s, plain, instance, triangles, k, md, counts, any_only, skip_shared, skip_own, what):
        d_out = torch.empty((triangles, max(k, 1), 12), dtype=torch.int32, device="cuda")
        d_inst = torch.empty((triangles, max(k, 1)), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(triangles, dtype=torch.int32, device="cuda")
        r = time_cell(lambda: s.instance_clearance_into(instance, 0, triangles, d_out.data_ptr() if k else 0, d_inst.data_ptr() if k else 0,
                                                        d_cnt.data_ptr() if counts else 0, md, k, any_only, skip_shared, skip_own,
                                                        stream.cuda_stream), triangles)
        r["max_dist2"] = float(md)
        if counts:
            r["nonzero"] = round(float((d_cnt > 0).float().mean()), 4)
        if k:
            found = d_out[:, 0, 7] >= 0
            d2 = d_out[:, 0, 3].contiguous().view(torch.float32)
            r["found"] = round(float(found.float().mean()), 4)
            r["dist_min"] = float(d2[found].min().sqrt()) if bool(found.any()) else None
        if plain is not None:
            d_plain = torch.empty((triangles, max(k, 1), 12), dtype=torch.int32, device="cuda")
            d_plain_cnt = torch.empty(triangles, dtype=torch.int32, device="cuda")
            p = time_cell(lambda: plain.self_clearance_into(0, triangles, d_plain.data_ptr() if k else 0, d_plain_cnt.data_ptr() if counts else 0,
                                                            md, k, any_only, skip_shared, stream.cuda_stream), triangles)
            same = (not k or bool(torch.equal(d_out, d_plain))) and (not counts or bool(torch.equal(d_cnt, d_plain_cnt)))
            r = {"instance": r, "scene": p, "instance_over_scene": round(r["ms"] / p["ms"], 3), "same_bytes": same}
        print(f"  {what}: instance form, K = {k}, max_dist2 = {md}, any = {any_only}: {r}", file=sys.stderr, flush=True)
        return r

    out = {"trials": args.trials, "warmup": args.warmup, "queries": n, "device": torch.cuda.get_device_name(0)}
    with H.bunny_scene(pkg) as (world, bunny, pos):
        tris = pos.reshape(-1, 3, 3)
        T = len(tris)
        diagonal = IC.scene_extent(pos)
        extent = float(np.ptp(pos.reshape(-1, 3).astype(np.float64), axis=0).max())
        out["triangles"], out["diagonal"] = T, round(diagonal, 4)
        inf, tol, thin = F(np.inf), F((0.02 * diagonal) ** 2), F((0.005 * diagonal) ** 2)

        def queries_for(maps, seed):
            """clearance_bench.py's near and far triangles, each mapped (in double, rounded) into a random instance"""
            rng = np.random.default_rng(seed)
            base = tris[rng.integers(0, T, n)].astype(np.float64)
            centre = base.mean(1, keepdims=True)
            way = rng.normal(size=(n, 1, 3))
            way /= np.linalg.norm(way, axis=2, keepdims=True)
            near = centre + (base - centre) * 0.8 + way * diagonal * 0.01 * rng.random((n, 1, 1))
            far = centre + (base - centre) * 0.8 + way * diagonal * (2 + 8 * rng.random((n, 1, 1)))
            M = np.asarray(maps, np.float64)[rng.integers(0, len(maps), n)]
            place = lambda q: (np.einsum("nrc,nkc->nkr", M[:, :, :3], q) + M[:, None, :, 3]).astype(F)
            return place(near), place(far)

        def rows(s, plain, maps, seed, what, own_instance):
            near, far = queries_for(maps, seed)
            d_near, d_far = dev(near), dev(far)
            res = {}
            res["near_K1"] = item_row(s, plain, near, d_near, 1, inf, False, False, what)
            res["near_K8_tol"] = item_row(s, plain, near, d_near, 8, tol, True, False, what)
            res["near_any_tol"] = item_row(s, plain, near, d_near, 0, tol, True, True, what)
            res["far_K1"] = item_row(s, plain, far, d_far, 1, inf, False, False, what)
            res["far_any_tol"] = item_row(s, plain, far, d_far, 0, tol, True, True, what)
            if plain is not None:
                res["own_K1_skip"] = own_row(s, plain, 0, T, 1, inf, False, False, True, False, what)
                res["own_any_tol"] = own_row(s, plain, 0, T, 0, thin, True, True, True, False, what)
            else:
                res["own_instance"] = own_instance
                res["own_K1_skip"] = own_row(s, None, own_instance, T, 1, inf, False, False, False, True, what)
                res["own_any_tol"] = own_row(s, None, own_instance, T, 0, tol, True, True, False, True, what)
            return res

        eye = np.eye(3, 4, dtype=F)[None]
        one = pkg.tracer.InstanceSet([bunny], eye)
        out["a_identity"] = rows(one, bunny, eye, 3, "one identity instance", 0)
        one.close()

        M = grid_transforms((8, 8), 1.5 * extent, np.random.default_rng(2026))
        grid = pkg.tracer.InstanceSet([bunny] * 64, M)
        out["b_bunny_8x8"] = rows(grid, None, M, 4, "64 copies", 27)
        grid.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

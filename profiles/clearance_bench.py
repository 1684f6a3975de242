"""Triangle-distance query throughput (include/shader_ray_clearance.h), one JSON line on stdout.

Scene: the bunny-class scene.  Rows, each on the device path:
  near_K1            2^18 query triangles near the surface (a scene triangle shrunk and lifted off by up to 1 % of the
                     diagonal), max_dist2 = +inf, K = 1, no counts: the nearest scene triangle and its witnesses (the form
                     that prunes)
  near_K8_tol        the same queries, max_dist2 = (2 % of the diagonal)^2, K = 8 with counts
  near_any_tol       the tolerance query (SHRAY_CLEARANCE_ANY) at the same max_dist2
  far_K1, far_any_tol   2^18 queries 2 to 10 diagonals away: +inf with K = 1, and the tolerance query (nothing is in reach)
  self_K1_skip       the self form over every triangle with SKIP_SHARED, +inf, K = 1: the nearest triangle that is no neighbour
  self_any_skip_tol  the self form's tolerance query at (0.5 % of the diagonal)^2

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.  Where max_dist2 is finite, n mean (max) and the three walk counters per query (node
visits, i.e. box bounds evaluated, leaf visits, triangle tests, i.e. pairs whose features were evaluated) come from one
blocking counting run over 2^10 of the same queries; the rows with +inf have none (the walk that counts skips nothing there).

  torch_vs_K1   near_K1 on 2^10 of the queries against the restatement (tests/clearance_ref.py) brute force through TorchOps
                on the GPU (every query against every triangle: what a caller would write without this query), the ratio of
                the times and whether every dist2 and triangle agrees

Usage: python profiles/clearance_bench.py [--trials 15] [--warmup 5]"""
import ctypes as C
import sys
import time

import numpy as np

import bench_harness as H

F = np.float32
COUNT = 1 << 18
SAMPLE = 1 << 10


def main():
    args = H.parser().parse_args()
    import torch
    import clearance_ref as CR
    import intersect_cases as IC
    import intersect_ref as IR
    import point_query_ref as PQ

    pkg = H.load_package()
    N = pkg._native
    lib = N.load_clearance()
    stream = torch.cuda.current_stream()
    median_ms = H.median_timer(args, slow_ms=500.0)

    def entry(queries, t):
        return H.entry(t, "Mqueries_s", queries, queries=queries)

    def launcher(scene, d_queries, count, k, md, counts, any_only, skip, d_out, d_cnt):
        """the item form on d_queries, or with d_queries None the self form over the first `count` triangles"""
        op = pkg.tracer.clearance_params(k, md, any_only, skip)
        out, cnt = C.c_void_p(d_out.data_ptr() if k else None), C.c_void_p(d_cnt.data_ptr() if counts else None)

        def launch():
            if d_queries is None:
                N.check(lib.shray_clearance_self_device(scene._handle, C.byref(op), 0, count, out, cnt, C.c_void_p(stream.cuda_stream)))
            else:
                N.check(lib.shray_clearance_triangles_device(scene._handle, C.byref(op), C.c_void_p(d_queries.data_ptr()), count, out,
                                                             cnt, C.c_void_p(stream.cuda_stream)))
        return launch

    def row(scene, sample, d_queries, count, k, md, counts, any_only, skip):
        d_out = torch.empty((count, max(k, 1), 12), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(count, dtype=torch.int32, device="cuda")
        r = entry(count, median_ms(launcher(scene, d_queries, count, k, md, counts, any_only, skip, d_out, d_cnt)))
        r["max_dist2"] = float(md)
        if k:
            d2 = d_out[:, 0, 3].contiguous().view(torch.float32)
            found = d_out[:, 0, 7] >= 0
            r["found"] = round(float(found.float().mean()), 4)
            r["dist_mean"] = round(float(d2[found].sqrt().mean()), 6) if bool(found.any()) else None
        if counts:
            full = d_cnt.cpu().numpy()
            r["n_mean"], r["n_max"], r["nonzero"] = round(float(full.mean()), 3), int(full.max()), round(float((full > 0).mean()), 4)
        if np.isfinite(md):
            _, _, c = scene.triangle_distances(sample, md, max_pairs=k, counters=True, any_only=any_only, skip_shared=skip)
            r["per_query"] = {key: round(c[key] / len(sample), 2) for key in ("node_visits", "leaf_visits", "triangle_tests")}
        print(f"  K = {k}, max_dist2 = {md}, counts = {counts}, any = {any_only}, skip = {skip}: {r['ms']} ms", file=sys.stderr, flush=True)
        return r

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    with H.bunny_scene(pkg) as (world, scene, pos):
        tris = pos.reshape(-1, 3, 3)
        T = len(tris)
        diagonal = IC.scene_extent(pos)
        rng = np.random.default_rng(3)
        base = tris[rng.integers(0, T, COUNT)].astype(np.float64)
        centre = base.mean(1, keepdims=True)
        way = rng.normal(size=(COUNT, 1, 3))
        way /= np.linalg.norm(way, axis=2, keepdims=True)
        near = (centre + (base - centre) * 0.8 + way * diagonal * 0.01 * rng.random((COUNT, 1, 1))).astype(F)
        far = (centre + (base - centre) * 0.8 + way * diagonal * (2 + 8 * rng.random((COUNT, 1, 1)))).astype(F)
        d_near, d_far = H.upload(IR.make_triangles(near), 12), H.upload(IR.make_triangles(far), 12)
        inf, tol, thin = F(np.inf), F((0.02 * diagonal) ** 2), F((0.005 * diagonal) ** 2)
        pick = np.sort(np.random.default_rng(5).permutation(T)[:SAMPLE])
        res = {"triangles": T, "diagonal": round(diagonal, 4)}
        res["near_K1"] = row(scene, near[:SAMPLE], d_near, COUNT, 1, inf, False, False, False)
        res["near_K8_tol"] = row(scene, near[:SAMPLE], d_near, COUNT, 8, tol, True, False, False)
        res["near_any_tol"] = row(scene, near[:SAMPLE], d_near, COUNT, 0, tol, True, True, False)
        res["far_K1"] = row(scene, far[:SAMPLE], d_far, COUNT, 1, inf, False, False, False)
        res["far_any_tol"] = row(scene, far[:SAMPLE], d_far, COUNT, 0, tol, True, True, False)
        res["self_K1_skip"] = row(scene, tris[pick], None, T, 1, inf, False, False, True)
        res["self_any_skip_tol"] = row(scene, tris[pick], None, T, 0, thin, True, True, True)
        out["bunny"] = res

        # what a caller would write today: every query against every triangle, the restatement on torch tensors
        few = near[:SAMPLE]
        d_few = d_near[:SAMPLE].contiguous()
        d_out = torch.empty((SAMPLE, 1, 12), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(SAMPLE, dtype=torch.int32, device="cuda")
        ours = entry(SAMPLE, median_ms(launcher(scene, d_few, SAMPLE, 1, inf, False, False, False, d_out, d_cnt)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d2, _ = CR.pair_table(PQ.TorchOps("cuda"), few, pos, pairs=1 << 22)
        torch.cuda.synchronize()
        brute_ms = (time.perf_counter() - t0) * 1e3
        got = d_out.cpu().numpy()
        nearest = d2.argmin(1)   # (the first of equal minima: the lowest index)
        agree = bool(np.array_equal(got[:, 0, 3].view(F).view(np.uint32), d2[np.arange(SAMPLE), nearest].view(np.uint32)) and
                     np.array_equal(got[:, 0, 7], nearest.astype(np.int32)))
        out["torch_vs_K1"] = {"kernel": ours, "torch_ms": round(brute_ms, 1), "torch_over_kernel": round(brute_ms / ours["ms"], 1),
                              "dist2_and_triangle_agree": agree}
    H.emit(out, args)


if __name__ == "__main__":
    main()

"""Triangle-intersection query throughput (include/shader_ray_intersect.h), one JSON line on stdout.

Scenes: the bunny-class scene and the 1M-triangle OBJ.  Rows, each on the device path:
  self_any_skip      self-intersection over every triangle, SHRAY_INTERSECT_ANY | SHRAY_INTERSECT_SKIP_SHARED
  self_K8_skip       the same with K = 8 and counts
  self_K8            K = 8 and counts without SKIP_SHARED: every triangle finds itself and its neighbours
  moved_K8, moved_any      the scene against a moved copy of itself (rotated by 0.05 rad, shifted by 3 % of the diagonal)
  slicers_counts, slicers_K8, slicers_any   2^20 slicing triangles of about 5 % of the diagonal about random surface points

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream,
with the fastest and the slowest launch.  n mean (max) and the three walk counters per query (node visits, i.e. box tests
evaluated, leaf visits, triangle tests) come from one blocking counting run over 2^12 of the same queries.

  torch_vs_k8   K = 8 with counts on 2^12 slicers of the bunny-class scene against the restatement's arithmetic in plain fp32
                torch on the GPU (every query against every triangle: what a caller would write without this query), the
                ratio of the times and whether indices and counts agree

Usage: python profiles/intersect_bench.py [--trials 15] [--warmup 5] [--no-million]"""
import ctypes as C
import sys

import numpy as np

import bench_harness as H

F = np.float32
COUNT = 1 << 20
SAMPLE = 1 << 12


def torch_intersect(pos, queries, k, chunk=256):
    """the header's test in fp32 torch, every query [n, 12] against every triangle: (indices [n, k], counts [n])"""
    import torch
    tri = pos.reshape(-1, 3, 3)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    big = torch.iinfo(torch.int32).max

    def mn(x, y):
        return torch.where(x < y, x, y)

    def mx(x, y):
        return torch.where(x > y, x, y)

    def cross(x, y):
        return torch.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                            x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)

    def dot(x, y):
        return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]

    firsts, counts = [], []
    for s in range(0, len(queries), chunk):
        q = queries[s:s + chunk]
        p0, p1, p2 = q[:, None, 0:3], q[:, None, 4:7], q[:, None, 8:11]
        sep = ((mn(mn(a, b), c) > mx(mx(p0, p1), p2)) | (mx(mx(a, b), c) < mn(mn(p0, p1), p2))).any(2)
        q0, q1, q2 = p0 - p0, p1 - p0, p2 - p0
        v0, v1, v2 = a - p0, b - p0, c - p0
        f = (q1 - q0, q2 - q1, q0 - q2)
        e = (v1 - v0, v2 - v1, v0 - v2)
        nq, nt = cross(f[0], f[1]), cross(e[0], e[1])
        axes = [nq, nt] + [cross(f[i], e[j]) for i in range(3) for j in range(3)] + [cross(nq, f[i]) for i in range(3)] + \
            [cross(nt, e[j]) for j in range(3)]
        for A in axes:
            s0, s1, s2 = dot(A, v0), dot(A, v1), dot(A, v2)
            t0, t1, t2 = dot(A, q0), dot(A, q1), dot(A, q2)
            sep |= (mn(mn(s0, s1), s2) > mx(mx(t0, t1), t2)) | (mx(mx(s0, s1), s2) < mn(mn(t0, t1), t2))
        sep |= (nt == 0).all(-1)
        corners = q.reshape(-1, 3, 4)[:, :, :3]
        walked = torch.isfinite(corners).all(2).all(1) & ~(nq == 0).all(-1)[:, 0]
        member = ~sep & walked[:, None]
        index = torch.where(member, torch.arange(member.shape[1], device=member.device)[None], big)
        first = torch.sort(index, 1).values[:, :k]
        firsts.append(torch.where(first == big, -1, first).int())
        counts.append(member.sum(1).int())
    return torch.cat(firsts), torch.cat(counts)


def main():
    ap = H.parser()
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch
    import intersect_cases as IC
    import intersect_ref as IR

    pkg = H.load_package()
    N = pkg._native
    lib = N.load_intersect()
    stream = torch.cuda.current_stream()
    median_ms = H.median_timer(args, slow_ms=500.0)

    def entry(queries, t):
        return H.entry(t, "Mqueries_s", queries, queries=queries)

    def launcher(scene, d_queries, count, k, any_only, skip, d_out, d_cnt):
        """the item form on d_queries, or with d_queries None the self form over the first `count` triangles"""
        op = pkg.tracer.intersect_params(k, any_only, skip)
        out, cnt = C.c_void_p(d_out.data_ptr() if k else None), C.c_void_p(d_cnt.data_ptr())

        def launch():
            if d_queries is None:
                N.check(lib.shray_intersect_self_device(scene._handle, C.byref(op), 0, count, out, cnt, C.c_void_p(stream.cuda_stream)))
            else:
                N.check(lib.shray_intersect_triangles_device(scene._handle, C.byref(op), C.c_void_p(d_queries.data_ptr()), count, out,
                                                             cnt, C.c_void_p(stream.cuda_stream)))
        return launch

    def row(scene, sample, d_queries, count, k, any_only, skip):
        """one table row: the timed launches, and n and the counters per query from a counting run over `sample` (host
        triangles [<= 2^12, 3, 3]: of the same queries)"""
        d_out = torch.empty((count, 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(count, dtype=torch.int32, device="cuda")
        r = entry(count, median_ms(launcher(scene, d_queries, count, k, any_only, skip, d_out, d_cnt)))
        full = d_cnt.cpu().numpy()
        r["n_mean"], r["n_max"], r["nonzero"] = round(float(full.mean()), 3), int(full.max()), round(float((full > 0).mean()), 4)
        _, _, c = scene.intersecting_triangles(sample, max_triangles=k, counters=True, any_only=any_only, skip_shared=skip)
        r["per_query"] = {key: round(c[key] / len(sample), 2) for key in ("node_visits", "leaf_visits", "triangle_tests")}
        print(f"  K = {k}, any = {any_only}, skip = {skip}: {r['ms']} ms, n {r['n_mean']} ({r['n_max']})", file=sys.stderr, flush=True)
        return r

    def scene_cases(scene, pos):
        tris = pos.reshape(-1, 3, 3)
        T = len(tris)
        diagonal = IC.scene_extent(pos)
        pick = np.sort(np.random.default_rng(5).permutation(T)[:SAMPLE])
        res = {"self_any_skip": row(scene, tris[pick], None, T, 0, True, True),
               "self_K8_skip": row(scene, tris[pick], None, T, 8, False, True),
               "self_K8": row(scene, tris[pick], None, T, 8, False, False)}
        moved = IC.moved_copy(pos, seed=8)
        d_moved = H.upload(IR.make_triangles(moved), 12)
        res["moved_K8"] = row(scene, moved[pick], d_moved, T, 8, False, False)
        res["moved_any"] = row(scene, moved[pick], d_moved, T, 0, True, False)
        # slicing triangles of about 5 % of the diagonal (corners on a circle of that diameter) about random surface points
        rng = np.random.default_rng(3)
        t = rng.integers(0, T, COUNT)
        w = rng.random((COUNT, 3)).astype(F)
        w /= w.sum(1, keepdims=True)
        centre = (tris[t] * w[:, :, None]).sum(1)
        slicers = (unit_slicers(COUNT, 11) * (0.025 * diagonal) + centre[:, None, :]).astype(F)
        d_slicers = H.upload(IR.make_triangles(slicers), 12)
        some = slicers[:SAMPLE]
        res["slicers_counts"] = row(scene, some, d_slicers, COUNT, 0, False, False)
        res["slicers_K8"] = row(scene, some, d_slicers, COUNT, 8, False, False)
        res["slicers_any"] = row(scene, some, d_slicers, COUNT, 0, True, False)
        return res, d_slicers

    def unit_slicers(n, seed):
        """[n, 3, 3]: three corners on a unit circle in a random plane about 0"""
        rng = np.random.default_rng(seed)
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        w = np.cross(u, rng.normal(size=(n, 3)))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        angles = rng.random((n, 1)) * 2 * np.pi + np.array([[0.0, 2.1, 4.2]])
        return np.cos(angles)[:, :, None] * u[:, None, :] + np.sin(angles)[:, :, None] * w[:, None, :]

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    with H.bunny_scene(pkg) as (world, scene, pos):
        out["bunny"], d_slicers = scene_cases(scene, pos)
        out["bunny"]["triangles"] = len(pos) // 9

        # what a caller would write today: every query against every triangle in torch, on 2^12 of the slicers
        few = d_slicers[:SAMPLE].contiguous()
        d_pos = torch.from_numpy(pos).cuda()
        want, want_n = torch_intersect(d_pos, few, 8)
        got, got_n = scene.intersecting_triangles(few, max_triangles=8)
        d_out = torch.empty((len(few), 8), dtype=torch.int32, device="cuda")
        d_cnt = torch.empty(len(few), dtype=torch.int32, device="cuda")
        ours = entry(len(few), median_ms(launcher(scene, few, len(few), 8, False, False, d_out, d_cnt)))
        brute = entry(len(few), median_ms(lambda: torch_intersect(d_pos, few, 8)))
        out["torch_vs_k8"] = {"kernel": ours, "torch": brute, "torch_over_kernel": round(brute["ms"] / ours["ms"], 2),
                              "indices_agree": bool((got == want).all()), "counts_agree": bool((got_n == want_n).all())}

    if not args.no_million:
        dw = pkg.tracer.DeviceWorld(pkg.scenes.million_obj())
        pos = np.asarray(dw.flat_arrays()["vertex_positions"], F)
        out["million"], _ = scene_cases(dw.scene, pos)
        out["million"]["triangles"] = len(pos) // 9
        dw.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

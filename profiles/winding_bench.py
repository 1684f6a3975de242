"""Winding-number query cost (include/shader_ray_winding.h), one JSON line on stdout.

  (a) the derivation of the node records on the bunny-class scene and on the 1M-triangle OBJ: a winding query of one point
      right after a refit that marks the records stale, less the same query with them current
  (b) the bunny-class scene, 2^20 points near the surface (Morton order) and 2^20 points uniform in its box grown by 30 %
      (Morton order): winding numbers at beta = 2 and in the exact mode (beta = inf)
  (c) the near points: the winding-signed distance beside signed_distance (include/shader_ray_sdf.h)
  (d) for scale and accuracy: the generalized winding number in torch float64 on the GPU (every point against every triangle)
      of 2^12 of the near and 2^12 of the uniform points, and the largest |w - w64| of both modes on them

Every time is the median of --trials runs after --warmup runs ((d): of 3 runs), bracketed by HIP events on the current torch stream.
Usage: python profiles/winding_bench.py [--trials 15] [--warmup 5] [--no-million]"""
import math

import numpy as np

import bench_harness as H
from bench_workloads import morton_order, near_points

F = np.float32


def main():
    ap = H.parser()
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    median_ms = H.median_timer(args)

    def derivation(path):
        with H.scene_of(pkg, path) as (world, scene, pos):
            pos = pos.reshape(-1, 3)
            one = H.upload(pkg.tracer.make_points(pos[:1]), 4)
            out = torch.empty(1, dtype=torch.float32, device="cuda")
            query = lambda: scene.winding_number_into(one.data_ptr(), 1, out.data_ptr(), 2.0, stream.cuda_stream)   # noqa: E731
            stale = lambda: scene.refit(pos)   # noqa: E731  (blocking; the same positions, a new geometry generation)
            fresh, lo, hi, _ = median_ms(query, before=stale)
            cached = median_ms(query).ms
            nodes = len(scene.winding_data())
        return {"triangles": len(pos) // 3, "nodes": nodes, "derive_ms": round(fresh - cached, 4), "stale_query_ms": round(fresh, 4),
                "stale_ms_min_max": [round(lo, 4), round(hi, 4)], "current_query_ms": round(cached, 4)}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    out["derive_bunny"] = derivation(pkg.scenes.bunny_trisrc())
    if not args.no_million:
        out["derive_million"] = derivation(pkg.scenes.million_obj())

    with H.bunny_scene(pkg) as (world, scene, positions):
        v = positions.reshape(-1, 3)
        lo, hi = v.min(0), v.max(0)
        near = near_points(positions, 1 << 20, seed=1)
        uniform = ((lo + hi) / 2 + (np.random.default_rng(2).random((1 << 20, 3)) * 2 - 1) * 0.65 * (hi - lo)).astype(F)
        sets = {"near": near[morton_order(near)], "uniform": uniform[morton_order(uniform)]}
        n = 1 << 20
        d_w = torch.empty(n, dtype=torch.float32, device="cuda")
        d_sd = torch.empty(n, dtype=torch.float32, device="cuda")
        d_rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")

        def row(fn):
            return H.entry(median_ms(fn), "Mpoints_s", n, places=1, trials=False, points=n)

        tri = torch.from_numpy(positions.reshape(-1, 3, 3).astype(np.float64)).cuda()

        def winding64(q):
            w = torch.zeros(len(q), dtype=torch.float64, device="cuda")
            for s in range(0, len(q), 64):
                r = tri[None] - q[s:s + 64, None, None, :]
                a, b, c = r[:, :, 0], r[:, :, 1], r[:, :, 2]
                la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
                det = (a * torch.cross(b, c, dim=-1)).sum(-1)
                den = la * lb * lc + (a * b).sum(-1) * lc + (a * c).sum(-1) * lb + (b * c).sum(-1) * la
                w[s:s + 64] = torch.atan2(det, den).sum(1) / (2 * np.pi)
            return w

        for kind, p in sets.items():
            d_pts = H.upload(pkg.tracer.make_points(p), 4)
            for label, beta in (("beta2", 2.0), ("exact", math.inf)):
                out[f"winding_{label}_bunny_{kind}"] = row(lambda: scene.winding_number_into(d_pts.data_ptr(), n, d_w.data_ptr(), beta,
                                                                                              stream.cuda_stream))
            if kind == "near":
                out["signed_distance_bunny_near"] = row(lambda: scene.signed_distance_into(d_pts.data_ptr(), n, d_sd.data_ptr(), d_rec.data_ptr(),
                                                                                            stream.cuda_stream))
                out["winding_signed_bunny_near"] = row(lambda: scene.winding_signed_distance_into(d_pts.data_ptr(), n, d_sd.data_ptr(),
                                                                                                   d_rec.data_ptr(), 2.0, stream.cuda_stream))
            # (d) float64 on 2^12 of the points
            sub = p[:: n // 4096][:4096]
            q = torch.from_numpy(sub.astype(np.float64)).cuda()
            ms = median_ms(lambda: winding64(q), trials=3, warmup=0).ms
            w64 = winding64(q).cpu().numpy()
            acc = {"points": len(sub), "torch_float64_ms": round(ms, 3), "us_per_point": round(ms * 1e3 / len(sub), 3)}
            for label, beta in (("beta2", 2.0), ("exact", math.inf)):
                w = scene.winding_number(sub, beta=beta)
                acc[f"{label}_max_abs_err"] = float(np.abs(w - w64).max())
                acc[f"{label}_inside_agreement"] = float(((w > 0.5) == (w64 > 0.5)).mean())
            out[f"float64_bunny_{kind}_2^12"] = acc
        out["beta2_speedup_per_point_vs_float64"] = round((out["float64_bunny_near_2^12"]["torch_float64_ms"] / 4096)
                                                          / (out["winding_beta2_bunny_near"]["ms"] / n), 1)
    H.emit(out, args)


if __name__ == "__main__":
    main()

"""Signed distance query cost (include/shader_ray_sdf.h), one JSON line on stdout.

  (a) the derivation of the pseudonormals (weld, sorts, sums) on the bunny-class scene and on the 1M-triangle OBJ: a signed
      query of one point right after a refit that marks the sign data stale, less the same query with the sign data current
  (b) the bunny-class scene, 2^20 points near the surface in Morton order: signed queries (records kept, and not kept)
      against closest-point queries of the same points
  (c) for scale: the generalized winding number in torch float64 on the GPU (every point against every triangle, the solid
      angles of Van Oosterom and Strackee) of 2^12 near points on the bunny-class scene: what a caller without this query
      would write for the sign alone

Every time is the median of --trials runs after --warmup runs ((c): of 3 runs), bracketed by HIP events on the current torch stream.
Usage: python profiles/sdf_bench.py [--trials 15] [--warmup 5] [--no-million]"""
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
            query = lambda: scene.signed_distance_into(one.data_ptr(), 1, out.data_ptr(), 0, stream.cuda_stream)   # noqa: E731
            stale = lambda: scene.refit(pos)   # noqa: E731  (blocking; the same positions, a new geometry generation)
            fresh, lo, hi, _ = median_ms(query, before=stale)
            cached = median_ms(query).ms
            info = scene.surface_info()
        return {"triangles": len(pos) // 3, "derive_ms": round(fresh - cached, 4), "stale_query_ms": round(fresh, 4),
                "stale_ms_min_max": [round(lo, 4), round(hi, 4)], "current_query_ms": round(cached, 4), "surface": info}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    out["derive_bunny"] = derivation(pkg.scenes.bunny_trisrc())
    if not args.no_million:
        out["derive_million"] = derivation(pkg.scenes.million_obj())

    with H.bunny_scene(pkg) as (world, scene, positions):
        p = near_points(positions, 1 << 20, seed=1)
        p = p[morton_order(p)]
        d_pts = H.upload(pkg.tracer.make_points(p), 4)
        d_rec = torch.empty((len(p), 8), dtype=torch.int32, device="cuda")
        d_sd = torch.empty(len(p), dtype=torch.float32, device="cuda")
        n = len(p)
        scene.signed_distance_into(d_pts.data_ptr(), 1, d_sd.data_ptr(), 0, stream.cuda_stream)   # derive once, outside the timings

        def row(fn):
            return H.entry(median_ms(fn), "Mpoints_s", n, places=1, trials=False, points=n)

        out["unsigned_bunny_near"] = row(lambda: scene.closest_points_into(d_pts.data_ptr(), n, d_rec.data_ptr(), stream.cuda_stream))
        out["signed_bunny_near"] = row(lambda: scene.signed_distance_into(d_pts.data_ptr(), n, d_sd.data_ptr(), d_rec.data_ptr(),
                                                                           stream.cuda_stream))
        out["signed_no_records_bunny_near"] = row(lambda: scene.signed_distance_into(d_pts.data_ptr(), n, d_sd.data_ptr(), 0,
                                                                                      stream.cuda_stream))
        out["signed_over_unsigned"] = round(out["signed_bunny_near"]["ms"] / out["unsigned_bunny_near"]["ms"], 4)

        # (c) the torch float64 winding number of 2^12 points
        tri = torch.from_numpy(positions.reshape(-1, 3, 3).astype(np.float64)).cuda()
        q = torch.from_numpy(p[:: len(p) // 4096][:4096].astype(np.float64)).cuda()

        def winding():
            w = torch.zeros(len(q), dtype=torch.float64, device="cuda")
            for s in range(0, len(q), 64):
                r = tri[None] - q[s:s + 64, None, None, :]
                a, b, c = r[:, :, 0], r[:, :, 1], r[:, :, 2]
                la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
                det = (a * torch.cross(b, c, dim=-1)).sum(-1)
                den = la * lb * lc + (a * b).sum(-1) * lc + (a * c).sum(-1) * lb + (b * c).sum(-1) * la
                w[s:s + 64] = torch.atan2(det, den).sum(1) / (2 * np.pi)
            return w

        ms = median_ms(winding, trials=3, warmup=0).ms
        inside = (winding() > 0.5).cpu().numpy()
        sd = scene.signed_distance(q.float().cpu().numpy())
        out["torch_winding_bunny_2^12"] = {"points": len(q), "ms": round(ms, 3), "us_per_point": round(ms * 1e3 / len(q), 3),
                                           "sign_agreement": float((inside == (sd < 0)).mean())}
        out["signed_speedup_per_point_vs_winding"] = round((ms / len(q)) / (out["signed_bunny_near"]["ms"] / n), 1)
    H.emit(out, args)


if __name__ == "__main__":
    main()

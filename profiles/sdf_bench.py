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
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    from point_query_bench import morton_order, near_points

    pkg = load_package()
    stream = torch.cuda.current_stream()

    def timed(fn, before=None):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def median_ms(fn, before=None):
        for _ in range(args.warmup):
            timed(fn, before)
        times = [timed(fn, before) for _ in range(args.trials)]
        return float(np.median(times)), float(min(times)), float(max(times))

    def derivation(path):
        world = pkg.World(path)
        scene = pkg.Scene(world.flatten())
        pos = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1, 3)
        one = torch.from_numpy(pkg.tracer.make_points(pos[:1]).view(F).reshape(-1, 4).copy()).cuda()
        out = torch.empty(1, dtype=torch.float32, device="cuda")
        query = lambda: scene.signed_distance_into(one.data_ptr(), 1, out.data_ptr(), 0, stream.cuda_stream)   # noqa: E731
        stale = lambda: scene.refit(pos)   # noqa: E731  (blocking; the same positions, a new geometry generation)
        fresh, lo, hi = median_ms(query, stale)
        cached, _, _ = median_ms(query)
        info = scene.surface_info()
        scene.close()
        world.close()
        return {"triangles": len(pos) // 3, "derive_ms": round(fresh - cached, 4), "stale_query_ms": round(fresh, 4),
                "stale_ms_min_max": [round(lo, 4), round(hi, 4)], "current_query_ms": round(cached, 4), "surface": info}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    out["derive_bunny"] = derivation(pkg.scenes.bunny_trisrc())
    if not args.no_million:
        out["derive_million"] = derivation(pkg.scenes.million_obj())

    world = pkg.World(pkg.scenes.bunny_trisrc())
    scene = pkg.Scene(world.flatten())
    positions = np.asarray(world.arrays()["vertex_positions"], F)
    p = near_points(positions, 1 << 20, seed=1)
    p = p[morton_order(p)]
    d_pts = torch.from_numpy(pkg.tracer.make_points(p).view(F).reshape(-1, 4).copy()).cuda()
    d_rec = torch.empty((len(p), 8), dtype=torch.int32, device="cuda")
    d_sd = torch.empty(len(p), dtype=torch.float32, device="cuda")
    n = len(p)
    scene.signed_distance_into(d_pts.data_ptr(), 1, d_sd.data_ptr(), 0, stream.cuda_stream)   # derive once, outside the timings

    def row(fn):
        ms, lo, hi = median_ms(fn)
        return {"points": n, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "Mpoints_s": round(n / ms / 1e3, 1)}

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

    ms = float(np.median([timed(winding) for _ in range(3)]))
    inside = (winding() > 0.5).cpu().numpy()
    sd = scene.signed_distance(q.float().cpu().numpy())
    out["torch_winding_bunny_2^12"] = {"points": len(q), "ms": round(ms, 3), "us_per_point": round(ms * 1e3 / len(q), 3),
                                       "sign_agreement": float((inside == (sd < 0)).mean())}
    out["signed_speedup_per_point_vs_winding"] = round((ms / len(q)) / (out["signed_bunny_near"]["ms"] / n), 1)
    scene.close()
    world.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

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
import argparse
import json
import math
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
        query = lambda: scene.winding_number_into(one.data_ptr(), 1, out.data_ptr(), 2.0, stream.cuda_stream)   # noqa: E731
        stale = lambda: scene.refit(pos)   # noqa: E731  (blocking; the same positions, a new geometry generation)
        fresh, lo, hi = median_ms(query, stale)
        cached, _, _ = median_ms(query)
        nodes = len(scene.winding_data())
        scene.close()
        world.close()
        return {"triangles": len(pos) // 3, "nodes": nodes, "derive_ms": round(fresh - cached, 4), "stale_query_ms": round(fresh, 4),
                "stale_ms_min_max": [round(lo, 4), round(hi, 4)], "current_query_ms": round(cached, 4)}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    out["derive_bunny"] = derivation(pkg.scenes.bunny_trisrc())
    if not args.no_million:
        out["derive_million"] = derivation(pkg.scenes.million_obj())

    world = pkg.World(pkg.scenes.bunny_trisrc())
    scene = pkg.Scene(world.flatten())
    positions = np.asarray(world.arrays()["vertex_positions"], F)
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
        ms, lo_, hi_ = median_ms(fn)
        return {"points": n, "ms": round(ms, 4), "ms_min_max": [round(lo_, 4), round(hi_, 4)], "Mpoints_s": round(n / ms / 1e3, 1)}

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
        d_pts = torch.from_numpy(pkg.tracer.make_points(p).view(F).reshape(-1, 4).copy()).cuda()
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
        ms = float(np.median([timed(lambda: winding64(q)) for _ in range(3)]))
        w64 = winding64(q).cpu().numpy()
        acc = {"points": len(sub), "torch_float64_ms": round(ms, 3), "us_per_point": round(ms * 1e3 / len(sub), 3)}
        for label, beta in (("beta2", 2.0), ("exact", math.inf)):
            w = scene.winding_number(sub, beta=beta)
            acc[f"{label}_max_abs_err"] = float(np.abs(w - w64).max())
            acc[f"{label}_inside_agreement"] = float(((w > 0.5) == (w64 > 0.5)).mean())
        out[f"float64_bunny_{kind}_2^12"] = acc
    out["beta2_speedup_per_point_vs_float64"] = round((out["float64_bunny_near_2^12"]["torch_float64_ms"] / 4096)
                                                      / (out["winding_beta2_bunny_near"]["ms"] / n), 1)
    scene.close()
    world.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

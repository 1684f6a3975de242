"""Instanced all-hits ray queries (include/shader_ray_instance_multihit.h), one JSON line on stdout.  2^20 rays a case.

  (a) one identity instance of the bunny-class scene against Scene.trace_all_hits_into on the same rays: the instance layer's cost
  (b) 64 bunny-class copies on an 8 x 8 grid with random rotations and scales, rays looking down at the grid
  (c) 4096 copies of lobed_528 on a 16 x 16 x 16 grid
For each: the first 1, 4 and 8 crossings pruned (no counts), the same with counts, and counts only.  For (b) and (c) also what a
caller can do today: K InstanceSet.trace_rays calls, each re-started from the previous hit (time only: its answers are not
comparable at coincident surfaces), and Scene.trace_all_hits on rays the host moved into every instance's object space plus
the host's merge by the key (wall time, on --compose-rays rays, scaled to a ray); and the per-ray averages of the counting form.

Every device time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
Usage: python profiles/instance_multihit_bench.py [--trials 15] [--warmup 5] [--compose-rays 4096]"""
import os
import time

import numpy as np

import bench_harness as H
from bench_workloads import down_rays, grid_transforms, through_rays

F = np.float32


def main():
    ap = H.parser()
    ap.add_argument("--compose-rays", type=int, default=4096, help="rays of the host composition (it walks instances x rays rays)")
    args = ap.parse_args()
    import torch
    import instance_multi_hit_ref as IM
    import instance_ref as I

    pkg = H.load_package()
    rng = np.random.default_rng(2026)
    stream = torch.cuda.current_stream()
    n = 1 << 20

    median_ms = H.median_timer(args)

    def entry(t):
        ms = round(t.ms, 4)
        return {"ms": ms, "Mrays_s": round(n / ms / 1e3, 1)}

    def forms(target, d_rays, instanced):
        """first 1 / 4 / 8 pruned, with counts, and counts only, of a set (instanced) or a scene"""
        d_hits = torch.empty((n, 8, 4), dtype=torch.int32, device="cuda")
        d_inst = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_counts = torch.empty(n, dtype=torch.int32, device="cuda")

        def run(k, counts):
            c = d_counts.data_ptr() if counts else 0
            if instanced:
                target.trace_all_hits_into(d_rays.data_ptr(), n, d_hits.data_ptr() if k else 0, d_inst.data_ptr() if k else 0, c, k, stream.cuda_stream)
            else:
                target.trace_all_hits_into(d_rays.data_ptr(), n, d_hits.data_ptr() if k else 0, c, k, stream.cuda_stream)

        out = {}
        for k in (1, 4, 8):
            out[f"first_{k}_pruned"] = entry(median_ms(lambda: run(k, False)))
            out[f"first_{k}_counts"] = entry(median_ms(lambda: run(k, True)))
        out["counts_only"] = entry(median_ms(lambda: run(0, True)))
        torch.cuda.synchronize()
        return out

    def retraced(s, d_rays):
        """K InstanceSet.trace_rays calls re-started from the previous hit"""
        work = d_rays.clone()
        d_one = torch.empty((n, 4), dtype=torch.int32, device="cuda")

        def retrace(k):
            work.copy_(d_rays)
            for _ in range(k):
                s.trace_rays_into(work.data_ptr(), n, d_one.data_ptr(), 0, stream.cuda_stream, max_bvh_iterations=0)
                hit = d_one[:, 3] >= 0
                t = d_one[:, 0].view(torch.float32)
                work[:, 0:3] += work[:, 4:7] * t[:, None]                       # re-start from the hit point
                work[:, 3] = torch.where(hit, work[:, 3] - t, torch.zeros_like(t))   # a miss ends the ray (tmax 0: no walk)

        return {f"{k}_trace_rays_calls": entry(median_ms(lambda: retrace(k))) for k in (1, 4, 8)}

    def host_composition(s, sc, o, d, tmax, k):
        """per-scene trace_all_hits on host-moved rays plus the host merge: wall seconds a world ray (one distinct scene)"""
        m = min(args.compose_rays, len(o))
        o, d, tmax = o[:m], d[:m], np.broadcast_to(np.asarray(tmax, F), (len(o),))[:m]
        t0 = time.perf_counter()
        W = s.world_to_object()
        parts, total = [], np.zeros(m, np.int64)
        for at in range(0, s.count, 64):
            ids = range(at, min(at + 64, s.count))
            moved = np.concatenate([pkg.tracer.make_rays(*I.object_rays(W[i], o, d), tmax) for i in ids])
            hits, counts = sc.trace_all_hits(moved, max_hits=k, counts=True)
            for j, i in enumerate(ids):
                parts.append(IM.held_members(hits[j * m:(j + 1) * m], i))
                total += counts[j * m:(j + 1) * m]
        IM.first_k(*(np.concatenate(p) for p in zip(*parts)), tmax, k)
        seconds = time.perf_counter() - t0
        return {"rays": m, "K": k, "seconds": round(seconds, 3), "us_per_ray": round(1e6 * seconds / m, 2),
                "Mrays_s": round(m / seconds / 1e6, 4)}

    def per_ray(s, o, d, tmax):
        m = 1 << 16
        rays = pkg.tracer.make_rays(o[:m], d[:m], np.broadcast_to(np.asarray(tmax, F), (len(o),))[:m])
        _, _, counts, c = s.trace_all_hits(rays, max_hits=1, counters=True)
        return {"rays": m, "crossings": round(float(counts.mean()), 3), "crossings_max": int(counts.max()),
                "walks": round(c["traversals"] / m, 3), "node_visits": round(c["node_visits"] / m, 2),
                "leaf_visits": round(c["leaf_visits"] / m, 2), "triangle_tests": round(c["triangle_tests"] / m, 2)}

    def device_rays(o, d, tmax):
        return H.upload(pkg.tracer.make_rays(o, d, tmax), 8)

    out = {"trials": args.trials, "warmup": args.warmup, "rays": n, "device": torch.cuda.get_device_name(0)}

    # (a) -----------------------------------------------------------------------------------------------------------------
    world = pkg.World(pkg.scenes.bunny_trisrc())
    bunny = pkg.Scene(world.flatten())
    positions = np.asarray(world.arrays()["vertex_positions"], F)
    one = pkg.tracer.InstanceSet([bunny], np.eye(3, 4, dtype=F)[None])
    o, d, tmax = through_rays(positions, n, seed=14)
    d_rays = device_rays(o, d, tmax)
    out["a_identity"] = {"scene": forms(bunny, d_rays, False), "instance": forms(one, d_rays, True), "per_ray": per_ray(one, o, d, tmax)}
    one.close()

    # (b) -----------------------------------------------------------------------------------------------------------------
    corners = positions.reshape(-1, 3).astype(np.float64)
    extent = float(np.ptp(corners, axis=0).max())
    M = grid_transforms((8, 8), 1.5 * extent, rng)
    grid = pkg.tracer.InstanceSet([bunny] * 64, M)
    o, d = down_rays((M[:, :, 3].min(0) - extent).astype(np.float64), (M[:, :, 3].max(0) + extent).astype(np.float64), n, rng)
    d_rays = device_rays(o, d, F(1e7))
    out["b_bunny_8x8"] = {"instances": 64, **forms(grid, d_rays, True), **retraced(grid, d_rays),
                          "host_composition": host_composition(grid, bunny, o, d, F(1e7), 4), "per_ray": per_ray(grid, o, d, F(1e7))}
    grid.close()

    # (c) -----------------------------------------------------------------------------------------------------------------
    lobed_world = pkg.World(os.path.join(H.ROOT, "tests", "golden", "lobed_528.trisrc"))
    lobed = pkg.Scene(lobed_world.flatten())
    lp = np.asarray(lobed_world.arrays()["vertex_positions"], F).reshape(-1, 3)
    size = float(np.ptp(lp, axis=0).max())
    M = grid_transforms((16, 16, 16), 1.5 * size, rng)
    many = pkg.tracer.InstanceSet([lobed] * len(M), M)
    o, d = down_rays(M[:, :, 3].min(0) - size, M[:, :, 3].max(0) + size, n, rng)
    d_rays = device_rays(o, d, F(1e7))
    out["c_lobed_4096"] = {"instances": len(M), **forms(many, d_rays, True), **retraced(many, d_rays),
                           "host_composition": host_composition(many, lobed, o, d, F(1e7), 4), "per_ray": per_ray(many, o, d, F(1e7))}
    many.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

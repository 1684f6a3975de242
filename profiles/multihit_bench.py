"""All-hits ray query throughput (include/shader_ray_multihit.h), one JSON line on stdout.

Scenes: the bunny-class scene and the 1M-triangle OBJ.  Rays, 2^20 of each per scene:
  through  from a sphere around the scene aimed at points in its box (every ray crosses the box), in Morton order of the origin
  random   tests/test_gpu_ray_query.py's random rays (origins in twice the box, inside and on the mesh; mixed tmax)
Per scene and ray set:
  (i)   the first K crossings for K = 1, 4, 8, with counts (the walk that skips nothing) and without (the pruned walk)
  (ii)  trace_rays' closest hit (kernel id 0, no iteration cap) on the same rays: the yardstick
  (iii) what a caller did before: K successive trace_rays calls, each re-started from the previous hit (time only: its
        answers are not comparable at coincident surfaces)
Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
The counters per ray are those of the walk that skips nothing (one blocking counting run) and of the closest-hit walk.
Usage: python profiles/multihit_bench.py [--trials 15] [--warmup 5] [--no-million]"""
import bench_harness as H
from bench_workloads import morton_order, through_rays


def main():
    ap = H.parser()
    ap.add_argument("--no-million", action="store_true")
    args = ap.parse_args()
    import torch
    import ray_query_ref as R
    from test_gpu_ray_query import random_rays

    pkg = H.load_package()
    stream = torch.cuda.current_stream()
    n = 1 << 20
    median_ms = H.median_timer(args)

    def entry(t):
        return H.entry(t, "Mrays_s", n, places=1, trials=False)

    def case(scene, o, d, tmax):
        rays = pkg.tracer.make_rays(o, d, tmax)
        d_rays = H.upload(rays, 8)
        d_hits = torch.empty((n, 8, 4), dtype=torch.int32, device="cuda")
        d_counts = torch.empty(n, dtype=torch.int32, device="cuda")
        out = {}
        for k in (1, 4, 8):
            for with_counts in (True, False):
                out[f"first_{k}" + ("_with_counts" if with_counts else "")] = entry(median_ms(lambda: scene.trace_all_hits_into(
                    d_rays.data_ptr(), n, d_hits.data_ptr(), d_counts.data_ptr() if with_counts else 0, k, stream.cuda_stream)))
        out["counts_only"] = entry(median_ms(lambda: scene.trace_all_hits_into(d_rays.data_ptr(), n, 0, d_counts.data_ptr(), 0,
                                                                              stream.cuda_stream)))
        d_one = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        out["trace_rays_closest"] = entry(median_ms(lambda: scene.trace_rays_into(d_rays.data_ptr(), n, d_one.data_ptr(),
                                                                                 stream.cuda_stream, max_bvh_iterations=0)))
        work = torch.empty_like(d_rays)

        def retrace(k):
            work.copy_(d_rays)
            for _ in range(k):
                scene.trace_rays_into(work.data_ptr(), n, d_one.data_ptr(), stream.cuda_stream, max_bvh_iterations=0)
                hit = d_one[:, 3].view(torch.int32) >= 0
                t = torch.where(hit, d_one[:, 0], torch.zeros_like(d_one[:, 0]))
                work[:, 0:3] += work[:, 4:7] * t[:, None]                       # re-start from the hit point
                work[:, 3] = torch.where(hit, work[:, 3] - t, torch.zeros_like(t))   # a miss ends the ray (tmax 0: no walk)

        for k in (4, 8):
            out[f"retrace_{k}_calls"] = entry(median_ms(lambda: retrace(k)))
        _, counts, c = scene.trace_all_hits(rays, max_hits=0, counters=True)
        _, cc = scene.trace_rays(rays, max_bvh_iterations=0, counters=True)
        out["per_ray"] = {"crossings": round(float(counts.mean()), 3), "crossings_max": int(counts.max()),
                          "unpruned_node_visits": round(c["node_visits"] / n, 2), "unpruned_leaf_visits": round(c["leaf_visits"] / n, 2),
                          "unpruned_triangle_tests": round(c["triangle_tests"] / n, 2),
                          "closest_node_visits": round(cc["node_visits"] / n, 2), "closest_leaf_visits": round(cc["leaf_visits"] / n, 2),
                          "closest_triangle_tests": round(cc["triangle_tests"] / n, 2)}
        return out

    out = {"trials": args.trials, "warmup": args.warmup, "rays": n, "device": torch.cuda.get_device_name(0)}
    scenes = [("bunny", pkg.scenes.bunny_trisrc)] + ([] if args.no_million else [("million", pkg.scenes.million_obj)])
    for name, path in scenes:
        with H.scene_of(pkg, path()) as (world, scene, _):
            arrays = R.SceneArrays(world.arrays())
            scene.set_kernel(0)
            o, d, tmax = through_rays(arrays.positions, n, seed=2026)
            order = morton_order(o)
            out[name] = {"triangles": len(arrays.positions),
                         "through": case(scene, o[order], d[order], tmax[order]),
                         "random": case(scene, *random_rays(arrays, n, seed=2027))}
    H.emit(out, args)


if __name__ == "__main__":
    main()

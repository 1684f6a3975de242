"""Instanced ray queries (include/shader_ray_instance.h), one JSON line on stdout.

  (a) one identity instance of the bunny-class scene against Scene.trace_rays_into on the same rays: the headline frame's
      1920x1080 primary rays and 2^21 ambient-occlusion rays (profiles/ray_query_bench.py's buffers): the instance layer's cost
  (b) 64 bunny-class copies on an 8 x 8 grid with random rotations and scales, against one merged scene of the same 4.4M
      triangles created through DeviceWorld from a generated file: query time and device memory of each
  (c) 4096 copies of lobed_528 on a 16 x 16 x 16 grid
  (d) the wall time of InstanceSet.update at 4096 and 65,536 instances

Every query time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
Usage: python profiles/instance_bench.py [--trials 15] [--warmup 5] [--skip-merged]"""
import os
import tempfile
import time

import numpy as np

import bench_harness as H
from bench_workloads import ao_rays, camera_rays, down_rays, grid_transforms

F = np.float32


def main():
    ap = H.parser()
    ap.add_argument("--skip-merged", action="store_true", help="(b) without the merged 4.4M-triangle scene")
    args = ap.parse_args()
    import torch
    import bench
    import ray_query_ref as R

    pkg = H.load_package()
    rng = np.random.default_rng(2026)
    stream = torch.cuda.current_stream()

    timing = H.median_timer(args)

    def median_of(fn):
        return round(timing(fn).ms, 4)

    def device_rays(o, d, tmax):
        return H.upload(pkg.tracer.make_rays(o, d, tmax), 8)

    def time_set(s, d_rays):
        n = d_rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        inst = torch.empty(n, dtype=torch.int32, device="cuda")
        ms = median_of(lambda: s.trace_rays_into(d_rays.data_ptr(), n, hits.data_ptr(), inst.data_ptr(), stream.cuda_stream))
        torch.cuda.synchronize()
        return {"rays": n, "ms": ms, "Mrays_s": round(n / ms / 1e3, 1), "hit_fraction": round(float((hits[:, 3] >= 0).float().mean()), 4)}

    def time_scene(sc, d_rays):
        n = d_rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        ms = median_of(lambda: sc.trace_rays_into(d_rays.data_ptr(), n, hits.data_ptr(), stream.cuda_stream))
        torch.cuda.synchronize()
        return {"rays": n, "ms": ms, "Mrays_s": round(n / ms / 1e3, 1), "hit_fraction": round(float((hits[:, 3] >= 0).float().mean()), 4)}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    # (a) -----------------------------------------------------------------------------------------------------------------
    world = pkg.World(pkg.scenes.bunny_trisrc())
    W, HEIGHT = 1920, 1080
    params = bench.orbit_params(pkg, world, W, HEIGHT)[0]
    bunny = pkg.Scene(world.flatten())
    one = pkg.tracer.InstanceSet([bunny], np.eye(3, 4, dtype=F)[None])
    positions = np.asarray(world.arrays()["vertex_positions"], F)
    o, d = camera_rays(params, W, HEIGHT, R.xform)
    primary = device_rays(o, d, F(1e7))
    o, d, tmax = ao_rays(positions, 1 << 21, seed=2024)
    ao = device_rays(o, d, tmax)
    out["a_identity"] = {"primary": {"scene": time_scene(bunny, primary), "instance": time_set(one, primary)},
                         "ao": {"scene": time_scene(bunny, ao), "instance": time_set(one, ao)}}
    one.close()
    del primary, ao

    # (b) -----------------------------------------------------------------------------------------------------------------
    corners = positions.reshape(-1, 3).astype(np.float64)
    extent = float(np.ptp(corners, axis=0).max())
    M = grid_transforms((8, 8), 1.5 * extent, rng)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    grid = pkg.tracer.InstanceSet([bunny] * 64, M)
    torch.cuda.synchronize()
    set_bytes = free0 - torch.cuda.mem_get_info()[0]
    lo = (M[:, :, 3].min(0) - extent).astype(np.float64)
    hi = (M[:, :, 3].max(0) + extent).astype(np.float64)
    o, d = down_rays(lo, hi, 1 << 21, rng)
    grid_rays = device_rays(o, d, F(1e7))
    b = {"instances": 64, "triangles": 64 * len(corners) // 3, "set": time_set(grid, grid_rays),
         "set_device_bytes_beyond_one_bunny": int(set_bytes)}
    if not args.skip_merged:
        # the bunny-class mesh with shared vertices (scenes.bunny_class_trisrc's own), 64 times, mapped in double
        pos, tri = pkg.scenes.lobed_sphere_mesh(132, 264, bumpiness=0.22, ears=True)
        pos = np.asarray(pos, F).astype(np.float64)
        allv = np.concatenate([pos @ m[:, :3].astype(np.float64).T + m[:, 3] for m in M]).astype(F)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "merged_64.obj")
            t0 = time.perf_counter()
            pkg.scenes.write_obj(path, allv, np.concatenate([tri + k * len(pos) for k in range(64)]))
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            merged = pkg.tracer.DeviceWorld(path)
            torch.cuda.synchronize()
            merged_bytes = free0 - torch.cuda.mem_get_info()[0]
        b["merged"] = time_scene(merged.scene, grid_rays)
        b["merged_device_bytes"] = int(merged_bytes)
        b["merged_seconds"] = {"write_file": round(t1 - t0, 2), **{k: round(v, 3) for k, v in merged.seconds.items()}}
        merged.close()
    out["b_bunny_8x8"] = b
    grid.close()
    del grid_rays

    # (c) -----------------------------------------------------------------------------------------------------------------
    lobed_world = pkg.World(os.path.join(H.ROOT, "tests", "golden", "lobed_528.trisrc"))
    lobed = pkg.Scene(lobed_world.flatten())
    lp = np.asarray(lobed_world.arrays()["vertex_positions"], F).reshape(-1, 3)
    size = float(np.ptp(lp, axis=0).max())
    M = grid_transforms((16, 16, 16), 1.5 * size, rng)
    many = pkg.tracer.InstanceSet([lobed] * len(M), M)
    lo, hi = M[:, :, 3].min(0) - size, M[:, :, 3].max(0) + size
    o, d = down_rays(lo, hi, 1 << 21, rng)
    out["c_lobed_4096"] = {"instances": len(M), **time_set(many, device_rays(o, d, F(1e7)))}

    # (d) -----------------------------------------------------------------------------------------------------------------
    d_out = {}
    for n, dims in ((4096, (16, 16, 16)), (65536, (64, 32, 32))):
        M = grid_transforms(dims, 1.5 * size, rng)
        s = many if n == 4096 else pkg.tracer.InstanceSet([lobed] * n, M)
        times = []
        for _ in range(5):
            M2 = M.copy()
            M2[:, :, 3] += rng.normal(size=(n, 3)).astype(F) * F(0.1 * size)
            t0 = time.perf_counter()
            s.update(M2)
            times.append(time.perf_counter() - t0)
        d_out[str(n)] = {"update_ms_median": round(1e3 * float(np.median(times)), 2), "update_ms_min": round(1e3 * min(times), 2)}
        s.close()
    out["d_update"] = d_out
    H.emit(out, args)


if __name__ == "__main__":
    main()

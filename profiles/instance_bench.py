"""Instanced ray queries (include/shader_ray_instance.h), one JSON line on stdout.

  (a) one identity instance of the bunny-class scene against Scene.trace_rays_into on the same rays: the headline frame's
      1920x1080 primary rays and 2^21 ambient-occlusion rays (profiles/ray_query_bench.py's buffers): the instance layer's cost
  (b) 64 bunny-class copies on an 8 x 8 grid with random rotations and scales, against one merged scene of the same 4.4M
      triangles created through DeviceWorld from a generated file: query time and device memory of each
  (c) 4096 copies of lobed_528 on a 16 x 16 x 16 grid
  (d) the wall time of InstanceSet.update at 4096 and 65,536 instances

Every query time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
Usage: python profiles/instance_bench.py [--trials 15] [--warmup 5] [--skip-merged]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

F = np.float32


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def grid_transforms(dims, spacing, rng, scale=(0.6, 1.0)):
    cells = np.stack(np.meshgrid(*[np.arange(k) for k in dims], indexing="ij"), -1).reshape(-1, len(dims))
    M = np.zeros((len(cells), 3, 4))
    for i, c in enumerate(cells):
        M[i, :, :3] = rotation(rng) * rng.uniform(*scale)
        M[i, :len(c), 3] = c * spacing
    return M.astype(F)


def down_rays(lo, hi, n, rng):
    """rays from above the region's top, aimed at random points of its floor (a camera looking down at the grid)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    size = hi - lo
    o = lo + size * rng.random((n, 3))
    o[:, 2] = hi[2] + size.max()
    aim = lo + size * rng.random((n, 3))
    aim[:, 2] = lo[2]
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-merged", action="store_true", help="(b) without the merged 4.4M-triangle scene")
    args = ap.parse_args()
    import torch
    import bench
    import ray_query_ref as R
    from ray_query_bench import ao_rays, camera_rays
    from __graft_entry__ import load_package

    pkg = load_package()
    rng = np.random.default_rng(2026)
    stream = torch.cuda.current_stream()

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        times = []
        for _ in range(args.trials):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b))
        return round(float(np.median(times)), 4)

    def device_rays(o, d, tmax):
        rays = pkg.tracer.make_rays(o, d, tmax)
        return torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()

    def time_set(s, d_rays):
        n = d_rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        inst = torch.empty(n, dtype=torch.int32, device="cuda")
        ms = median_ms(lambda: s.trace_rays_into(d_rays.data_ptr(), n, hits.data_ptr(), inst.data_ptr(), stream.cuda_stream))
        torch.cuda.synchronize()
        return {"rays": n, "ms": ms, "Mrays_s": round(n / ms / 1e3, 1), "hit_fraction": round(float((hits[:, 3] >= 0).float().mean()), 4)}

    def time_scene(sc, d_rays):
        n = d_rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        ms = median_ms(lambda: sc.trace_rays_into(d_rays.data_ptr(), n, hits.data_ptr(), stream.cuda_stream))
        torch.cuda.synchronize()
        return {"rays": n, "ms": ms, "Mrays_s": round(n / ms / 1e3, 1), "hit_fraction": round(float((hits[:, 3] >= 0).float().mean()), 4)}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    # (a) -----------------------------------------------------------------------------------------------------------------
    world = pkg.World(pkg.scenes.bunny_trisrc())
    W, H = 1920, 1080
    params = bench.orbit_params(pkg, world, W, H)[0]
    bunny = pkg.Scene(world.flatten())
    one = pkg.tracer.InstanceSet([bunny], np.eye(3, 4, dtype=F)[None])
    positions = np.asarray(world.arrays()["vertex_positions"], F)
    o, d = camera_rays(params, W, H, R.xform)
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
    lobed_world = pkg.World(os.path.join(ROOT, "tests", "golden", "lobed_528.trisrc"))
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()

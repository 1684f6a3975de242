"""Refit against rebuild (include/shader_ray_refit.h), one JSON line on stdout.  For the bunny-class scene and the 1M-triangle
OBJ, loaded through the device-resident pipeline (tracer.DeviceWorld) and moved by a fixed seeded deformation (a twist about
the vertical axis with a radial bulge and 1 % seeded noise):

  (a) shray_scene_refit_device of the moved vertices (device tensors, the tree's triangle_vertices already resident): the
      whole blocking call, validation readback and final readback included
  (b) the full rebuild of the same vertices: shray_bvh_build_device, shray_flatten_device_tree, shray_scene_create_from_device
      (host arrays in, as DeviceWorld does; the new scene destroyed outside the timed span)
  (c) closest-hit primary rays of the headline view (bench.py's first orbit view, 1920x1080, framed on the mesh as loaded)
      on the refit scene and on the rebuilt one: what the refit's tree quality costs
  and sah_cost of both trees (the rebuilt one's by a refit of it to the vertices it was built on), and of the tree as loaded.

Times: median of --trials after --warmup, bracketed by HIP events on the current torch stream (the host-blocking calls (a)
and (b) also as host wall time).  Usage: python profiles/refit_bench.py [--trials 15] [--warmup 5]"""
import ctypes as C
import time

import numpy as np

import bench_harness as H
from bench_workloads import camera_rays

F = np.float32


def twist(vd, seed=7):
    p = vd[:, :3].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    c, ext = (lo + hi) / 2, float(np.max(hi - lo))
    q = p - c
    rng = np.random.default_rng(seed)
    ang = 0.6 * q[:, 1] / ext
    r = 1.0 + 0.15 * np.sin(3.0 * q[:, 1] / ext * np.pi) + 0.01 * rng.standard_normal(len(q))
    x = (q[:, 0] * np.cos(ang) - q[:, 2] * np.sin(ang)) * r
    z = (q[:, 0] * np.sin(ang) + q[:, 2] * np.cos(ang)) * r
    out = vd.copy()
    out[:, :3] = (np.stack([x, q[:, 1], z], 1) + c).astype(F)
    return out


def main():
    ap = H.parser()
    args = ap.parse_args()
    import torch
    import bench
    import ray_query_ref as RQ

    pkg = H.load_package()
    N = pkg._native
    hip = N.load_hip()
    stream = torch.cuda.current_stream()

    def median(fn):
        for _ in range(args.warmup):
            fn()
        gpu, wall = [], []
        for _ in range(args.trials):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(a.elapsed_time(b))
        return {"ms": round(float(np.median(gpu)), 4), "ms_min_max": [round(min(gpu), 4), round(max(gpu), 4)],
                "wall_ms": round(float(np.median(wall)), 4)}

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "scenes": []}
    W, HEIGHT = 1920, 1080
    for label, path in (("bunny-class trisrc", pkg.scenes.bunny_trisrc()), ("1M-triangle obj", pkg.scenes.million_obj())):
        world = pkg.tracer.DeviceWorld(path, pkg.scenes.environment_constant(), device=0)
        lib = N.load_host()
        tv, vdp, nt, nv = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int32(), C.c_int32()
        assert lib.shray_host_triangles(world._world_handle, C.byref(tv), C.byref(nt), C.byref(vdp), C.byref(nv)) == 0
        load_tv = np.ctypeslib.as_array(tv, shape=(3 * nt.value,)).copy()
        vd = np.ctypeslib.as_array(vdp, shape=(9 * nv.value,)).reshape(-1, 9).copy()
        moved = twist(vd)
        d_moved = torch.from_numpy(moved).cuda()
        loaded_stats = world.refit(vd)                # the tree as built (and the tree's triangle_vertices uploaded, once)
        row = {"scene": label, "triangles": nt.value, "sah_cost_loaded": round(loaded_stats["sah_cost"], 4)}
        row["a_refit_device"] = median(lambda: world.refit(d_moved, stream.cuda_stream))
        refit_stats = world.refit(d_moved, stream.cuda_stream)

        # (b) the full rebuild of the same vertices
        m_tv = load_tv.ctypes.data_as(C.POINTER(C.c_int32))
        m_vd = np.ascontiguousarray(moved)
        options = pkg.host.bvh_options_from_environment()
        options.struct_size = C.sizeof(N.BvhOptions)
        handles = []

        def rebuild():
            tree, flat, scene = C.c_void_p(), C.c_void_p(), C.c_void_p()
            N.check(hip.shray_bvh_build_device(m_tv, nt, m_vd.ctypes.data_as(C.POINTER(C.c_float)), nv, 9, C.byref(options), C.byref(tree)))
            N.check(hip.shray_flatten_device_tree(tree, 2048, C.byref(flat)))
            N.check(hip.shray_scene_create_from_device(tree, flat, C.byref(scene)))
            handles.append((tree, flat, scene))

        def drain():
            torch.cuda.synchronize()
            while handles:
                tree, flat, scene = handles.pop()
                hip.shray_scene_destroy(scene)
                hip.shray_device_flat_destroy(flat)
                hip.shray_device_tree_destroy(tree)

        times = []
        for k in range(args.warmup + args.trials):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rebuild()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
            drain()
        row["b_rebuild"] = {"wall_ms": round(float(np.median(times)), 4), "wall_ms_min_max": [round(min(times), 4), round(max(times), 4)]}
        rebuild()
        tree, flat, handle = handles.pop()
        rebuilt_scene = pkg.Scene.__new__(pkg.Scene)
        rebuilt_scene._lib, rebuilt_scene._handle = hip, handle
        rebuilt_scene.set_environment(pkg.scenes.environment_constant())
        # the rebuilt tree's SAH cost: a refit of it to the very vertices it was built on leaves it as it is
        dtree = N.TreeDesc()
        N.check(hip.shray_device_tree_download(tree, C.byref(dtree), None))
        post_tv = np.ctypeslib.as_array(dtree.triangle_vertices, shape=(3 * nt.value,)).copy()
        rebuilt_stats = rebuilt_scene.refit(m_vd, post_tv, normal_offset=6)
        hip.shray_device_flat_destroy(flat)
        hip.shray_device_tree_destroy(tree)

        # (c) primary rays of the headline view on both scenes
        params = bench.orbit_params(pkg, world, W, HEIGHT)[0]
        o, d = camera_rays(params, W, HEIGHT, RQ.xform)
        rays = H.upload(pkg.tracer.make_rays(o, d, F(1e7)), 8)
        hits = torch.empty((W * HEIGHT, 4), dtype=torch.int32, device="cuda")
        for key, sc in (("c_primary_refit", world.scene), ("c_primary_rebuilt", rebuilt_scene)):
            row[key] = median(lambda: sc.trace_rays_into(rays.data_ptr(), W * HEIGHT, hits.data_ptr(), stream.cuda_stream))
            torch.cuda.synchronize()
            row[key]["hit_fraction"] = round(float((hits[:, 3] >= 0).float().mean().item()), 4)
        row["sah_cost_refit"] = round(refit_stats["sah_cost"], 4)
        row["sah_cost_rebuilt"] = round(rebuilt_stats["sah_cost"], 4)
        row["exact_div_ok"] = [refit_stats["exact_div_ok"], rebuilt_stats["exact_div_ok"]]
        out["scenes"].append(row)
        rebuilt_scene.close()
        world.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

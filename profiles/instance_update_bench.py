"""The device update of an instance set (shray_instance_set_update_device) against the host update, one JSON line on stdout.

  (a) at 64, 4096, 65,536 and 2^20 copies of lobed_528 on a grid: the wall time of the host update (InstanceSet.update with a
      numpy array, which waits for the device and uploads) and the device time of the device update (InstanceSet.update_into
      on the current torch stream, bracketed by HIP events), each the median of --trials after --warmup; and whether the two
      built the same set (top-level nodes and records, bit for bit)
  (b) one animation step at 4096 instances: refit a member scene, update the set, trace 2^21 rays, all on one stream, with
      the device update against the host update

Usage: python profiles/instance_update_bench.py [--trials 10] [--warmup 3] [--sizes 64,4096,65536,1048576]
       python profiles/instance_update_bench.py --trace-only   (device updates at 65,536 instances only, for a trace)"""
import ctypes as C
import json
import os
import time

import numpy as np

import bench_harness as H

F = np.float32
GRIDS = {64: (4, 4, 4), 4096: (16, 16, 16), 65536: (64, 32, 32), 1 << 20: (128, 128, 64)}


def transforms(dims, spacing, rng):
    """one instance per grid cell: a random rotation times a scale in [0.6, 1], at the cell (vectorised)"""
    cells = np.stack(np.meshgrid(*[np.arange(k) for k in dims], indexing="ij"), -1).reshape(-1, 3)
    q = rng.normal(size=(len(cells), 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = np.zeros((len(cells), 3, 4))
    M[:, :, :3] = R * rng.uniform(0.6, 1.0, (len(cells), 1, 1))
    M[:, :, 3] = cells * spacing
    return M.astype(F)


def set_arrays(s):
    count = C.c_int32()
    s._lib.shrayi_instance_set_arrays(s._handle, None, None, C.byref(count))
    nodes = np.zeros((count.value, 8), np.uint32)
    records = np.zeros((4 * s.count, 4), np.uint32)
    s._lib.shrayi_instance_set_arrays(s._handle, nodes.ctypes.data_as(C.c_void_p), records.ctypes.data_as(C.c_void_p), None)
    return nodes, records


def main():
    ap = H.parser(trials=10, warmup=3)
    ap.add_argument("--sizes", default="64,4096,65536,1048576")
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import torch

    pkg = H.load_package()
    rng = np.random.default_rng(2026)
    stream = torch.cuda.current_stream()
    world = pkg.World(os.path.join(H.ROOT, "tests", "golden", "lobed_528.trisrc"))
    lobed = pkg.Scene(world.flatten())
    lp = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1, 3)
    size = float(np.ptp(lp, axis=0).max())

    timing = H.median_timer(args)

    def events_ms(fn):
        return round(timing(fn).ms, 4)

    def moved(M):
        M2 = M.copy()
        M2[:, :, 3] += rng.normal(size=(len(M), 3)).astype(F) * F(0.1 * size)
        return M2

    if args.trace_only:
        M = transforms(GRIDS[65536], 1.5 * size, rng)
        s = pkg.tracer.InstanceSet([lobed] * len(M), M)
        d = [torch.from_numpy(moved(M)).cuda() for _ in range(4)]
        torch.cuda.synchronize()
        for k in range(8):
            s.update_into(d[k % 4].data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        print(json.dumps({"trace_only": True, "instances": len(M), "updates": 8, "status": s.update_status()}))
        return

    out = {"trials": args.trials, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    a = {}
    for n in (int(v) for v in args.sizes.split(",")):
        M = transforms(GRIDS[n], 1.5 * size, rng)
        t0 = time.perf_counter()
        s = pkg.tracer.InstanceSet([lobed] * n, M)
        ref = pkg.tracer.InstanceSet([lobed] * n, M)
        create_s = time.perf_counter() - t0
        host_M = [moved(M) for _ in range(2)]
        d_M = [torch.from_numpy(m).cuda() for m in host_M]
        host_times = []
        for k in range(args.warmup + args.trials):
            t0 = time.perf_counter()
            ref.update(host_M[k % 2])
            if k >= args.warmup:
                host_times.append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
        flip = [0]

        def device_update():
            s.update_into(d_M[flip[0] % 2].data_ptr(), stream.cuda_stream)
            flip[0] += 1
        ms = events_ms(device_update)
        # the enqueue alone (the host cost of a device update), and the equality of the two built sets
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.update_into(d_M[0].data_ptr(), stream.cuda_stream)
        enqueue_ms = 1e3 * (time.perf_counter() - t0)
        ref.update(host_M[0])
        assert s.update_status() == -1
        equal = all(np.array_equal(x, y) for x, y in zip(set_arrays(s), set_arrays(ref)))
        a[str(n)] = {"host_update_ms": round(float(np.median(host_times)), 3), "device_update_ms": ms,
                     "device_enqueue_ms": round(enqueue_ms, 3), "speedup": round(float(np.median(host_times)) / ms, 2),
                     "same_set": equal, "create_s": round(create_s, 2)}
        s.close()
        ref.close()
        del d_M
    out["a_update"] = a

    # (b) refit -> update -> trace, one stream ----------------------------------------------------------------------------------
    own = pkg.Scene(world.flatten())
    corners = own.geometry()["vertex_positions"].reshape(-1, 3)
    d_corners = [torch.from_numpy(np.ascontiguousarray(corners * F(1.0 + 0.01 * k))).cuda() for k in range(2)]
    M = transforms(GRIDS[4096], 1.5 * size, rng)
    members = [own if i % 8 == 0 else lobed for i in range(len(M))]
    s = pkg.tracer.InstanceSet(members, M)
    ref = pkg.tracer.InstanceSet(members, M)
    lo, hi = M[:, :, 3].min(0) - size, M[:, :, 3].max(0) + size
    nr = 1 << 21
    o = (lo + (hi - lo) * rng.random((nr, 3))).astype(F)
    o[:, 2] = hi[2] + 2 * size
    aim = lo + (hi - lo) * rng.random((nr, 3))
    aim[:, 2] = lo[2]
    dvec = aim - o
    dvec = (dvec / np.linalg.norm(dvec, axis=1, keepdims=True)).astype(F)
    rays = pkg.tracer.make_rays(o, dvec, F(1e7))
    d_rays = H.upload(rays, 8)
    hits = torch.empty((nr, 4), dtype=torch.int32, device="cuda")
    inst = torch.empty(nr, dtype=torch.int32, device="cuda")
    d_M = torch.from_numpy(M).cuda()
    step = [0]

    def device_step():
        own.refit(d_corners[step[0] % 2], stream_ptr=stream.cuda_stream)
        s.update_into(d_M.data_ptr(), stream.cuda_stream)
        s.trace_rays_into(d_rays.data_ptr(), nr, hits.data_ptr(), inst.data_ptr(), stream.cuda_stream)
        step[0] += 1

    def host_step():
        own.refit(d_corners[step[0] % 2], stream_ptr=stream.cuda_stream)
        ref.update(M)
        ref.trace_rays_into(d_rays.data_ptr(), nr, hits.data_ptr(), inst.data_ptr(), stream.cuda_stream)
        step[0] += 1

    def trace_only():
        s.trace_rays_into(d_rays.data_ptr(), nr, hits.data_ptr(), inst.data_ptr(), stream.cuda_stream)
    out["b_step_4096"] = {"rays": nr, "device_update_step_ms": events_ms(device_step),
                          "host_update_step_ms": events_ms(host_step),
                          "trace_alone_ms": events_ms(trace_only)}
    s.close()
    ref.close()
    own.close()
    H.emit(out, args)


if __name__ == "__main__":
    main()

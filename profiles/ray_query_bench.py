"""Ray-query throughput on the bunny-class scene (include/shader_ray_query.h), one JSON line on stdout.

  (a) the headline frame's 1920x1080 primary rays (bench.py's first orbit view) as an explicit ray buffer, closest hit;
      beside it, shray_render_device of the same frame (1 spp, the same rays plus the bounces and the shading)
  (b) 2^21 incoherent rays: seeded points on the surface, cosine-distributed directions about the surface normal,
      tmax = a tenth of the scene's extent (ambient-occlusion-like), closest hit
  (c) (b) as any-hit

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
Usage: python profiles/ray_query_bench.py [--kernel 0|1] [--trials 15] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

F = np.float32


def camera_rays(params, width, height, xform):
    """the 1-spp pixel-centre rays of trace_pixels in object space, float32 (row 0 = the bottom row)"""
    px, py = np.meshgrid(np.arange(width, dtype=F), np.arange(height, dtype=F))
    u = (px.reshape(-1) + F(0.5)) / F(width)
    v = (py.reshape(-1) + F(0.5)) / F(height)
    ipw, aspect = F(params.image_plane_width), F(params.aspect)
    eye = np.stack([ipw * (u - F(0.5)), ipw * (v - F(0.5)) * aspect, np.full_like(u, F(-1))], axis=1)
    eye = eye / np.sqrt((eye * eye).sum(1, dtype=F), dtype=F)[:, None]
    origin = xform(params.camera_matrix, np.zeros((1, 3), F), 1.0)
    d = xform(params.camera_normal_matrix, eye, 0.0)
    d = d / np.sqrt((d * d).sum(1, dtype=F), dtype=F)[:, None]
    return np.repeat(xform(params.object_matrix, origin, 1.0), len(d), axis=0), xform(params.object_normal_matrix, d, 0.0)


def ao_rays(positions, n, seed):
    """points on the surface (uniform over triangles' area), cosine-distributed directions about the geometric normal
    (its side chosen at random), the origin lifted off the surface by 1e-4 of the scene's extent"""
    rng = np.random.default_rng(seed)
    tri = positions.reshape(-1, 3, 3).astype(np.float64)
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.linalg.norm(cross, axis=1)
    k = rng.choice(len(tri), n, p=area / area.sum())
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    p = tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])
    nrm = cross[k] / np.maximum(area[k], 1e-30)[:, None]
    nrm *= np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
    # a cosine-weighted direction in the normal's frame
    r1, r2 = rng.random(n), rng.random(n)
    phi, s = 2 * np.pi * r1, np.sqrt(r2)
    t1 = np.cross(nrm, np.where(np.abs(nrm[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]]))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    d = t1 * (s * np.cos(phi))[:, None] + t2 * (s * np.sin(phi))[:, None] + nrm * np.sqrt(1 - r2)[:, None]
    extent = float(np.linalg.norm(tri.reshape(-1, 3).max(0) - tri.reshape(-1, 3).min(0)))
    return (p + nrm * 1e-4 * extent).astype(F), d.astype(F), F(extent / 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    import ray_query_ref as R
    from __graft_entry__ import load_package

    pkg = load_package()
    world = pkg.World(pkg.scenes.bunny_trisrc())
    W, H = 1920, 1080
    params = bench.orbit_params(pkg, world, W, H)[0]
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048))
    scene.set_kernel(args.kernel)
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
        return float(np.median(times)), float(min(times)), float(max(times))

    def device_rays(o, d, tmax):
        rays = pkg.tracer.make_rays(o, d, tmax)
        return torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()

    def query(d_rays, any_hit=False):
        d_hits = torch.empty((d_rays.shape[0], 4), dtype=torch.int32, device="cuda")
        fn = lambda: scene.trace_rays_into(d_rays.data_ptr(), d_rays.shape[0], d_hits.data_ptr(), stream.cuda_stream, any_hit=any_hit)
        ms = median_ms(fn)
        torch.cuda.synchronize()
        hit_fraction = float((d_hits[:, 3] >= 0).float().mean().item())
        return ms, hit_fraction

    out = {"scene": "bunny-class trisrc (69,168 triangles)", "kernel": args.kernel, "trials": args.trials, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    o, d = camera_rays(params, W, H, R.xform)
    ra = device_rays(o, d, F(1e7))
    (ms, lo, hi), frac = query(ra)
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    rms, rlo, rhi = median_ms(lambda: scene.render_into(params, W, H, 1, frame.data_ptr(), stream.cuda_stream, None))
    out["a_primary_closest"] = {"rays": W * H, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                                "Mrays_s": round(W * H / ms / 1e3, 1), "hit_fraction": round(frac, 4),
                                "render_ms": round(rms, 4), "render_ms_min_max": [round(rlo, 4), round(rhi, 4)]}
    n = 1 << 21
    o, d, tmax = ao_rays(np.asarray(world.arrays()["vertex_positions"], F), n, seed=2024)
    rb = device_rays(o, d, tmax)
    for key, any_hit in (("b_ao_closest", False), ("c_ao_any", True)):
        (ms, lo, hi), frac = query(rb, any_hit)
        out[key] = {"rays": n, "tmax": float(tmax), "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                    "Mrays_s": round(n / ms / 1e3, 1), "hit_fraction": round(frac, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

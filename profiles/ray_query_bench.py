"""Ray-query throughput on the bunny-class scene (include/shader_ray_query.h), one JSON line on stdout.

  (a) the headline frame's 1920x1080 primary rays (bench.py's first orbit view) as an explicit ray buffer, closest hit;
      beside it, shray_render_device of the same frame (1 spp, the same rays plus the bounces and the shading)
  (b) 2^21 incoherent rays: seeded points on the surface, cosine-distributed directions about the surface normal,
      tmax = a tenth of the scene's extent (ambient-occlusion-like), closest hit
  (c) (b) as any-hit

Every time is the median of --trials launches after --warmup launches, bracketed by HIP events on the current torch stream.
Usage: python profiles/ray_query_bench.py [--kernel 0|1] [--trials 15] [--warmup 5]"""
import numpy as np

import bench_harness as H
from bench_workloads import ao_rays, camera_rays

F = np.float32


def main():
    ap = H.parser()
    ap.add_argument("--kernel", type=int, default=0)
    args = ap.parse_args()

    pkg = H.load_package()
    with H.bunny_scene(pkg, pkg.scenes.environment_hdr_sky(2048)) as (world, scene, positions):
        run(pkg, args, world, scene, positions)


def run(pkg, args, world, scene, positions):
    import torch
    import bench
    import ray_query_ref as R
    W, HEIGHT = 1920, 1080
    params = bench.orbit_params(pkg, world, W, HEIGHT)[0]
    scene.set_kernel(args.kernel)
    stream = torch.cuda.current_stream()
    median_ms = H.median_timer(args)

    def device_rays(o, d, tmax):
        return H.upload(pkg.tracer.make_rays(o, d, tmax), 8)

    def query(d_rays, any_hit=False):
        d_hits = torch.empty((d_rays.shape[0], 4), dtype=torch.int32, device="cuda")
        fn = lambda: scene.trace_rays_into(d_rays.data_ptr(), d_rays.shape[0], d_hits.data_ptr(), stream.cuda_stream, any_hit=any_hit)
        ms = median_ms(fn)
        torch.cuda.synchronize()
        hit_fraction = float((d_hits[:, 3] >= 0).float().mean().item())
        return ms, hit_fraction

    out = {"scene": "bunny-class trisrc (69,168 triangles)", "kernel": args.kernel, "trials": args.trials, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    o, d = camera_rays(params, W, HEIGHT, R.xform)
    ra = device_rays(o, d, F(1e7))
    (ms, lo, hi, _), frac = query(ra)
    frame = torch.empty((HEIGHT, W, 4), dtype=torch.float32, device="cuda")
    rms, rlo, rhi, _ = median_ms(lambda: scene.render_into(params, W, HEIGHT, 1, frame.data_ptr(), stream.cuda_stream, None))
    out["a_primary_closest"] = {"rays": W * HEIGHT, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                                "Mrays_s": round(W * HEIGHT / ms / 1e3, 1), "hit_fraction": round(frac, 4),
                                "render_ms": round(rms, 4), "render_ms_min_max": [round(rlo, 4), round(rhi, 4)]}
    n = 1 << 21
    o, d, tmax = ao_rays(positions, n, seed=2024)
    rb = device_rays(o, d, tmax)
    for key, any_hit in (("b_ao_closest", False), ("c_ao_any", True)):
        (ms, lo, hi, _), frac = query(rb, any_hit)
        out[key] = {"rays": n, "tmax": float(tmax), "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                    "Mrays_s": round(n / ms / 1e3, 1), "hit_fraction": round(frac, 4)}
    H.emit(out, args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The timed loop's launches with a camera that does not stand still (EXPERIMENTS R9.1; run it in the parent's checkout and here).

    python profiles/view_cache_camera.py [--steps 200] [--runs 3]

bench.py's loop -- the bunny-class mesh at 1920x1080, 1 spp, gold, the orbit's object rotations, four frames per launch over four
streams -- with the camera's distance set per launch: `fixed` (bench.py's own loop), `moving` (another distance in every launch:
nothing is ever cached, and the loop must time like the parent's) and `alternating` (two distances in turn: both views stay
cached).  One line per mode and run: ms per frame, and the view cache's statistics where the library has them."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch                                  # noqa: E402
import bench                                  # noqa: E402
from __graft_entry__ import load_package      # noqa: E402


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 200
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 3
    pkg = load_package()
    world = pkg.World(pkg.scenes.bunny_trisrc())
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048), device=0)
    W, H, batch, lanes = bench.WIDTH, bench.HEIGHT, 4, 4
    orbit = bench.orbit_params(pkg, world, W, H)
    zoom = orbit[0].camera_matrix[14]
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(lanes - 1)]
    outs = [torch.empty(batch * H * W * 4, dtype=torch.float32, device="cuda") for _ in range(lanes)]

    def distance(mode, launch):
        if mode == "moving":
            return zoom * (1.0 + 0.0005 * (launch % 64))
        if mode == "alternating":
            return zoom * (1.0 + 0.01 * (launch % 2))
        return zoom

    def loop(mode, frames, first_launch):
        for j in range(frames // batch):
            views = []
            for k in range(batch):
                p = orbit[(j * batch + k) % bench.ORBIT].copy()
                p.camera_matrix[14] = distance(mode, first_launch + j)
                views.append(p)
            scene.render_batch_into(views, W, H, 1, outs[j % lanes].data_ptr(), H * W * 16, streams[j % lanes].cuda_stream, None)
        return frames // batch

    for mode in ("fixed", "moving", "alternating"):
        launch = loop(mode, 80, 0)          # warm-up and clock ramp
        torch.cuda.synchronize()
        for _ in range(runs):
            before = scene.view_cache_stats() if hasattr(scene, "view_cache_stats") else None
            t0 = time.perf_counter()
            launch += loop(mode, steps, launch)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            row = {"mode": mode, "ms_per_frame": round(dt / steps * 1e3, 5), "mrays_per_s": round(W * H * steps / dt / 1e6, 1)}
            if before is not None:
                after = scene.view_cache_stats()
                row.update({"launches": steps // batch, "launches_cached": after["launches_cached"] - before["launches_cached"],
                            "entries_built": after["entries_built"] - before["entries_built"], "bytes_held": after["bytes_held"]})
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

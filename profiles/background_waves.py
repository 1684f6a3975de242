#!/usr/bin/env python3
"""Share of the headline frame's 8x8 wave tiles whose primary rays all leave the scene, over the orbit's views (EXPERIMENTS R9.1).

    python profiles/background_waves.py [out.json]

The timed kernels render a frame in 8x8 pixel tiles, one wave each; a tile without a primary hit is a wave that the view cache
serves from its background table.  Primary hits come from the ray-query library (shray_primary_hits_device); the frames are
bench.py's: bunny-class mesh, 1920x1080, the trackball orbit of 20 views."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                  # noqa: E402  (the orbit's definition)
from __graft_entry__ import load_package      # noqa: E402


def main():
    pkg = load_package()
    world = pkg.World(pkg.scenes.bunny_trisrc())
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(256), device=0)
    W, H = bench.WIDTH, bench.HEIGHT
    rows = []
    for k, params in enumerate(bench.orbit_params(pkg, world, W, H)):
        triangle = scene.primary_hits(params, W, H)["triangle"]
        hit = (triangle >= 0) | (triangle == pkg._native.HIT_CAP)         # (a capped ray keeps its wave on the full path too)
        th, tw = -(-H // 8), -(-W // 8)
        padded = np.zeros((th * 8, tw * 8), bool)
        padded[:H, :W] = hit
        per_tile = padded.reshape(th, 8, tw, 8).sum(axis=(1, 3))
        rows.append({"view": k, "pixels_hit": float(hit.mean()), "tiles": int(th * tw), "tiles_without_hit": int((per_tile == 0).sum()),
                     "tiles_mixed": int(((per_tile > 0) & (per_tile < 64)).sum())})
        print(rows[-1], flush=True)
    share = float(np.mean([r["tiles_without_hit"] / r["tiles"] for r in rows]))
    out = {"width": W, "height": H, "views": rows, "mean_share_of_tiles_without_hit": share}
    print(json.dumps({"mean_share_of_tiles_without_hit": share}))
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()

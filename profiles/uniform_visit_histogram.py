#!/usr/bin/env python3
"""Wave-uniform node visits by outcome (diagnostic build with -DSHRAY_DIAG_UNIFORM):
    make -C shader-ray_amd variant VARIANT=uniform HIP_EXTRA="-DSHRAY_DIAGNOSTICS -DSHRAY_DIAG_UNIFORM"
    SHRAY_DIAG_LIB=shader-ray_amd/_variants/libshray_hip_uniform.so python profiles/uniform_visit_histogram.py [--million] [--material 6]
Of the node stage's wave-visits whose walking lanes are all at one record -- the ones a packet-level (scalar interval) test could
decide for the whole wave -- how many end with every lane entering, with no lane entering, or mixed.

--origin (round 8, R8.1; a library built with -DSHRAY_DIAG_UNIFORM_ORIGIN as well, e.g. VARIANT=uniform_origin): where the
"no lane enters" uniform visits come from -- directly after a uniform every-lane-enters-a-branch turn of the same stage call (the
popped word is the one the wave has just pushed: a one-deep scalar mirror serves it), at one remove or more, or elsewhere -- and
how many uniform every-lane-enters turns are at a leaf's record.  That build's tallies 5-7 hold these instead of the
distinct-record classes and the walking lanes (variants/diag_uniform_visit.inc)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--material", type=int, default=0)
    ap.add_argument("--million", action="store_true")
    ap.add_argument("--origin", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    pkg = load_package()
    N = pkg._native
    N.HIP_LIB = os.environ["SHRAY_DIAG_LIB"]
    lib = N.load_hip()
    lib.shray_debug_timeline.restype = C.c_int
    world = pkg.World(pkg.scenes.million_obj() if args.million else pkg.scenes.bunny_trisrc())
    scene = pkg.Scene(world.flatten(), pkg.scenes.environment_hdr_sky(2048), device=0)
    W, H = args.width, args.height
    params = world.frame_params(W, H, material=args.material)
    patches = ((W + 15) // 16) * ((H + 15) // 16)
    stamps = np.zeros((patches * 4, 16), dtype=np.uint64)
    N.check(lib.shray_debug_timeline(scene._handle, C.byref(params), W, H, 1, stamps.ctypes.data_as(C.c_void_p)))
    t = stamps[:, 4:12].astype(np.float64).sum(axis=0)
    visits, uniform, all_enter, all_miss, mixed, two, three_four, lanes = t
    if args.origin:
        return origin(args, stamps, visits, uniform, all_enter, all_miss, mixed)
    print(f"scene: {'1M triangles' if args.million else 'bunny-class'}, material {args.material}, {W}x{H}, one frame (the start-up view)")
    print(f"wave-visits of the node stage          {visits:14.0f}   ({lanes / visits:.1f} walking lanes on average)")
    print(f"  distinct records among the walking lanes: 1: {uniform / visits:.3f}   2: {two / visits:.3f}   3-4: {three_four / visits:.3f}   "
          f"more: {(visits - uniform - two - three_four) / visits:.3f}")
    print(f"  wave-uniform (one record)            {uniform:14.0f}   {uniform / visits:6.3f} of all")
    print(f"    every lane enters                  {all_enter:14.0f}   {all_enter / max(uniform, 1):6.3f} of the uniform ones")
    print(f"    no lane enters                     {all_miss:14.0f}   {all_miss / max(uniform, 1):6.3f}")
    print(f"    mixed                              {mixed:14.0f}   {mixed / max(uniform, 1):6.3f}")
    print(f"  a packet-level decision could settle {all_enter + all_miss:14.0f}   {(all_enter + all_miss) / max(uniform, 1):6.3f} of the uniform visits = "
          f"{(all_enter + all_miss) / visits:6.3f} of all wave-visits")


def origin(args, stamps, visits, uniform, all_enter, all_miss, mixed):
    direct = float((stamps[:, 9] & np.uint64(0xffffffff)).astype(np.float64).sum())
    across = float((stamps[:, 9] >> np.uint64(32)).astype(np.float64).sum())
    removed = float(stamps[:, 10].astype(np.float64).sum())
    at_leaf = float(stamps[:, 11].astype(np.float64).sum())
    print(f"scene: {'1M triangles' if args.million else 'bunny-class'}, material {args.material}, {args.width}x{args.height}, "
          f"one frame (the start-up view)")
    print(f"wave-visits of the node stage          {visits:14.0f}")
    print(f"  wave-uniform (one record)            {uniform:14.0f}   {uniform / visits:6.3f} of all")
    print(f"    every lane enters                  {all_enter:14.0f}   {all_enter / max(uniform, 1):6.3f} of the uniform ones")
    print(f"      ... a leaf's record              {at_leaf:14.0f}   {at_leaf / max(all_enter, 1):6.3f} of those")
    print(f"    mixed                              {mixed:14.0f}   {mixed / max(uniform, 1):6.3f} of the uniform ones")
    print(f"    no lane enters                     {all_miss:14.0f}   {all_miss / max(uniform, 1):6.3f} of the uniform ones")
    print(f"      directly after a run's push      {direct + across:14.0f}   {(direct + across) / max(all_miss, 1):6.3f} of those")
    print(f"        within one group of four turns {direct:14.0f}   {direct / max(all_miss, 1):6.3f}   (the one-deep mirror)")
    print(f"        across the exit tests          {across:14.0f}   {across / max(all_miss, 1):6.3f}")
    print(f"      at one remove or more            {removed:14.0f}   {removed / max(all_miss, 1):6.3f}   (a deeper mirror)")
    print(f"      elsewhere (through LDS)          {all_miss - direct - across - removed:14.0f}   "
          f"{(all_miss - direct - across - removed) / max(all_miss, 1):6.3f}")
    print(f"  mirrored pops per wave-visit: {direct / visits:.4f}; no-lane-enters uniform turns per wave-visit: {all_miss / visits:.4f}; "
          f"every-lane-enters-a-leaf turns per wave-visit: {at_leaf / visits:.4f}")


if __name__ == "__main__":
    main()

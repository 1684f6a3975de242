"""The scaffold of the profiles/*_bench.py scripts, once: the timer, the median with its warm-up and slow-launch fallback, the
alternating A/B measurement, the entry formatter, the common options, the two benchmark scenes, the upload and the final line.

Importing this module puts the repository root, tests/ and profiles/ on sys.path and imports neither torch nor the package,
so a script's --help needs no GPU.  The clock is an argument (a function that runs fn and returns milliseconds): the scripts
pass `event_clock()`, the tests a scripted one.  DESIGN §34 has the per-script slow_ms table and the A/B protocol that
profiles/ab_band.py judges."""
import argparse
import contextlib
import functools
import json
import os
import statistics
import sys
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

F = np.float32


class Timing(NamedTuple):
    ms: float       # the median
    lo: float
    hi: float
    trials: int     # the trials actually run: 3 where the slow-launch fallback applied


def event_clock(stream=None):
    """the clock of every script: fn bracketed by two HIP events on `stream` (default: the current torch stream)"""
    import torch
    stream = torch.cuda.current_stream() if stream is None else stream

    def clock(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)
    return clock


def timed(fn, before=None, *, clock):
    """milliseconds of one launch of fn; `before`, when given, runs first and outside the bracket"""
    if before:
        before()
    return clock(fn)


def median_ms(fn, *, before=None, trials, warmup, slow_ms=None, clock):
    """Timing of `trials` launches after `warmup` untimed ones (each after `before`, when given).  With slow_ms, one probe
    launch comes first, and a probe over slow_ms milliseconds makes it 3 trials and no warm-up."""
    if slow_ms is not None and timed(fn, before, clock=clock) > slow_ms:
        trials, warmup = 3, 0
    for _ in range(warmup):
        if before:
            before()
        fn()
    times = [timed(fn, before, clock=clock) for _ in range(trials)]
    return Timing(float(statistics.median(times)), float(min(times)), float(max(times)), trials)


def alternating(fn_a, fn_b, *, trials, clock):
    """fn_a and fn_b in turn: three untimed rounds of both, then `trials` timed pairs, a before b.  Per side the median and
    the fastest launch, and the spread of the yardstick fn_a itself: the medians of its first and second half of the pairs."""
    for fn in (fn_a, fn_b) * 3:
        fn()
    pairs = [(clock(fn_a), clock(fn_b)) for _ in range(trials)]
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    half = trials // 2
    median = lambda xs: float(statistics.median(xs)) if xs else float("nan")   # noqa: E731  (one trial: the first half is empty)
    return {"ms": [median(a), median(b)], "ms_min": [float(min(a)), float(min(b))],
            "a_first_second_half": [median(a[:half]), median(a[half:])]}


def median_timer(args, slow_ms=None, clock=None):
    """median_ms bound to a script's --trials and --warmup, its slow-launch threshold, and the event clock unless one is given.
    A call may override trials, warmup and before; slow_ms stays bound, so an overridden call still makes its probe launch
    and still falls back to 3 trials over the threshold (near_bench's torch brute force, at trials=3, relies on that)."""
    clock = event_clock() if clock is None else clock
    return functools.partial(median_ms, trials=args.trials, warmup=args.warmup, slow_ms=slow_ms, clock=clock)


def entry(t, rate_key=None, count=None, *, places=4, divisor=1e3, trials=True, **first):
    """a result cell of a Timing: the keys of `first`, ms and ms_min_max to 4 places, trials (unless trials=False), and under
    `rate_key` the throughput count / ms / divisor to `places` places"""
    out = dict(first, ms=round(t.ms, 4), ms_min_max=[round(t.lo, 4), round(t.hi, 4)])
    if trials:
        out["trials"] = t.trials
    if rate_key:
        out[rate_key] = round(count / t.ms / divisor, places)
    return out


def parser(trials=15, warmup=5, out=None):
    """the options every script has; a script adds its own to the parser returned"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=trials)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--out", default=out, metavar="FILE", help="also write the JSON line here")
    return ap


def emit(out, args):
    """the script's one JSON line: on stdout, and in --out when given"""
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


def load_package():
    from __graft_entry__ import load_package as load
    return load()


@contextlib.contextmanager
def scene_of(pkg, path, *scene_args):
    """(world, scene, positions) of the scene file at `path`, both closed on the way out; scene_args go to Scene after the
    flattened world (an environment, say)"""
    world = pkg.World(path)
    scene = pkg.Scene(world.flatten(), *scene_args)
    try:
        yield world, scene, np.asarray(world.arrays()["vertex_positions"], F)
    finally:
        scene.close()
        world.close()


def bunny_scene(pkg, *scene_args):
    return scene_of(pkg, pkg.scenes.bunny_trisrc(), *scene_args)


def million_scene(pkg, *scene_args):
    return scene_of(pkg, pkg.scenes.million_obj(), *scene_args)


def lobed_scene(pkg, *scene_args):
    """the 528-triangle member of the many-instance rows"""
    return scene_of(pkg, os.path.join(ROOT, "tests", "golden", "lobed_528.trisrc"), *scene_args)


def upload(records, width):
    """a host array of packed records (make_points, make_rays, make_boxes, make_triangles) as a [n, width] float32 GPU tensor"""
    import torch
    return torch.from_numpy(records.view(F).reshape(-1, width).copy()).cuda()

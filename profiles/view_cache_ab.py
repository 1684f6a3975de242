#!/usr/bin/env python3
"""Interleaved A/B of bench.py's two forms between builds of libshray_hip.so (EXPERIMENTS R9.1: the view cache).

    python profiles/view_cache_ab.py --parent DIR [--variant NAME=PATH ...] [--runs 3] [--out FILE]

Builds compared, in this order within every round: `parent` (DIR: a built checkout of the parent commit, whose own bench.py is
run -- its Python layer binds the entry points its library has), `cached` (this tree's library), `off` (this tree's library with SHRAY_VIEW_CACHE=0: must time like the parent) and every --variant (another
build of this tree, e.g. `make variant`).  Forms: --steps 200, and --steps 20 --warmup 5.  One bench.py child process per
run, one at a time; a child that does not end with code 0 ends the comparison.  Prints one line per run and, at the end, every
build's range per form and whether its slowest run beats the parent's fastest (the rule of R7.1 / R8.1)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [["--steps", "200"], ["--steps", "20", "--warmup", "5"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per bench.py run")
    args = ap.parse_args()
    builds = [("parent", {}), ("cached", {}), ("off", {"SHRAY_VIEW_CACHE": "0"})]
    builds += [(v.split("=", 1)[0], {"SHRAY_HIP_LIB": os.path.abspath(v.split("=", 1)[1])}) for v in args.variant]
    sink = open(args.out, "a") if args.out else None

    def say(text):
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    values = {}
    for form in FORMS:
        for _ in range(args.runs):
            for name, extra in builds:
                env = {k: v for k, v in os.environ.items() if k not in ("SHRAY_HIP_LIB", "SHRAY_VIEW_CACHE")}
                env.update(extra)
                tree = os.path.abspath(args.parent) if name == "parent" else ROOT
                run = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", *form], env=env, cwd=tree,
                                     capture_output=True, text=True, timeout=args.timeout)
                if run.returncode != 0:
                    say(f"{name:<12} {' '.join(form):<28} left with code {run.returncode}: {run.stderr[-300:]}")
                    return run.returncode
                line = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
                values.setdefault((name, " ".join(form)), []).append(line["value"])
                say(f"{name:<12} {' '.join(form):<28} {line['ms_per_step']} ms/frame {line['value']} Mrays/s")
    say("\nRule: the slowest run of a build against the fastest run of the parent, per form")
    for form in FORMS:
        f = " ".join(form)
        best_parent = max(values[("parent", f)])
        for name, _ in builds:
            v = sorted(values[(name, f)])
            verdict = "" if name == "parent" else f"   slowest / parent's fastest = {v[0] / best_parent:.4f}" + ("  SEPARATES" if v[0] > best_parent else "")
            say(f"{f:<28} {name:<12} {v[0]:>10.1f} .. {v[-1]:>10.1f}  median {v[len(v) // 2]:>10.1f}{verdict}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

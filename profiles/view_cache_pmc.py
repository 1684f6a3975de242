#!/usr/bin/env python3
"""Hardware counters of the timed loop's four-frame launches, one tree (EXPERIMENTS R9.1; run it in the parent's checkout and here).

    python profiles/view_cache_pmc.py [--steps 80] [--skip 4] [out.txt]

Runs bench.py's --counter-child form (scene load, --steps frames of the timed loop's launches, exit) under `rocprofv3 --pmc`, one
counter group per pass and nothing traced beside it, the program behind `--` as a child; prints every counter's mean per launch
of the stack tracer's batch kernel, the first --skip launches left out (the launches before a view-cache entry exists), and the
other kernels' totals (the cache's prepass)."""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ["SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_SMEM SQ_WAVE_CYCLES", "FETCH_SIZE", "WRITE_SIZE"]


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 80
    skip = int(args[args.index("--skip") + 1]) if "--skip" in args else 4
    out_path = next((a for a in args if a.endswith(".txt")), None)
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    lines = []
    for group in GROUPS:
        out = tempfile.mkdtemp(prefix="shray_pmc_", dir="/tmp")
        cmd = [tool, "--pmc", *group.split(), "--output-format", "csv", "-d", out, "--", sys.executable, os.path.join(ROOT, "bench.py"),
               "--counter-child", "--steps", str(steps), "--warmup", "0"]
        run = subprocess.run(cmd, cwd="/tmp", stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=240)
        if run.returncode != 0:
            print(f"pass {group}: code {run.returncode}: {run.stderr[-300:]}")
            return run.returncode
        per = {}      # (kernel, counter) -> {dispatch id: value}
        for path in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                key = (r["Kernel_Name"].split("(")[0], r["Counter_Name"])
                d = per.setdefault(key, {})
                d[int(r["Dispatch_Id"])] = d.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
        shutil.rmtree(out, ignore_errors=True)
        for (kernel, counter), by_dispatch in sorted(per.items()):
            values = [v for _, v in sorted(by_dispatch.items())]
            if "trace_stack_batch" in kernel:
                kept = values[skip:]
                lines.append(f"{kernel:<60} {counter:<18} launches {len(kept):>3} (after {skip} skipped)  mean per launch {sum(kept) / len(kept):>16.1f}")
            elif "view_cache" in kernel:
                lines.append(f"{kernel:<60} {counter:<18} launches {len(values):>3}  total {sum(values):>16.1f}")
    text = "\n".join(lines)
    print(text)
    if out_path:
        open(out_path, "a").write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

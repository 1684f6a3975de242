"""profiles/bench_harness.py on the GPU: the event clock around a trivial launch, and one real script end to end at its
smallest size, in a child process."""
import json
import math
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench_harness as H  # noqa: E402

pytestmark = pytest.mark.gpu


def test_event_clock_times_a_trivial_launch(gpu):
    import torch
    x = torch.ones(1 << 20, device="cuda")
    y = torch.empty_like(x)
    add = lambda: torch.add(x, 1.0, out=y)   # noqa: E731
    clock = H.event_clock(torch.cuda.current_stream())
    t = H.median_ms(add, trials=3, warmup=1, clock=clock)
    assert t.trials == 3 and all(math.isfinite(v) and v > 0 for v in t[:3]) and t.lo <= t.ms <= t.hi
    assert H.median_timer(types.SimpleNamespace(trials=3, warmup=1), slow_ms=500.0)(add).trials == 3      # the default clock
    r = H.alternating(add, lambda: torch.mul(x, 2.0, out=y), trials=4, clock=clock)
    for key in ("ms", "ms_min", "a_first_second_half"):
        assert len(r[key]) == 2 and all(math.isfinite(v) and v > 0 for v in r[key])
    assert r["ms_min"][0] <= r["ms"][0] and r["ms_min"][1] <= r["ms"][1]
    assert float(y[0]) == 2.0


def test_one_script_end_to_end_at_its_smallest_size(gpu, tmp_path):
    """16384 boxes are one slab of the 128^2 grid, the fewest for which the script's grid cells number what was asked for"""
    out = tmp_path / "line.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "instance_overlap_bench.py"), "--boxes", "16384", "--trials", "1",
                        "--warmup", "0", "--out", str(out)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0] + "\n" == out.read_text()
    line = json.loads(lines[0])
    assert line["boxes"] == 16384 and line["trials"] == 1 and line["warmup"] == 0
    assert line["a_identity"]["grid128"]["counts_only"]["instance"]["ms"] > 0
    assert line["b_bunny_8x8"]["surface_5pct"]["any"]["ms"] > 0

    def answers(node):
        if isinstance(node, dict):
            for key, value in node.items():
                if key == "same_answer":
                    yield value
                else:
                    yield from answers(value)

    found = list(answers(line))
    assert len(found) == 6 and all(v is True for v in found)

"""profiles/bench_harness.py, bench_workloads.py and ab_band.py on the CPU: the timing logic on a scripted clock, the entry
formatter against recorded entries, the band rule against the recorded A/B file, every script's --help, and the workload
generators against values recorded from the commit before they moved.

tests/golden/bench_workloads.npz was written once from that commit's functions (instance_bench.grid_transforms and down_rays,
point_query_bench.morton_order and near_points, instance_point_bench.near_surface_points, ray_query_bench.camera_rays and
ao_rays, multihit_bench.through_rays) on the inputs stored beside the outputs: `positions`, 20 random triangles; `points`,
64 normal points; `mats`, four random 4x4 matrices for a 16x9 camera; the seeds are the ones in the test below."""
import glob
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles")
sys.path.insert(0, PROFILES)
import ab_band  # noqa: E402
import bench_harness as H  # noqa: E402
import bench_workloads as W  # noqa: E402

AB_FILE = os.path.join(PROFILES, "packed_walk_ab.jsonl")
SCRIPTS = sorted(glob.glob(os.path.join(PROFILES, "*_bench.py")))


class Script:
    """a clock that replays a list of times, and the log of everything that ran, in order"""

    def __init__(self, times):
        self.times, self.log = list(times), []

    def clock(self, fn):
        self.log.append("[")
        fn()
        self.log.append("]")
        return self.times.pop(0)

    def fn(self, name="fn"):
        return lambda: self.log.append(name)


def test_median_ms_counts_its_calls_and_takes_the_median():
    s = Script([5.0, 1.0, 3.0, 9.0])
    t = H.median_ms(s.fn(), trials=4, warmup=2, clock=s.clock)
    assert t == H.Timing(4.0, 1.0, 9.0, 4) and (t.ms, t.lo, t.hi, t.trials) == (4.0, 1.0, 9.0, 4)
    assert s.log.count("fn") == 2 + 4 and s.log[:2] == ["fn", "fn"] and s.log.count("[") == 4       # warm-up is not timed
    s = Script([2.0, 7.0, 4.0])
    assert H.median_ms(s.fn(), trials=3, warmup=0, clock=s.clock).ms == 4.0


def test_slow_probe_is_one_extra_call_and_strictly_over_the_threshold():
    s = Script([10.0, 1.0, 2.0, 3.0])
    t = H.median_ms(s.fn(), trials=3, warmup=2, slow_ms=500.0, clock=s.clock)
    assert t.trials == 3 and t.ms == 2.0 and s.log.count("fn") == 1 + 2 + 3
    s = Script([500.0] + [1.0] * 5)                                     # equal to the threshold: not slow
    t = H.median_ms(s.fn(), trials=5, warmup=2, slow_ms=500.0, clock=s.clock)
    assert t.trials == 5 and s.log.count("fn") == 1 + 2 + 5
    s = Script([500.5, 4.0, 6.0, 5.0])                                  # over it: 3 trials, no warm-up
    t = H.median_ms(s.fn(), trials=15, warmup=5, slow_ms=500.0, clock=s.clock)
    assert t == H.Timing(5.0, 4.0, 6.0, 3) and s.log.count("fn") == 1 + 3 and s.log.count("[") == 4


def test_before_runs_once_per_launch_and_outside_the_bracket():
    s = Script([1.0, 2.0, 3.0])
    H.median_ms(s.fn(), before=s.fn("before"), trials=2, warmup=2, slow_ms=10.0, clock=s.clock)
    timed, warm = ["before", "[", "fn", "]"], ["before", "fn"]
    assert s.log == timed + warm * 2 + timed * 2
    s = Script([1.0])
    assert H.timed(s.fn(), s.fn("before"), clock=s.clock) == 1.0 and s.log == timed


def test_median_timer_binds_the_options_and_a_call_overrides_them():
    s = Script([1.0] * 4 + [2.0] * 3)
    median_ms = H.median_timer(types.SimpleNamespace(trials=4, warmup=1), clock=s.clock)
    assert median_ms(s.fn()).trials == 4 and s.log.count("fn") == 5
    assert median_ms(s.fn(), trials=3, warmup=0) == H.Timing(2.0, 2.0, 2.0, 3)


def test_alternating_order_medians_and_halves():
    #            a     b
    s = Script([1.0, 10.0, 2.0, 20.0, 9.0, 30.0, 4.0, 40.0, 5.0, 50.0])
    r = H.alternating(s.fn("a"), s.fn("b"), trials=5, clock=s.clock)
    assert s.log == ["a", "b"] * 3 + ["[", "a", "]", "[", "b", "]"] * 5
    assert r["ms"] == [4.0, 30.0] and r["ms_min"] == [1.0, 10.0]
    assert r["a_first_second_half"] == [1.5, 5.0]                       # a's first 5 // 2 = 2 pairs, then the other 3
    s = Script([3.0, 4.0])                                              # one trial: an empty first half is NaN, not an error
    r = H.alternating(s.fn("a"), s.fn("b"), trials=1, clock=s.clock)
    assert r["ms"] == [3.0, 4.0] and math.isnan(r["a_first_second_half"][0]) and r["a_first_second_half"][1] == 3.0


def recorded(path, *keys, where=None):
    with open(path) as f:
        node = next(r for r in map(json.loads, f) if where is None or all(r[k] == v for k, v in where.items()))
    for key in keys:
        node = node[key]
    return node


def rebuilt(e):
    return H.Timing(e["ms"], e["ms_min_max"][0], e["ms_min_max"][1], e["trials"])


def test_entry_reproduces_recorded_entries_digit_for_digit():
    """(the recorded throughputs were taken from the unrounded median; these three are entries where the rounded one gives the
    same four places)"""
    e = recorded(os.path.join(PROFILES, "overlap_bench.json"), "bunny", "surface_5pct", "K8_counts")
    assert e == {"boxes": 1048576, "ms": 19.6388, "ms_min_max": [19.2984, 20.1465], "trials": 15, "Mboxes_s": 53.3931}
    assert H.entry(rebuilt(e), "Mboxes_s", e["boxes"], boxes=e["boxes"]) == e
    assert json.dumps(H.entry(rebuilt(e), "Mboxes_s", e["boxes"], boxes=e["boxes"])) == json.dumps(e)         # and the key order
    e = recorded(os.path.join(PROFILES, "instance_near_bench.json"), "a_identity", "radius_0.02", "K64_counts", "instance")
    assert e == {"ms": 48.6193, "ms_min_max": [48.1064, 49.338], "trials": 15, "Mpoints_s": 5.3918}
    assert json.dumps(H.entry(rebuilt(e), "Mpoints_s", 262144)) == json.dumps(e)
    e = recorded(AB_FILE, "bunny", "r1pct", "K64_pruned", where={"script": "near_bench", "build": "parent", "round": 1})
    assert e == {"points": 1048576, "ms": 69.0402, "ms_min_max": [67.7994, 69.6942], "trials": 7, "Mpoints_s": 15.1879}
    assert json.dumps(H.entry(rebuilt(e), "Mpoints_s", e["points"], points=e["points"])) == json.dumps(e)
    t = H.Timing(1.23456, 1.0, 2.0, 7)                                                                    # the other shapes
    assert H.entry(t, "Mrays_s", 1 << 20, places=1, trials=False) == {"ms": 1.2346, "ms_min_max": [1.0, 2.0], "Mrays_s": 849.4}
    assert H.entry(t) == {"ms": 1.2346, "ms_min_max": [1.0, 2.0], "trials": 7}
    # the rate comes from the unrounded median, as in every script: 2^20 / 0.88144 / 1e3, not 2^20 / 0.8814 / 1e3 = 1189.671
    assert H.entry(H.Timing(0.88144, 0.8, 0.9, 7), "Mpoints_s", 1 << 20) == {"ms": 0.8814, "ms_min_max": [0.8, 0.9], "trials": 7,
                                                                              "Mpoints_s": 1189.617}


def counts(table, gating):
    return tuple(sum(1 for e in table if e["gating"] == gating and e["verdict"] == v) for v in ab_band.VERDICTS)


def test_ab_band_on_the_recorded_file():
    with open(AB_FILE) as f:
        rows, rounds = ab_band.read_rows(f)
    table = ab_band.judge(rows, rounds)
    assert len(table) == 214 and counts(table, True) == (145, 10, 59, 0)
    table = ab_band.judge(rows, rounds, ["*torch*"])
    assert counts(table, True) == (135, 10, 57, 0) and counts(table, False) == (10, 0, 2, 0)
    by_name = {(e["script"], e["row"]): e for e in table}
    e = by_name["near_bench", "bunny.r1pct.K1_pruned.ms"]
    assert e["verdict"] == "above" and f"{e['median']:.4g}" == "1.28" and [float(f"{x:.4g}") for x in e["band"]] == [0.8336, 0.977]
    assert by_name["near_bench", "bunny.r5pct.K64_pruned.ms"]["verdict"] == "below"
    assert by_name["near_bench", "bunny.r1pct.K4_counts.ms"]["verdict"] == "inside"
    assert "| near | `bunny.r1pct.K1_pruned.ms` | 0.8814, 0.9292, 0.8985 | 1.28, 1.334, 1.268 | 0.8336 – 0.977 | 1.28, above |" in \
        ab_band.markdown(table).split("\n")
    assert not ab_band.summary(table)["passes"]


def test_ab_band_on_this_harness_own_recorded_run():
    """profiles/bench_harness_ab.jsonl: four scripts from the parent and through the harness, three rounds"""
    with open(os.path.join(PROFILES, "bench_harness_ab.jsonl")) as f:
        table = ab_band.judge(*ab_band.read_rows(f), ["*torch*"])
    assert {e["script"] for e in table} == {"near_bench", "instance_overlap_bench", "sdf_bench", "instance_point_bench"}
    assert counts(table, True) == (62, 1, 0, 0) and counts(table, False) == (3, 0, 0, 0) and ab_band.summary(table)["passes"]


def test_ab_band_incomplete_rows_and_exit_status(tmp_path, capsys):
    with open(AB_FILE) as f:
        lines = [line for line in f if json.loads(line)["script"] == "overlap_bench"]
    whole = tmp_path / "whole.jsonl"
    whole.write_text("".join(lines))
    assert ab_band.main([str(whole)]) == 0                              # every row of this script was inside
    result = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert result["passes"] and result["gating"]["above"] == 0 and result["rows"] == sum(result["gating"].values())
    dropped = [line for line in lines if not (json.loads(line)["script"], json.loads(line)["build"], json.loads(line)["round"]) ==
               ("overlap_bench", "this", 2)]
    part = tmp_path / "part.jsonl"
    part.write_text("".join(dropped))
    assert ab_band.main([str(part)]) == 1
    after = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with open(part) as f:
        table = ab_band.judge(*ab_band.read_rows(f))
    assert {e["verdict"] for e in table if e["script"] == "overlap_bench"} == {"incomplete"}
    assert after["gating"]["incomplete"] == sum(1 for e in table if e["script"] == "overlap_bench") > 0 and not after["passes"]
    assert ab_band.main([str(part), "--report-only", "overlap_bench:*"]) == 0           # reported, not gating


def test_ab_band_append_round_trips_a_line(tmp_path):
    target = tmp_path / "ab.jsonl"
    line = {"trials": 3, "bunny": {"a": {"ms": 1.5, "n_mean": 2.0}, "wall_ms": 7}, "same_answer": True}
    for build, ms in (("parent", 1.5), ("this", 1.6)):
        line["bunny"]["a"]["ms"] = ms
        p = subprocess.run([sys.executable, os.path.join(PROFILES, "ab_band.py"), "append", str(target), "--script", "x_bench", "--build", build,
                            "--round", "1"], input=json.dumps(line) + "\n", text=True, capture_output=True)
        assert p.returncode == 0, p.stderr
    records = [json.loads(x) for x in target.read_text().splitlines()]
    assert records[1] == {"script": "x_bench", "build": "this", "round": 1, **line}
    with open(target) as f:
        rows, _ = ab_band.read_rows(f)
    assert rows == {("x_bench", "bunny.a.ms"): {"parent": {1: 1.5}, "this": {1: 1.6}},
                    ("x_bench", "bunny.wall_ms"): {"parent": {1: 7.0}, "this": {1: 7.0}}}


OPTIONS = {"clearance": [], "instance": ["--skip-merged"], "instance_clearance": ["--queries"], "instance_intersect": ["--queries"],
           "instance_multihit": ["--compose-rays"], "instance_near": ["--points"], "instance_overlap": ["--boxes"], "instance_pairs": [],
           "instance_point": ["--points"], "instance_sdf": ["--points"], "instance_update": ["--sizes", "--trace-only"],
           "instance_winding": ["--points"], "intersect": ["--no-million"], "multihit": ["--no-million"],
           "near": ["--no-million", "--max-tests", "--ab"], "overlap": ["--no-million"], "point_query": ["--no-million"],
           "ray_query": ["--kernel"], "refit": [], "sdf": ["--no-million"], "winding": ["--no-million"]}
DEFAULTS = {"instance_update": ("10", "3")}
HELP_CHILD = """
import os, runpy, sys
sys.path.insert(0, os.path.dirname(sys.argv[1]))      # as `python profiles/x_bench.py` would
sys.argv = [sys.argv[1], "--help"]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    assert e.code == 0, e.code
    assert "torch" not in sys.modules, "--help imported torch"
    sys.exit(0)
sys.exit("--help did not exit")
"""


def test_there_are_21_scripts_and_none_defines_the_scaffold_or_imports_another():
    assert sorted(OPTIONS) == [os.path.basename(p)[:-len("_bench.py")] for p in SCRIPTS] and len(SCRIPTS) == 21
    for path in SCRIPTS:
        text = open(path).read()
        assert "def timed" not in text and "def median_ms" not in text, path
        assert not [line for line in text.splitlines() if "_bench import" in line and line.lstrip().startswith(("from", "import"))], path


@pytest.mark.parametrize("path", SCRIPTS, ids=[os.path.basename(p)[:-3] for p in SCRIPTS])
def test_script_help_needs_no_torch_and_lists_its_options(path):
    name = os.path.basename(path)[:-len("_bench.py")]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", HELP_CHILD, path], capture_output=True, text=True, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    for option in ["--trials", "--warmup", "--out"] + OPTIONS[name]:
        assert option in p.stdout, (name, option)
    trials, warmup = DEFAULTS.get(name, ("15", "5"))
    usage = open(path).read().split('"""')[1]
    assert f"[--trials {trials}]" in usage and f"[--warmup {warmup}]" in usage


def test_script_defaults_are_the_ones_they_had():
    assert vars(H.parser().parse_args([])) == {"trials": 15, "warmup": 5, "out": None}
    assert vars(H.parser(trials=10, warmup=3, out="x.json").parse_args([])) == {"trials": 10, "warmup": 3, "out": "x.json"}


def test_emit_prints_the_line_and_writes_the_same_line(tmp_path, capsys):
    out = {"a": 1, "b": {"ms": 0.5}}
    H.emit(out, types.SimpleNamespace(out=str(tmp_path / "o.json")))
    assert capsys.readouterr().out == json.dumps(out) + "\n" == (tmp_path / "o.json").read_text()
    H.emit(out, types.SimpleNamespace(out=None))
    assert json.loads(capsys.readouterr().out) == out


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "bench_workloads.npz")) as z:
        return {k: z[k] for k in z.files}


def same(got, want):
    got = np.asarray(got)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_workload_generators_are_bit_equal_to_the_recorded_ones(golden):
    import ray_query_ref as R
    g = golden
    assert same(W.grid_transforms((2, 2), 1.5, np.random.default_rng(7)), g["grid_2x2"])
    assert same(W.grid_transforms((2, 2, 2), 0.75, np.random.default_rng(8), scale=(1.0, 1.0)), g["grid_2x2x2_rigid"])
    assert same(W.morton_order(g["points"]), g["morton_order"])
    assert same(W.near_points(g["positions"], 64, seed=3), g["near_points"])
    assert same(W.near_surface_points(g["positions"], g["grid_2x2"], 64, np.random.default_rng(9)), g["near_surface_points"])
    mats = g["mats"]
    params = types.SimpleNamespace(image_plane_width=0.7, aspect=9 / 16, camera_matrix=mats[0], camera_normal_matrix=mats[1],
                                   object_matrix=mats[2], object_normal_matrix=mats[3])
    o, d = W.camera_rays(params, 16, 9, R.xform)
    assert same(o, g["camera_origin"]) and same(d, g["camera_direction"])
    o, d, tmax = W.ao_rays(g["positions"], 64, seed=5)
    assert same(o, g["ao_origin"]) and same(d, g["ao_direction"]) and same(tmax, g["ao_tmax"])
    o, d = W.down_rays([-1, -2, 0], [3, 2, 1], 64, np.random.default_rng(10))
    assert same(o, g["down_origin"]) and same(d, g["down_direction"])
    o, d, tmax = W.through_rays(g["positions"], 64, seed=11)
    assert same(o, g["through_origin"]) and same(d, g["through_direction"]) and same(tmax, g["through_tmax"])

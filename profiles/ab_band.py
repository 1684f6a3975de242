"""The band rule of an A/B timing run, as code: is each timed row of this commit inside the parent's own spread?

The input is a .jsonl in which every line is one bench script's JSON line plus three tags: `script`, `build` ("parent" or
"this") and `round` (profiles/packed_walk_ab.jsonl is one; DESIGN §33 is what was decided on it).  A *row* is a numeric leaf
whose last key is `ms` or ends in `_ms`; the script and the leaf's dotted path name it.  For every row present in every round
of both builds, with lo and hi the parent's fastest and slowest round and w = hi - lo, the band is [lo - w, hi + w], and the
verdict is where this commit's median falls: inside, below (faster) or above.  A row that some round of either build lacks is
"incomplete" and never passes.

  python profiles/ab_band.py FILE.jsonl [--report-only PATTERN ...]
      prints the per-row table (markdown, DESIGN §33's columns) and then one JSON line of counts per verdict, gating and
      report-only apart.  A pattern is a shell-style wildcard matched against "script:row"; a row that matches is printed
      and counted but does not gate.  Exit status 1 when a gating row is above its band or incomplete, else 0.
  python profiles/ab_band.py append FILE.jsonl --script NAME --build parent|this --round N  < one JSON line
      tags a script's line and appends it to FILE.jsonl, so that an A/B run needs no wrapper of its own:
          python profiles/near_bench.py --no-million | python profiles/ab_band.py append ab.jsonl --script near_bench --build this --round 1

The worked example, §33's split:
  python profiles/ab_band.py profiles/packed_walk_ab.jsonl
      214 rows: 145 inside, 10 below, 59 above
  python profiles/ab_band.py profiles/packed_walk_ab.jsonl --report-only '*torch*'
      202 gating rows (135 inside, 10 below, 57 above) and 12 report-only rows (10 inside, 2 above): the twelve rows whose
      path names torch are the torch brute forces and, in the three `torch_vs_*` cells, the 2^12-query kernel launch beside
      them, which is launch overhead more than kernel

Only the standard library is used."""
import argparse
import fnmatch
import json
import statistics
import sys

VERDICTS = ("inside", "below", "above", "incomplete")
TAGS = ("script", "build", "round")


def timed_leaves(node, path=()):
    """(dotted path, value) of every numeric leaf whose last key is `ms` or ends in `_ms`"""
    if isinstance(node, dict):
        for key, value in node.items():
            yield from timed_leaves(value, path + (str(key),))
    elif isinstance(node, (int, float)) and not isinstance(node, bool) and path and (path[-1] == "ms" or path[-1].endswith("_ms")):
        yield ".".join(path), float(node)


def read_rows(lines):
    """{(script, row): {build: {round: ms}}} in the file's order, and {script: {build: set of rounds}}"""
    rows, rounds = {}, {}
    for line in lines:
        if not line.strip():
            continue
        record = json.loads(line)
        script, build, rnd = (record[tag] for tag in TAGS)
        rounds.setdefault(script, {"parent": set(), "this": set()})[build].add(rnd)
        for path, ms in timed_leaves({k: v for k, v in record.items() if k not in TAGS}):
            rows.setdefault((script, path), {"parent": {}, "this": {}})[build][rnd] = ms
    return rows, rounds


def judge(rows, rounds, report_only=()):
    """one dict per row: script, row, parent and this (the rounds' times in order), band, median, verdict, gating"""
    table = []
    for (script, path), times in rows.items():
        want = rounds[script]["parent"] | rounds[script]["this"]
        parent, this = ([times[build][r] for r in sorted(times[build])] for build in ("parent", "this"))
        entry = {"script": script, "row": path, "parent": parent, "this": this, "band": None, "median": None,
                 "gating": not any(fnmatch.fnmatchcase(f"{script}:{path}", p) for p in report_only)}
        if set(times["parent"]) != want or set(times["this"]) != want:
            entry["verdict"] = "incomplete"
        else:
            lo, hi = min(parent), max(parent)
            entry["band"] = (lo - (hi - lo), hi + (hi - lo))
            entry["median"] = statistics.median(this)
            entry["verdict"] = "below" if entry["median"] < entry["band"][0] else "above" if entry["median"] > entry["band"][1] else "inside"
        table.append(entry)
    return table


def summary(table):
    count = lambda gating: {v: sum(1 for e in table if e["gating"] == gating and e["verdict"] == v) for v in VERDICTS}   # noqa: E731
    gating, reported = count(True), count(False)
    return {"rows": len(table), "gating": gating, "report_only": reported, "passes": gating["above"] == 0 and gating["incomplete"] == 0}


def markdown(table):
    g = lambda x: f"{x:.4g}"   # noqa: E731
    lines = ["| script | row | parent, three runs (ms) | this commit, three runs (ms) | band | this commit's median |", "|---|---|---|---|---|---|"]
    for e in table:
        script = e["script"][:-len("_bench")] if e["script"].endswith("_bench") else e["script"]
        band = "—" if e["band"] is None else f"{g(e['band'][0])} – {g(e['band'][1])}"
        verdict = {"below": "below (faster)"}.get(e["verdict"], e["verdict"]) + ("" if e["gating"] else " (host work: does not gate)")
        last = verdict if e["median"] is None else f"{g(e['median'])}, {verdict}"
        lines.append(f"| {script} | `{e['row']}` | {', '.join(map(g, e['parent']))} | {', '.join(map(g, e['this']))} | {band} | {last} |")
    return "\n".join(lines)


def append(path, line, script, build, rnd):
    record = {"script": script, "build": build, "round": rnd, **json.loads(line)}
    with open(path, "a") as f:
        f.write(json.dumps(record) + "\n")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if argv[:1] == ["append"]:
        ap = argparse.ArgumentParser(prog="ab_band.py append")
        ap.add_argument("file")
        ap.add_argument("--script", required=True)
        ap.add_argument("--build", required=True, choices=("parent", "this"))
        ap.add_argument("--round", required=True, type=int)
        args = ap.parse_args(argv[1:])
        append(args.file, sys.stdin.read(), args.script, args.build, args.round)
        return 0
    ap = argparse.ArgumentParser(prog="ab_band.py")
    ap.add_argument("file")
    ap.add_argument("--report-only", nargs="*", default=[], metavar="PATTERN")
    args = ap.parse_args(argv)
    with open(args.file) as f:
        table = judge(*read_rows(f), args.report_only)
    print(markdown(table))
    result = summary(table)
    print(json.dumps(result))
    return 0 if result["passes"] else 1


if __name__ == "__main__":
    sys.exit(main())

"""Measures the joint unit parse (otg_unitparse_batch): HIP-event times of the forward pass and of the traceback, separately, on --alleles
(65 536) alleles of 100-2 000 bases per workload.  An allele is a window of a noisy stream of tracts of its unit set (3 % substitutions, 2 %
deletions, 2 % insertions).  The sets: CAG,CCG (4 lanes a task); the five HTT units (8 lanes); one 29-base unit with a 3-base one (32 lanes);
and CAG alone, the forward pass beside the unit alignment's kernel on the same task.  The yardstick is otg_unitalign_batch on the same alleles,
run once per unit of the set and summed: what a caller had to do before, and it gives no segments.  The script starts itself as a child
--rounds times; a child makes two warm-up calls and then --repeats calls of every workload, the parse and the yardstick alternating.  Prints
one JSON line: per workload the median ms of each round, DP cells per second of the forward pass (sum of L x sum of p over the tasks, over
the median), parse : yardstick, the traceback's share of the parse, segments per allele, and the run-to-run spread (the largest relative
distance between two rounds).
    python scripts/bench_unitparse.py [--alleles N] [--repeats R] [--rounds K] [--out profiles/unitparse_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otter_amd  # noqa: E402


def unit_sets(rng):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return {"cag_ccg": [b"CAG", b"CCG"], "htt": [b"CAG", b"CAA", b"CCG", b"CCA", b"CCT"], "p29_p3": [acgt[rng.integers(0, 4, 29)].tobytes(), b"GAA"],
            "cag": [b"CAG"]}


def workload(units, n, seed, stream=8 << 20):
    """n alleles of 100-2 000 bases, windows of a stream of tracts (5-40 copies of a unit of the set) with noise -> (arena with 64 bytes of
    slack, offsets, lengths)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts, total = [], 0
    while total < stream + stream // 16:
        u = units[int(rng.integers(0, len(units)))]
        parts.append(u * int(rng.integers(5, 41)))
        total += len(parts[-1])
    s = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    sub = rng.random(len(s)) < 0.03
    s[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    s = s[rng.random(len(s)) >= 0.02]
    ins = np.flatnonzero(rng.random(len(s)) < 0.02)
    s = np.insert(s, ins, acgt[rng.integers(0, 4, len(ins))])[:stream]
    lens = rng.integers(100, 2001, n).astype(np.uint32)
    off = rng.integers(0, len(s) - 2000, n).astype(np.uint64)
    return np.concatenate([s, np.zeros(64, dtype=np.uint8)]), off, lens


def child(a):
    sets = unit_sets(np.random.default_rng(1000))
    work, res = {}, {"ms": {}, "cells": {}, "segments_per_allele": {}}
    for i, (w, units) in enumerate(sets.items()):
        arena, off, ln = workload(units, a.alleles, 2000 + i)
        idx = np.arange(len(ln), dtype=np.uint32)
        work[w] = (arena, off, ln, units, idx, np.zeros(len(ln), dtype=np.uint32))
        res["cells"][w] = int(ln.astype(np.int64).sum()) * sum(len(u) for u in units)
    times = {w: {"forward": [], "trace": [], "unitalign": []} for w in sets}
    with otter_amd.Context(0) as ctx:
        for i in range(2 + a.repeats):
            for w, (arena, off, ln, units, idx, zero) in work.items():
                sums, _, _ = ctx.unitparse_batch(arena, off, ln, [units], idx, zero)
                fwd, back = ctx.unitparse_last_ms()
                each = 0.0
                for k in range(len(units)):                                # the yardstick: one unit alignment per unit of the set
                    ctx.unitalign_batch(arena, off, ln, units, idx, np.full(len(ln), k, dtype=np.uint32))
                    each += ctx.unitalign_last_ms()
                if i >= 2:
                    times[w]["forward"].append(fwd); times[w]["trace"].append(back); times[w]["unitalign"].append(each)
                res["segments_per_allele"][w] = round(float(sums["n_segments"].mean()), 2)
    res["ms"] = {w: {k: round(float(np.median(v)), 4) for k, v in t.items()} for w, t in times.items()}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alleles", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rounds = []
    for _ in range(a.rounds):
        env = dict(os.environ)
        env["OTG_NO_TORCH_PRELOAD"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--alleles", str(a.alleles), "--repeats", str(a.repeats)], capture_output=True,
                           text=True, env=env)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the child failed (%d)" % r.returncode)
        rounds.append(json.loads(lines[-1][7:]))
    out = {"alleles": a.alleles, "repeats": a.repeats, "rounds": a.rounds, "trace_budget_mb": os.environ.get("OTG_UNITPARSE_TRACE_MB", "default"), "workloads": {}}
    spread = 0.0
    for w in rounds[0]["ms"]:
        row = {}
        for part in ("forward", "trace", "unitalign"):
            ms = [c["ms"][w][part] for c in rounds]
            row[part + "_ms_rounds"] = ms
            row[part + "_ms"] = round(float(np.median(ms)), 4)
            if min(ms) > 0:
                spread = max(spread, (max(ms) - min(ms)) / min(ms))
        parse = row["forward_ms"] + row["trace_ms"]
        row["cells"] = rounds[0]["cells"][w]
        row["forward_cells_per_s"] = round(row["cells"] / (row["forward_ms"] / 1e3), 0) if row["forward_ms"] else None
        row["parse_over_unitalign"] = round(parse / row["unitalign_ms"], 3) if row["unitalign_ms"] else None
        row["forward_over_unitalign"] = round(row["forward_ms"] / row["unitalign_ms"], 3) if row["unitalign_ms"] else None
        row["trace_share"] = round(row["trace_ms"] / parse, 3) if parse else None
        row["segments_per_allele"] = rounds[0]["segments_per_allele"][w]
        out["workloads"][w] = row
    out["run_to_run_spread"] = round(spread, 4)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

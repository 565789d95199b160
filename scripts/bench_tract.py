"""Measures the tract mode of the copy numbers (otg_tract_batch) next to the global unit alignment (otg_unitalign_batch) on the same alleles:
HIP-event times on --alleles alleles, the workloads and units of scripts/bench_unitalign.py (noisy repeats of 100-2 000 bases of one unit per
workload: p = 3, 7, 13, 29: the segment classes of 4, 8, 16 and 32 lanes; p = 37: a whole wave; p = 100 and 200: 2 and 4 positions per
lane), every allele between 0-50 random flank bases on both sides.  Three arms: packed segments on the narrow key (the default), every task on
a whole wave (OTG_TRACT_SEG64=1), every task on the 64-bit key (OTG_TRACT_WIDE=1).  The switches are read once per process, so the script starts
itself as a child per arm, in turn, --rounds times; a child makes two warm-up calls and then --repeats calls of every workload, alternating.
Prints one JSON line: per workload and arm the median ms of each round of the local pass and of the second pass (the sub-rows, the global
alignment of the tracts, the merge), from the same run the ms of otg_unitalign_batch on the same alleles, DP cells per second of the local
pass (sum of L x p over the tasks, over the median), the ratios local : global, seg64 : packed and wide : narrow, and the run-to-run spread
(the largest relative distance between two rounds of one arm).
    python scripts/bench_tract.py [--alleles N] [--repeats R] [--rounds K] [--out profiles/tract_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import otter_amd  # noqa: E402
from bench_unitalign import UNITS, workload  # noqa: E402

ARMS = {"packed": None, "seg64": "OTG_TRACT_SEG64", "wide": "OTG_TRACT_WIDE"}


def flanked(p, n, seed):
    """the workload of bench_unitalign.py with every allele copied out between 0-50 random bases on both sides -> (arena with 64 bytes of
    slack, offsets, lengths, unit)"""
    stream, off, lens, unit = workload(p, n, seed)
    rng = np.random.default_rng(seed + 7 * p)
    fl, fr = rng.integers(0, 51, n), rng.integers(0, 51, n)
    total = (fl + lens + fr).astype(np.int64)
    start = np.cumsum(total) - total
    arena = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(total.sum()) + 64)]
    arena[-64:] = 0
    owner = np.repeat(np.arange(n), lens.astype(np.int64))
    within = np.arange(len(owner), dtype=np.int64) - np.repeat(np.cumsum(lens.astype(np.int64)) - lens, lens.astype(np.int64))
    arena[start[owner] + fl[owner] + within] = stream[off.astype(np.int64)[owner] + within]
    return arena, start.astype(np.uint64), total.astype(np.uint32), unit


def child(a):
    res = {"arm": a.arm, "cells": {}}
    sets = {}
    for p in UNITS:
        arena, off, ln, unit = flanked(p, a.alleles, 1000)
        sets[p] = (arena, off, ln, [unit], np.arange(len(ln), dtype=np.uint32), np.zeros(len(ln), dtype=np.uint32))
        res["cells"]["p%d" % p] = int(ln.astype(np.int64).sum()) * p
    times = {("p%d" % p): {"local": [], "second": [], "global": []} for p in UNITS}
    tracts = {}
    with otter_amd.Context(0) as ctx:
        for i in range(2 + a.repeats):
            for p in UNITS:
                rec = ctx.tract_batch(*sets[p])
                both, local = ctx.tract_last_ms()
                ctx.unitalign_batch(*sets[p])
                if i >= 2:
                    t = times["p%d" % p]
                    t["local"].append(local); t["second"].append(both - local); t["global"].append(ctx.unitalign_last_ms())
                tracts["p%d" % p] = [int((rec["flags"] == 0).sum()), float((rec["end"] - rec["begin"]).astype(np.int64).sum()) / float(sets[p][2].astype(np.int64).sum())]
    res["ms"] = {w: {k: round(float(np.median(v)), 4) for k, v in t.items()} for w, t in times.items()}
    res["tracts"] = tracts
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alleles", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--arm", default="packed")
    a = ap.parse_args()
    if a.child:
        return child(a)
    arms = {arm: [] for arm in ARMS}
    for _ in range(a.rounds):
        for arm, switch in ARMS.items():
            env = {k: v for k, v in os.environ.items() if not k.startswith(("OTG_TRACT_", "OTG_UNITALIGN_"))}
            env["OTG_NO_TORCH_PRELOAD"] = "1"
            if switch:
                env[switch] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--alleles", str(a.alleles), "--repeats", str(a.repeats)],
                               capture_output=True, text=True, env=env)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("the %s child failed (%d)" % (arm, r.returncode))
            arms[arm].append(json.loads(lines[-1][7:]))
            sys.stderr.write("%s: round %d of %d measured\n" % (arm, len(arms[arm]), a.rounds)); sys.stderr.flush()
    out = {"alleles": a.alleles, "repeats": a.repeats, "rounds": a.rounds, "flank_bases": "0-50 on both sides", "workloads": {}}
    spread = 0.0
    for w in arms["packed"][0]["ms"]:
        row = {"cells": arms["packed"][0]["cells"][w], "tracts_found": arms["packed"][0]["tracts"][w][0],
               "tract_share_of_bases": round(arms["packed"][0]["tracts"][w][1], 4)}
        for arm in arms:
            for part in ("local", "second", "global"):
                ms = [c["ms"][w][part] for c in arms[arm]]
                row["%s_%s_ms_rounds" % (arm, part)] = ms
                row["%s_%s_ms" % (arm, part)] = round(float(np.median(ms)), 4)
                if min(ms) > 0:
                    spread = max(spread, (max(ms) - min(ms)) / min(ms))
            row["%s_local_cells_per_s" % arm] = round(row["cells"] / (row["%s_local_ms" % arm] / 1e3), 0)
        row["local_over_global"] = round(row["packed_local_ms"] / row["packed_global_ms"], 3)
        row["seg64_over_packed"] = round(row["seg64_local_ms"] / row["packed_local_ms"], 3)
        row["wide_over_narrow"] = round(row["wide_local_ms"] / row["packed_local_ms"], 3)
        out["workloads"][w] = row
    out["run_to_run_spread"] = round(spread, 4)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

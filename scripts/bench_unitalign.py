"""Measures the cyclic unit alignment (otg_unitalign_batch, otg_unitalign_motifs): HIP-event times on --alleles (65 536) alleles of 100-2 000
bases, noisy repeats of one unit per workload (p = 3, 7, 13, 29: the segment classes of 4, 8, 16 and 32 lanes; p = 37: a whole wave; p = 100 and
200: 2 and 4 positions per lane), and of the motif_batch + unitalign_motifs chain on the allele set of scripts/bench_motif.py (BASELINE
configs[3], --chain-regions regions).  The packed segment classes are measured against OTG_UNITALIGN_SEG64=1, this code's own
one-task-per-wave path.  That switch is read once per process, so the script starts itself as a child per arm, packed and seg64 in turn,
--rounds times; a child makes two warm-up calls and then --repeats calls of every workload, alternating.  Prints one JSON line: per workload
and arm the median ms of each round, DP cells per second (sum of L x p over the tasks, over the median), the lane use (cells over the unit
positions a wave holds x the longest allele of every wave, from the kernel's own binning), the packed : seg64 ratio, and the run-to-run
spread (the largest relative distance between two rounds of one arm).
    python scripts/bench_unitalign.py [--alleles N] [--chain-regions N] [--repeats R] [--rounds K] [--out profiles/unitalign_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otter_amd  # noqa: E402
from otter_amd import synth  # noqa: E402

UNITS = (3, 7, 13, 29, 37, 100, 200)


def workload(p, n, seed, stream=8 << 20):
    """n alleles of 100-2 000 bases, each a window of one noisy repeat of a random p-base unit (3 % substitutions, 2 % deletions, 2 %
    insertions over `stream` bases) -> (arena with 64 bytes of slack, offsets, lengths, unit)"""
    rng = np.random.default_rng(seed + p)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    unit = acgt[rng.integers(0, 4, p)]
    s = unit[np.arange(stream + stream // 16) % p]
    sub = rng.random(len(s)) < 0.03
    s[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    s = s[rng.random(len(s)) >= 0.02]
    ins = np.flatnonzero(rng.random(len(s)) < 0.02)
    s = np.insert(s, ins, acgt[rng.integers(0, 4, len(ins))])[:stream]
    lens = rng.integers(100, 2001, n).astype(np.uint32)
    off = rng.integers(0, len(s) - 2000, n).astype(np.uint64)
    return np.concatenate([s, np.zeros(64, dtype=np.uint8)]), off, lens, unit.tobytes()


def bucket(L):
    """ua_bucket of otg_unitalign_core.hpp"""
    if L < 256:
        return L >> 4
    e = int(L).bit_length() - 1
    return 16 + (e - 8) * 16 + ((L >> (e - 4)) & 15)


def lane_use(lens, p, seg64):
    """cells over issued lane-rows for tasks of one unit length, binned as ua_classify bins them"""
    lanes = 64 if (seg64 or p > 32) else max(4, 1 << (p - 1).bit_length())
    per_wave = 64 // lanes
    order = sorted((L for L in lens if L > 0), key=lambda L: -bucket(L))      # (inside a bucket the kernel's order is that of its atomics)
    rows = sum(max(order[i:i + per_wave]) for i in range(0, len(order), per_wave))
    slots = 64 * (1 if p <= 64 else 2 if p <= 128 else 4)                    # unit positions a wave holds
    return float(sum(order)) * p / (slots * rows) if rows else 0.0


def child(a):
    seg64 = os.environ.get("OTG_UNITALIGN_SEG64") == "1"
    res = {"seg64": seg64, "ms": {}, "cells": {}, "lane_use": {}}
    sets = {}
    for p in UNITS:
        arena, off, ln, unit = workload(p, a.alleles, 1000)
        sets[p] = (arena, off, ln, [unit], np.arange(len(ln), dtype=np.uint32), np.zeros(len(ln), dtype=np.uint32))
        res["cells"]["p%d" % p] = int(ln.astype(np.int64).sum()) * p
        res["lane_use"]["p%d" % p] = round(lane_use([int(x) for x in ln], p, seg64), 4)
    b = synth.config_batch(3, a.chain_regions, workers=min(16, os.cpu_count() or 1))
    times = {("p%d" % p): [] for p in UNITS}
    times["chain_motif"], times["chain_unitalign"] = [], []
    with otter_amd.Context(0) as ctx:
        for i in range(2 + a.repeats):
            for p in UNITS:
                ctx.unitalign_batch(*sets[p])
                if i >= 2:
                    times["p%d" % p].append(ctx.unitalign_last_ms())
            mrec, _ = ctx.motif_batch(b["arena"], b["seq_off"], b["seq_len"])
            rec = ctx.unitalign_motifs()
            if i >= 2:
                times["chain_motif"].append(sum(ctx.motif_last_ms())); times["chain_unitalign"].append(ctx.unitalign_last_ms())
    Lc, pc = b["seq_len"].astype(np.int64), mrec["period"].astype(np.int64)
    res["cells"]["chain_unitalign"] = int((Lc * pc)[rec["flags"] == 0].sum())
    res["chain_alleles"] = int(len(Lc)); res["chain_aligned"] = int((rec["flags"] == 0).sum())
    res["ms"] = {k: round(float(np.median(v)), 4) for k, v in times.items()}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alleles", type=int, default=65536)
    ap.add_argument("--chain-regions", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    arms = {"packed": [], "seg64": []}
    for _ in range(a.rounds):
        for arm in ("packed", "seg64"):
            env = {k: v for k, v in os.environ.items() if not k.startswith("OTG_UNITALIGN_")}
            env["OTG_NO_TORCH_PRELOAD"] = "1"
            if arm == "seg64":
                env["OTG_UNITALIGN_SEG64"] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--alleles", str(a.alleles), "--chain-regions", str(a.chain_regions),
                                "--repeats", str(a.repeats)], capture_output=True, text=True, env=env)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("the %s child failed (%d)" % (arm, r.returncode))
            arms[arm].append(json.loads(lines[-1][7:]))
    out = {"alleles": a.alleles, "chain_regions": a.chain_regions, "repeats": a.repeats, "rounds": a.rounds, "workloads": {}}
    spread = 0.0
    for w in arms["packed"][0]["ms"]:
        row = {}
        for arm in arms:
            ms = [c["ms"][w] for c in arms[arm]]
            row[arm + "_ms_rounds"] = ms
            row[arm + "_ms"] = round(float(np.median(ms)), 4)
            if min(ms) > 0:
                spread = max(spread, (max(ms) - min(ms)) / min(ms))
        cells = arms["packed"][0]["cells"].get(w)
        if cells:
            row["cells"] = cells
            row["packed_cells_per_s"] = round(cells / (row["packed_ms"] / 1e3), 0)
            row["seg64_cells_per_s"] = round(cells / (row["seg64_ms"] / 1e3), 0)
        if w in arms["packed"][0]["lane_use"]:
            row["packed_lane_use"] = arms["packed"][0]["lane_use"][w]; row["seg64_lane_use"] = arms["seg64"][0]["lane_use"][w]
        row["seg64_over_packed"] = round(row["seg64_ms"] / row["packed_ms"], 3) if row["packed_ms"] else None
        out["workloads"][w] = row
    out["run_to_run_spread"] = round(spread, 4)
    out["chain_alleles"] = arms["packed"][0]["chain_alleles"]; out["chain_aligned"] = arms["packed"][0]["chain_aligned"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

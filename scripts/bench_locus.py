"""Measures the locus mode (otg_locus_batch) next to the two operators it is built from, on the same alleles: HIP-event times on --alleles
flanked alleles per unit-set shape: CAG,CCG (8 lanes); HTT's five units (16 lanes); GAA,AGAA (8 lanes); one unit of 37 bases (a whole wave);
one unit of 256 bases (4 positions per lane).  An allele is a core of 100-2 000 bases (noisy tracts of the set's units, drawn from a pool of
--pool cores per shape) between 0-50 random flank bases on both sides.  Baselines, neither of them the code under test: the forward pass of
the global joint parse (otg_unitparse_batch, otg_unitparse_last_ms) for every shape, and for the two single-unit shapes the local pass of the
tract mode (otg_tract_batch, otg_tract_last_ms), whose kernel this change does not touch.  Three arms: packed tasks on the narrow key (the
default), every task on a whole wave (OTG_LOCUS_SEG64=1), every task on the 64-bit key (OTG_LOCUS_WIDE=1).  The switches are read once per
process, so the script starts itself as a child per arm, in turn, --rounds times; a child makes two warm-up calls and then --repeats calls of
every workload, alternating.  Prints one JSON line: per workload and arm the median ms of each round of the local pass and of the second
pass, from the same run the forward ms of the global parse (and the tract mode's local ms), DP cells per second of the local pass (sum of L x
the set's unit bases over the tasks, over the median), the ratios local : parse forward, local : tract local, seg64 : packed and wide :
narrow, and the run-to-run spread (the largest relative distance between two rounds of one arm).
    python scripts/bench_locus.py [--alleles N] [--repeats R] [--rounds K] [--out profiles/locus_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otter_amd  # noqa: E402

ARMS = {"packed": None, "seg64": "OTG_LOCUS_SEG64", "wide": "OTG_LOCUS_WIDE"}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def shapes(seed=1000):
    rng = np.random.default_rng(seed)
    unit = lambda p: ACGT[rng.integers(0, 4, p)].tobytes()
    return {"CAG_CCG": [b"CAG", b"CCG"], "HTT": [b"CAG", b"CAA", b"CCG", b"CCA", b"CCT"], "GAA_AGAA": [b"GAA", b"AGAA"], "p37": [unit(37)], "p256": [unit(256)]}


def core(rng, units, L, rate=0.03):
    """L bases of tracts of the set's units, then substitutions, insertions and deletions at `rate` per base, vectorised"""
    parts, have = [], 0
    while have < L + L // 8 + 8:
        u = np.frombuffer(units[int(rng.integers(0, len(units)))], dtype=np.uint8)
        t = np.tile(u, int(rng.integers(3, 40)) if len(u) < 37 else int(rng.integers(1, 6)))
        parts.append(t); have += len(t)
    s = np.concatenate(parts)
    x = rng.random(len(s))
    s = np.where(x < rate / 3, ACGT[rng.integers(0, 4, len(s))], s)         # substitutions
    s = s[(x < rate / 3) | (x >= 2 * rate / 3)]                              # deletions
    ins = np.flatnonzero(rng.random(len(s)) < rate / 3)
    return np.insert(s, ins, ACGT[rng.integers(0, 4, len(ins))])[:L]


def workload(units, n, pool, seed):
    """-> (arena with 64 bytes of slack, offsets, lengths)"""
    rng = np.random.default_rng(seed)
    cores = [core(rng, units, int(rng.integers(100, 2001))) for _ in range(pool)]
    clen = np.array([len(c) for c in cores], dtype=np.int64)
    cstart = np.cumsum(clen) - clen
    stream = np.concatenate(cores)
    pick = rng.integers(0, pool, n)
    lens = clen[pick]
    fl, fr = rng.integers(0, 51, n), rng.integers(0, 51, n)
    total = fl + lens + fr
    start = np.cumsum(total) - total
    arena = ACGT[rng.integers(0, 4, int(total.sum()) + 64)]
    arena[-64:] = 0
    owner = np.repeat(np.arange(n), lens)
    within = np.arange(len(owner), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    arena[start[owner] + fl[owner] + within] = stream[cstart[pick][owner] + within]
    return arena, start.astype(np.uint64), total.astype(np.uint32)


def child(a):
    res = {"arm": a.arm, "cells": {}}
    sets = {}
    for k, (w, units) in enumerate(shapes().items()):
        arena, off, ln = workload(units, a.alleles, a.pool, 2000 + k)
        n = len(ln)
        sets[w] = (arena, off, ln, units, np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
        res["cells"][w] = int(ln.astype(np.int64).sum()) * sum(len(u) for u in units)
    times = {w: {"local": [], "second": [], "parse_forward": [], "tract_local": []} for w in sets}
    found = {}
    with otter_amd.Context(0) as ctx:
        for i in range(2 + a.repeats):
            for w, (arena, off, ln, units, ts, tq) in sets.items():
                rec = ctx.locus_batch(arena, off, ln, [units], ts, tq)[0]
                both, local = ctx.locus_last_ms()
                ctx.unitparse_batch(arena, off, ln, [units], ts, tq)
                fwd = ctx.unitparse_last_ms()[0]
                tl = None
                if len(units) == 1:
                    ctx.tract_batch(arena, off, ln, units, ts, tq)
                    tl = ctx.tract_last_ms()[1]
                if i >= 2:
                    t = times[w]
                    t["local"].append(local); t["second"].append(both - local); t["parse_forward"].append(fwd)
                    if tl is not None:
                        t["tract_local"].append(tl)
                found[w] = [int((rec["flags"] == 0).sum()), float((rec["end"] - rec["begin"]).astype(np.int64).sum()) / float(ln.astype(np.int64).sum()),
                            float(rec["switches"].astype(np.int64).sum()) / len(ln)]
        res["tiers"] = list(ctx.locus_last_tiers())
    res["ms"] = {w: {k: round(float(np.median(v)), 4) for k, v in t.items() if v} for w, t in times.items()}
    res["found"] = found
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alleles", type=int, default=65536)
    ap.add_argument("--pool", type=int, default=1024)
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
            env = {k: v for k, v in os.environ.items() if not k.startswith(("OTG_LOCUS_", "OTG_TRACT_", "OTG_UNITPARSE_", "OTG_UNITALIGN_"))}
            env["OTG_NO_TORCH_PRELOAD"] = "1"
            if switch:
                env[switch] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--alleles", str(a.alleles), "--pool", str(a.pool), "--repeats",
                                str(a.repeats)], capture_output=True, text=True, env=env)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("the %s child failed (%d)" % (arm, r.returncode))
            arms[arm].append(json.loads(lines[-1][7:]))
            sys.stderr.write("%s: round %d of %d measured\n" % (arm, len(arms[arm]), a.rounds)); sys.stderr.flush()
    out = {"alleles": a.alleles, "pool": a.pool, "repeats": a.repeats, "rounds": a.rounds, "flank_bases": "0-50 on both sides", "workloads": {}}
    spread = 0.0
    for w in arms["packed"][0]["ms"]:
        f = arms["packed"][0]["found"][w]
        row = {"cells": arms["packed"][0]["cells"][w], "tracts_found": f[0], "tract_share_of_bases": round(f[1], 4), "switches_per_allele": round(f[2], 3)}
        for arm in arms:
            for part in arms[arm][0]["ms"][w]:
                ms = [c["ms"][w][part] for c in arms[arm]]
                row["%s_%s_ms_rounds" % (arm, part)] = ms
                row["%s_%s_ms" % (arm, part)] = round(float(np.median(ms)), 4)
                if min(ms) > 0:
                    spread = max(spread, (max(ms) - min(ms)) / min(ms))
            row["%s_local_cells_per_s" % arm] = round(row["cells"] / (row["%s_local_ms" % arm] / 1e3), 0)
        row["local_over_parse_forward"] = round(row["packed_local_ms"] / row["packed_parse_forward_ms"], 3)
        if "packed_tract_local_ms" in row:
            row["local_over_tract_local"] = round(row["packed_local_ms"] / row["packed_tract_local_ms"], 3)
        row["seg64_over_packed"] = round(row["seg64_local_ms"] / row["packed_local_ms"], 3)
        row["wide_over_narrow"] = round(row["wide_local_ms"] / row["packed_local_ms"], 3)
        out["workloads"][w] = row
    out["tiers_packed"] = arms["packed"][0]["tiers"]
    out["tiers_wide"] = arms["wide"][0]["tiers"]
    out["run_to_run_spread"] = round(spread, 4)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Measures the repeat structure (otg_repeat_batch) next to the motif annotation (otg_motif_batch) on the same alleles: the HIP-event times
of the runs and the select phase against the count and the reduce phase, which sweep the same planes.  Two batches: the 300 alleles of
tests/motif_cases.random_set(), and --alleles (default 65 536) alleles of 100-2 000 bases, half random sequence and half random units of
1-40 bases with 0-3 substitutions.  Warm-up calls, then --repeats calls of each, alternating; prints one JSON line with the medians.
    python scripts/bench_repeat.py [--alleles N] [--max-period P] [--repeats R] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import motif_cases as Cs  # noqa: E402


def large_set(n, seed=31):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in range(n):
        L = int(rng.integers(100, 2001))
        if i % 2 == 0:
            s = acgt[rng.integers(0, 4, L)]
        else:
            u = acgt[rng.integers(0, 4, int(rng.integers(1, 41)))]
            s = np.tile(u, L // len(u) + 1)[:L].copy()
            for _ in range(int(rng.integers(0, 4))):
                j = int(rng.integers(0, L))
                s[j] = acgt[(int(np.flatnonzero(acgt == s[j])[0]) + int(rng.integers(1, 4))) % 4]
        out.append(s.tobytes())
    return out


def measure(ctx, seqs, max_period, repeats):
    arena, off, ln = abi.pack_seqs(seqs)
    rep, mot = [], []
    for i in range(2 + repeats):
        sums, _, segs = ctx.repeat_batch(arena, off, ln, max_period=max_period)
        r = ctx.repeat_last_ms()
        ctx.motif_batch(arena, off, ln, max_period=max_period)
        m = ctx.motif_last_ms()
        if i >= 2:
            rep.append(r); mot.append(m)
    med = lambda v, k: round(float(np.median([x[k] for x in v])), 3)
    return {"alleles": len(seqs), "bases": int(ln.sum()), "segments": int(len(segs)), "repeat_segments": int(sums["n_repeats"].sum()),
            "repeat_runs_ms_median": med(rep, 0), "repeat_select_ms_median": med(rep, 1), "motif_count_ms_median": med(mot, 0),
            "motif_reduce_ms_median": med(mot, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alleles", type=int, default=65536)
    ap.add_argument("--max-period", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with otter_amd.Context(0) as ctx:
        res = {"max_period": a.max_period, "repeats": a.repeats, "random_set": measure(ctx, Cs.random_set(), a.max_period, a.repeats),
               "large_set": measure(ctx, large_set(a.alleles), a.max_period, a.repeats)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

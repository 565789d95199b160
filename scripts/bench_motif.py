"""Measures the motif annotation (otg_motif_batch) on the allele set of BASELINE configs[3] (5 000 regions x 101 alleles of 1-5 kb): the
HIP-event time of the pack and match-count kernels and of the reduce-and-unit kernel at --max-period (default 256), next to the k-mer
counting of the same alleles at k = 3 (otg_kmer_usage_last_ms) as a scale mark.  Warm-up calls, then --repeats calls of each, alternating;
prints one JSON line with the medians, the spread, and the base compares per second (sum over alleles of sum over p <= P of L - p).
    python scripts/bench_motif.py [--regions N] [--max-period P] [--repeats R] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otter_amd  # noqa: E402
from otter_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=synth.CONFIGS[3]["n_regions"])
    ap.add_argument("--max-period", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    b = synth.config_batch(3, a.regions, workers=min(16, os.cpu_count() or 1))
    arena, off, ln = b["arena"], b["seq_off"], b["seq_len"]
    L = ln.astype(np.int64)
    P = np.minimum(a.max_period, L // 2)
    compares = int((P * L - P * (P + 1) // 2).sum())
    motif, kmer = [], []
    with otter_amd.Context(0) as ctx:
        for i in range(2 + a.repeats):
            rec, _ = ctx.motif_batch(arena, off, ln, max_period=a.max_period)
            m = ctx.motif_last_ms()
            ctx.kmer_usage_batch(arena, off, ln, k=3, device_tensor=True)
            k = ctx.kmer_usage_last_ms()
            if i >= 2:
                motif.append(m); kmer.append(k)
    cnt = np.array([m[0] for m in motif]); red = np.array([m[1] for m in motif]); km = np.array([k[0] + k[1] for k in kmer])
    tot = cnt + red
    res = {"alleles": int(len(ln)), "bases": int(L.sum()), "max_period": a.max_period, "repeats": a.repeats, "base_compares": compares,
           "motif_count_ms_median": round(float(np.median(cnt)), 3), "motif_reduce_ms_median": round(float(np.median(red)), 3),
           "motif_ms_median": round(float(np.median(tot)), 3), "motif_ms_min": round(float(tot.min()), 3), "motif_ms_max": round(float(tot.max()), 3),
           "compares_per_s": round(compares / (float(np.median(cnt)) / 1e3), 0),
           "kmer_k3_ms_median": round(float(np.median(km)), 3), "kmer_k3_ms_min": round(float(km.min()), 3), "kmer_k3_ms_max": round(float(km.max()), 3),
           "alleles_with_period": int((rec["period"] > 0).sum())}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

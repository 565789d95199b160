#!/usr/bin/env python3
"""What the edit metric of the genotype clustering costs: scripts/genotype_metric_probe.py [--config C] [--regions R] [--repeats N] [--out FILE]
The configs[C] genotype batch as bench.py --full builds it (default 3: 5 000 regions x 101 alleles of 1-5 kb; --regions cuts it) through
otg_genotype_cluster_metric_batch in both modes and, next to them, otg_genotype_cluster_batch: one untimed warm-up each, then `repeats`
rounds in which the three alternate.  Prints one JSON line (and writes it to --out): total pairs and n_aligned, median / min / max of align_ms,
cluster_ms and the kernel time, regions/s from the kernel time, and the share of regions whose genotype count differs between the modes."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import otter_amd  # noqa: E402
from otter_amd import abi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3); ap.add_argument("--regions", type=int, default=0)
ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--out", default=None)
a = ap.parse_args()

b = synth.config_batch(a.config)
n = len(b["n_alleles"]) if not a.regions else min(a.regions, len(b["n_alleles"]))
na = int(b["first_allele"][n])
args = (b["arena"], b["seq_off"][:na].copy(), b["seq_len"][:na].copy(), np.ascontiguousarray(b["first_allele"][:n]), b["n_alleles"][:n].copy())
A = b["n_alleles"][:n].astype(np.int64)
P = abi.default_params()


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


with otter_amd.Context(0) as ctx:
    def run(mode):
        if mode == "old":
            res = ctx.genotype_cluster_batch(P, *args)
            return res, {"kernel_ms": ctx.last_kernel_ms()}
        res = ctx.genotype_cluster_metric_batch(P, *args, metric=mode)
        al, cl = ctx.genotype_metric_last_ms()
        return res, {"align_ms": al, "cluster_ms": cl, "kernel_ms": ctx.last_kernel_ms()}
    modes = ("old", "length", "edit")
    first = {m: run(m)[0] for m in modes}                    # warm-up: workspaces allocated, kernels loaded
    rounds = {m: [] for m in modes}
    for _ in range(a.repeats):
        for m in modes:
            rounds[m].append(run(m)[1])

for i in range(6):
    assert np.array_equal(first["old"][i], first["length"][i], equal_nan=True), i
command = " ".join(x for i, x in enumerate(sys.argv) if x != "--out" and sys.argv[i - 1] != "--out")      # where the line goes is no part of the measurement
res = {"bench": "genotype_metric", "command": command, "config": a.config, "regions": n, "alleles": na,
       "pairs": int((A * (A - 1) // 2).sum()), "n_aligned": first["edit"][7], "repeats": a.repeats,
       "regions_differ_share": float((first["edit"][4] != first["length"][4]).mean()),
       "genotypes_per_region": {"length": float(first["length"][4].mean()), "edit": float(first["edit"][4].mean())}}
for m in modes:
    res[m] = {k: stat([r[k] for r in rounds[m]]) for k in rounds[m][0]}
    res[m]["regions_per_s"] = n / (res[m]["kernel_ms"]["median"] / 1e3)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")

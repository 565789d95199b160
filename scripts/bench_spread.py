"""Measures the spread operator (otg_assemble_spread) on a resident assemble batch: HIP-event times of the call's device work summed, of the reads' locus
call, of the consensus locus call and of the stats kernel (otg_spread_last_ms), next to the local pass of the reads' locus call
(otg_locus_last_ms afterwards), which is the number the stats kernel is judged against.  Workload: --regions regions x --reads reads, two
alleles of one random unit of 2-6 bases per region (60-400 bases, 20-40 base flanks, HiFi-like errors, copy numbers scattered by 0-3).
Then the stats kernel alone at member counts 16, 64, 256 and 1 024: homozygous regions of that depth whose reads are identical, so that each
is one allele with exactly that many members (the JSON reports the smallest and the largest member count that occurred); 256 is the last
size of the register tier, 1 024 runs on the re-read tier; max_cov raised.  One assemble run per workload, two warm-up calls of
the operator, then --repeats calls; medians.  Prints one JSON line.
    python scripts/bench_spread.py [--regions N] [--reads D] [--repeats R] [--out profiles/spread_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otter_amd  # noqa: E402
from otter_amd import abi, synth  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def batch_of(rng, n_regions, depth, het=True):
    """-> (batch, unit_sets, region_set): region r has its own one-unit set.  het=False: one allele per region, its reads without errors and
    at one copy number, so that the region is one cluster and the allele has exactly `depth` members"""
    rate, split = synth.ERR["hifi"]
    chunks, reads, regions, unit_sets = [], [], [], []
    pos = 0
    for r in range(n_regions):
        p = int(rng.integers(2, 7))
        unit = rng.integers(0, 4, p, dtype=np.uint8)
        while np.all(unit == unit[0]):
            unit = rng.integers(0, 4, p, dtype=np.uint8)
        fl, fr = rng.integers(0, 4, int(rng.integers(20, 41)), dtype=np.uint8), rng.integers(0, 4, int(rng.integers(20, 41)), dtype=np.uint8)
        ca = int(rng.integers(max(2, 40 // p), 200 // p))
        cb = ca + int(rng.integers(max(4, ca // 3), ca + 4)) if het else ca
        first = len(reads)
        for i in range(depth):
            c = max(1, (ca if i % 2 == 0 else cb) + int(rng.integers(-3, 4)) * int(rng.random() < 0.3)) if het else ca
            tmpl = np.concatenate([fl, np.tile(unit, c), fr])
            seq = ACGT[synth._mutate(rng, tmpl, rate, split) if het else tmpl]
            chunks.append(seq)
            reads.append((pos, seq.size, 1, 1, 0, -1, -1, 0, seq.size))
            pos += seq.size
        regions.append((first, depth, 0, 0, 0, 0))
        unit_sets.append([ACGT[unit].tobytes()])
    arena = np.concatenate(chunks + [np.zeros(64, dtype=np.uint8)])
    return {"arena": arena, "reads": np.array(reads, dtype=abi.read_dt), "regions": np.array(regions, dtype=abi.region_dt)}, unit_sets, list(range(n_regions))


def measure(ctx, batch, unit_sets, region_set, repeats, max_cov):
    res = ctx.assemble(abi.default_params(max_cov=max_cov), batch)
    t = {"total": [], "reads_locus": [], "consensus_locus": [], "stats": [], "reads_local_pass": []}
    for i in range(2 + repeats):
        rec = ctx.assemble_spread(unit_sets, region_set)[0]
        ms = ctx.spread_last_ms()
        local = ctx.locus_last_ms()[1]
        if i >= 2:
            for k, v in zip(t, list(ms) + [local]):
                t[k].append(v)
    out = {k + "_ms": round(float(np.median(v)), 4) for k, v in t.items()}
    out.update(alleles=int(len(rec)), reads=int(len(batch["reads"])), called=int(rec["n_called"].sum()),
               members_per_allele_min=int(rec["n_called"].min()) if len(rec) else 0, members_per_allele_max=int(rec["n_called"].max()) if len(rec) else 0,
               stats_over_reads_local_pass=round(out["stats_ms"] / out["reads_local_pass_ms"], 4) if out["reads_local_pass_ms"] else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=4096)
    ap.add_argument("--reads", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"regions": a.regions, "reads_per_region": a.reads, "repeats": a.repeats, "warmup": 2}
    with otter_amd.Context(0) as ctx:
        out["workload"] = measure(ctx, *batch_of(np.random.default_rng(4000), a.regions, a.reads), a.repeats, 200)
        out["stats_by_members"] = {}
        for m, n in ((16, 256), (64, 64), (256, 16), (1024, 8)):
            out["stats_by_members"][str(m)] = dict(measure(ctx, *batch_of(np.random.default_rng(4100 + m), n, m, het=False), a.repeats, 2048), regions=n)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

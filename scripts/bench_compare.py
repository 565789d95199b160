"""regions/s of otg_compare_files (`otter compare` from files to text) on a synthetic job, plus the device time of the two passes of
otg_edit_align_batch (score chain, provenance pass) on the same pairs.  10 000 regions of configs[1] lengths (1-5 kb); per region two truth
alleles (two haplotypes) and two assembled alleles (a near copy of the first haplotype, and the second one).  Prints one JSON line.
usage: python scripts/bench_compare.py [--regions N] [--threads T] [--repeat R] [--workdir DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
from compare_fixtures import aux, write_allele_bam, oriented  # noqa: E402
from helpers import rand_seq, mutate  # noqa: E402


def make_job(d, n, seed=1):
    rng = np.random.default_rng(seed)
    chrom, step = "chrB", 6000
    trecs, qrecs, pairs = [], [], []
    with open(os.path.join(d, "regions.bed"), "w") as f:
        for r in range(n):
            s, e = 1000 + step * r, 1000 + step * r + 100
            ta = aux("ta", "Z", "%s:%d-%d" % (chrom, s, e))
            L = int(rng.integers(1000, 5001))
            h0 = rand_seq(rng, L)
            h1 = mutate(rng, h0, 0.02)
            q0 = mutate(rng, h0, 0.003)
            for a, h in enumerate((h0, h1)):
                trecs.append((s + a, "%s_h%d_%d" % (chrom, a, r), h, aux("RG", "Z", "truth") + ta + aux("sp", "A", "b")))
            for a, q in enumerate((q0, h1)):
                qrecs.append((s + a, "%s:%d-%d_%d" % (chrom, s, e, a), q, aux("RG", "Z", "asm") + ta))
            for t in (h0, h1):
                for q in (q0, h1):
                    if t != q:
                        pairs.append(oriented(t, q))
            f.write("%s\t%d\t%d\n" % (chrom, s, e))
    write_allele_bam(os.path.join(d, "truth.bam"), chrom, step * n + 2000, ["truth"], trecs)
    write_allele_bam(os.path.join(d, "query.bam"), chrom, step * n + 2000, ["asm"], qrecs)
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=10000)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    d = a.workdir or tempfile.mkdtemp(prefix="bench_compare_")
    t0 = time.time()
    pairs = make_job(d, a.regions)
    t_make = time.time() - t0
    bed, tb, qb = (os.path.join(d, x) for x in ("regions.bed", "truth.bam", "query.bam"))
    otter_amd.compare_files(tb, qb, bed, threads=a.threads)                       # warm-up (contexts, workspaces)
    walls = []
    for _ in range(a.repeat):
        t0 = time.time()
        text, warn, st = otter_amd.compare_files(tb, qb, bed, threads=a.threads)
        walls.append(time.time() - t0)
    wall = float(np.median(walls))
    out = {"regions": a.regions, "pairs_aligned": int(st["n_reads"]), "wall_s_median": round(wall, 3), "regions_per_s": round(a.regions / wall, 1),
           "ms_ingest": round(st["ms_ingest"], 1), "ms_hot_path": round(st["ms_hot_path"], 1), "ms_emit": round(st["ms_emit"], 1),
           "lines": text.count(b"\n"), "fixture_s": round(t_make, 1)}
    arena, offs, lens = abi.pack_seqs([s for p in pairs for s in p])
    tasks = abi.make_tasks([(int(offs[2 * i]), int(lens[2 * i]), int(offs[2 * i + 1]), int(lens[2 * i + 1]), None) for i in range(len(pairs))])
    with otter_amd.Context(0) as ctx:
        ctx.edit_align_batch(arena, tasks, want_cigars=False)
        sm, pm = [], []
        for _ in range(a.repeat):
            ctx.edit_align_batch(arena, tasks, want_cigars=False)
            x, y = ctx.edit_align_last_ms()
            sm.append(x); pm.append(y)
        ctx.edit_align_batch(arena, tasks, want_cigars=True)
        _, pm_cig = ctx.edit_align_last_ms()
    out.update({"kernel_ms_score_pass": round(float(np.median(sm)), 2), "kernel_ms_provenance_pass": round(float(np.median(pm)), 2),
                "kernel_ms_provenance_pass_with_op_strings": round(pm_cig, 2), "pairs_kernel": len(pairs)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

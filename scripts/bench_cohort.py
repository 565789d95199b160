#!/usr/bin/env python3
"""One pass against the round trip: scripts/bench_cohort.py S R D [--len LO HI] [--repeats N] [--threads T] [--out FILE]
builds a cohort fixture (S samples x R regions x D reads per region) and times, in one process,
  (a) otter_amd.cohort_files                       sample BAMs -> joint VCF, alleles staying on the device
  (b) the S otter_amd.assemble_files calls         sample BAMs -> per-sample allele SAM text
  (c) otter_amd.genotype_files on the merged BAM   allele BAM -> VCF
The merged allele BAM of (c) is written OUTSIDE the timed region: the round trip's sort / compress / index step is a gift to the baseline.
One untimed warm-up of each leg first (contexts and workspaces are kept by the dispatcher), then `repeats` timed rounds a, b, c in turn;
wall clock of the calls and the stage busy times the library reports.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import otter_amd  # noqa: E402
from otter_amd import bamwrite  # noqa: E402
import cohort_helpers as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("S", type=int); ap.add_argument("R", type=int); ap.add_argument("D", type=int)
ap.add_argument("--len", type=int, nargs=2, default=(1000, 5000))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out", default=None)
a = ap.parse_args()

tmp = tempfile.mkdtemp()
t0 = time.time()
fx = bamwrite.make_cohort_fixture(tmp, a.R, a.S, depth=a.D, len_range=tuple(a.len), seed=41)
t_fix = time.time() - t0


def leg_a():
    t = time.perf_counter()
    text, st = otter_amd.cohort_files(fx["bams"], fx["names"], fx["bed"], fx["fasta"], threads=a.threads)
    return (time.perf_counter() - t) * 1e3, st, text


def leg_b():
    t = time.perf_counter()
    out = [otter_amd.assemble_files(b, fx["bed"], fasta=fx["fasta"], read_group=n, threads=a.threads) for b, n in zip(fx["bams"], fx["names"])]
    ms = (time.perf_counter() - t) * 1e3
    st = {k: sum(o[1][k] for o in out) for k in ("ms_ingest", "ms_hot_path", "ms_emit", "n_reads", "n_alleles")}
    return ms, st, [o[0] for o in out]


merged = os.path.join(tmp, "merged.bam")


def leg_c():
    t = time.perf_counter()
    text, st = otter_amd.genotype_files(merged, fx["bed"], fasta=fx["fasta"], threads=a.threads)
    return (time.perf_counter() - t) * 1e3, st, text


_, _, vcf_a = leg_a()
_, _, sams = leg_b()
H.sam_to_bam_python(H.merge_sams(sams), merged)
_, _, vcf_c = leg_c()
same = vcf_a == vcf_c
rounds = {"a": [], "b": [], "c": []}
for _ in range(a.repeats):
    for k, f in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
        ms, st, _x = f()
        rounds[k].append({"wall_ms": ms, "ms_ingest": st["ms_ingest"], "ms_hot_path": st["ms_hot_path"], "ms_emit": st["ms_emit"]})


def summary(rs):
    w = [r["wall_ms"] for r in rs]
    return {"wall_ms_median": statistics.median(w), "wall_ms_min": min(w), "wall_ms_max": max(w), "rounds": rs}


commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
bc = [rb["wall_ms"] + rc["wall_ms"] for rb, rc in zip(rounds["b"], rounds["c"])]
res = {"bench": "cohort", "command": " ".join(sys.argv), "commit": commit, "samples": a.S, "regions": a.R, "depth": a.D, "len_range": list(a.len),
       "threads": a.threads, "repeats": a.repeats, "fixture_s": t_fix, "vcf_bytes": len(vcf_a), "one_pass_equals_round_trip": same,
       "a_cohort_files": summary(rounds["a"]), "b_assemble_files_x_S": summary(rounds["b"]), "c_genotype_files": summary(rounds["c"]),
       "b_plus_c_wall_ms_median": statistics.median(bc), "b_plus_c_wall_ms_min": min(bc), "b_plus_c_wall_ms_max": max(bc)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")

#!/usr/bin/env python3
"""What the fused cohort matrix saves: scripts/bench_cohort_matrix.py MODE FIXTURE_DIR [-k K] [--regions R] [--samples S] [--depth D]
[--repeats N] [--threads T] [--root DIR] [--out FILE]
  MODE fused     wall time of cohort_files(matrix_k=K): sample BAMs -> joint VCF and the k-mer usage matrix, the rows staying in HBM
  MODE two_step  wall time of cohort_files, the VCF written to a file, vcf2mat_files on that file (runs on a build without matrix_k too:
                 --root names the tree whose otter_amd is imported, default the tree of this script)
FIXTURE_DIR holds the cohort of bamwrite.make_cohort_fixture (built on first use, reused after: both modes time the same files).  One untimed
warm-up, then `repeats` timed rounds; prints one JSON line with the median and the spread (and writes it to --out)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["fused", "two_step"]); ap.add_argument("fixture")
ap.add_argument("-k", type=int, default=3)
ap.add_argument("--regions", type=int, default=10000); ap.add_argument("--samples", type=int, default=3); ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--len", type=int, nargs=2, default=(200, 600))
ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import otter_amd  # noqa: E402
from otter_amd import bamwrite  # noqa: E402

meta = os.path.join(a.fixture, "fixture.json")
if os.path.exists(meta):
    fx = json.load(open(meta))
else:
    os.makedirs(a.fixture, exist_ok=True)
    t0 = time.time()
    fx = bamwrite.make_cohort_fixture(a.fixture, a.regions, a.samples, depth=a.depth, len_range=tuple(a.len), seed=41)
    fx = {k: fx[k] for k in ("bams", "names", "bed", "fasta")}
    fx["fixture_s"] = time.time() - t0
    json.dump(fx, open(meta, "w"))
args = (fx["bams"], fx["names"], fx["bed"], fx["fasta"])
vcf_path = os.path.join(a.fixture, "joint_%s.vcf" % a.mode)


def fused():
    t = time.perf_counter()
    vcf, st, mat = otter_amd.cohort_files(*args, threads=a.threads, matrix_k=a.k)
    return {"wall_ms": (time.perf_counter() - t) * 1e3, "ms_hot_path": st["ms_hot_path"], "ms_emit": st["ms_emit"], "ms_ingest": st["ms_ingest"]}, vcf, mat


def two_step():
    t = time.perf_counter()
    vcf, st = otter_amd.cohort_files(*args, threads=a.threads)
    t1 = time.perf_counter()
    with open(vcf_path, "wb") as f:
        f.write(vcf)
    t2 = time.perf_counter()
    mat, st2 = otter_amd.vcf2mat_files(vcf_path, fx["bed"], k=a.k, threads=a.threads)
    t3 = time.perf_counter()
    return {"wall_ms": (t3 - t) * 1e3, "cohort_ms": (t1 - t) * 1e3, "write_ms": (t2 - t1) * 1e3, "vcf2mat_ms": (t3 - t2) * 1e3,
            "vcf2mat_ms_ingest": st2["ms_ingest"], "vcf2mat_ms_hot_path": st2["ms_hot_path"], "vcf2mat_ms_emit": st2["ms_emit"]}, vcf, mat


leg = fused if a.mode == "fused" else two_step
_, vcf, mat = leg()
rounds = [leg()[0] for _ in range(a.repeats)]
w = [r["wall_ms"] for r in rounds]
res = {"bench": "cohort_matrix", "mode": a.mode, "command": " ".join(sys.argv), "k": a.k, "regions": a.regions, "samples": a.samples, "depth": a.depth,
       "len_range": list(a.len), "threads": a.threads, "repeats": a.repeats, "vcf_bytes": len(vcf), "matrix_bytes": len(mat), "matrix_rows": mat.count(b"\n"),
       "vcf_sha1": hashlib.sha1(vcf).hexdigest(), "matrix_sha1": hashlib.sha1(mat).hexdigest(),
       "wall_ms_median": statistics.median(w), "wall_ms_min": min(w), "wall_ms_max": max(w), "rounds": rounds}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")

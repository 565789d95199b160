"""Measures `otter vcf2mat` (otg_vcf2mat_files and otg_kmer_usage_batch) on a synthetic VCF: --records records (default 50 000), each with a
REF and 1-5 ALT alleles of 1-10 kb, at k = 3 and k = 6.  Prints one JSON line per k: records/s and output MB/s of the file-to-text path
(text discarded), its stage busy times (read, device, emit), the kernel time of one device batch and the allele GB/s it reaches, and a
single-thread CPU baseline (tests/vcf2mat_ref.cpp, the tests' C++ restatement) run on the first --cpu-records records.
    python scripts/bench_vcf2mat.py [--records N] [--threads T] [--cpu-records M] [--ks 3,6]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402


def make_vcf(path, n, seed=1, len_range=(1000, 10000)):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    nal = 0
    with open(path, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n")
        for i in range(n):
            m = 1 + int(rng.integers(1, 6))
            lens = rng.integers(len_range[0], len_range[1] + 1, m)
            seq = acgt[rng.integers(0, 4, int(lens.sum()))].tobytes()
            al, p = [], 0
            for ln in lens:
                al.append(seq[p:p + int(ln)]); p += int(ln)
            f.write(b"chr1\t%d\tchr1:%d-%d\t%s\t%s\t.\tPASS\t.\tGT\t0/1\n" % (100 * i, 100 * i, 100 * i + 50, al[0], b",".join(al[1:])))
            nal += m
    return nal


def files_run(vcf, bed, k, threads):
    L = otter_amd.load()
    job = abi.Vcf2matJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode(); job.k = k; job.threads = threads; job.device = 0; job.batch_alleles = 0
    out = [0]

    def sink(_user, data, n):               # the text is counted, not kept
        out[0] += n
        return 0
    cb = abi.WRITE_FN(sink)
    st = abi.JobStats()
    L.otg_vcf2mat_files.argtypes = [C.POINTER(abi.Vcf2matJob), abi.WRITE_FN, C.c_void_p, C.POINTER(abi.JobStats)]
    t0 = time.perf_counter()
    rc = L.otg_vcf2mat_files(C.byref(job), cb, None, C.byref(st))
    wall = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError("otg_vcf2mat_files failed (%d): %s" % (rc, (L.otg_last_error(None) or b"").decode()))
    return wall, {f: getattr(st, f) for f, _ in abi.JobStats._fields_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-records", type=int, default=2000)
    ap.add_argument("--ks", default="3,6")
    a = ap.parse_args()
    import vcf2mat_fixtures as F
    with tempfile.TemporaryDirectory() as tmp:
        vcf, bed = os.path.join(tmp, "bench.vcf"), os.path.join(tmp, "bench.bed")
        open(bed, "w").write("chr1\t0\t100\n")
        t0 = time.perf_counter()
        n_alleles = make_vcf(vcf, a.records)
        gen_s = time.perf_counter() - t0
        cpu_vcf = os.path.join(tmp, "cpu.vcf")
        make_vcf(cpu_vcf, a.cpu_records)
        exe = F.build_driver(tmp)
        # one device batch of the alleles of 4 096 further records (about 16 000 alleles) for the kernel time
        kern_vcf = os.path.join(tmp, "kernel.vcf")
        make_vcf(kern_vcf, 4096, seed=2)
        r = otter_amd.vcf_read_alleles(kern_vcf)
        nb = len(r["seq_len"])
        end = int(r["seq_off"][nb - 1]) + int(r["seq_len"][nb - 1])
        arena = np.ascontiguousarray(r["arena"][:end])
        with otter_amd.Context(0) as ctx:
            for k in [int(x) for x in a.ks.split(",")]:
                ctx.kmer_usage_batch(arena, r["seq_off"][:nb], r["seq_len"][:nb], k=k)       # warm-up
                ctx.kmer_usage_batch(arena, r["seq_off"][:nb], r["seq_len"][:nb], k=k)
                c_ms, e_ms = ctx.kmer_usage_last_ms()
                files_run(vcf, bed, k, a.threads)                                             # warm-up (file cache, device pool)
                wall, st = files_run(vcf, bed, k, a.threads)
                t0 = time.perf_counter()
                cpu_bytes = len(subprocess.run([exe, "text", str(k), cpu_vcf], capture_output=True, check=True).stdout)
                cpu_s = time.perf_counter() - t0
                print(json.dumps({
                    "k": k, "records": a.records, "alleles": n_alleles, "vcf_MB": round(os.path.getsize(vcf) / 1e6, 1), "threads": a.threads,
                    "wall_s": round(wall, 3), "records_per_s": round(a.records / wall, 1), "out_MB_per_s": round(st["output_bytes"] / 1e6 / wall, 1),
                    "out_MB": round(st["output_bytes"] / 1e6, 1), "ms_read": round(st["ms_ingest"], 1), "ms_device": round(st["ms_hot_path"], 1),
                    "ms_emit": round(st["ms_emit"], 1), "kernel_batch_alleles": nb, "kernel_ms": round(c_ms + e_ms, 3),
                    "kernel_allele_GB_per_s": round(end / 1e9 / ((c_ms + e_ms) / 1e3), 1),
                    "cpu_baseline_records": a.cpu_records, "cpu_baseline_s": round(cpu_s, 3),
                    "cpu_baseline_records_per_s": round(a.cpu_records / cpu_s, 1), "cpu_baseline_out_MB": round(cpu_bytes / 1e6, 1),
                    "speedup_vs_cpu": round((a.records / wall) / (a.cpu_records / cpu_s), 1), "gen_s": round(gen_s, 1)}), flush=True)


if __name__ == "__main__":
    main()

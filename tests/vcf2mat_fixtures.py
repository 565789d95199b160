"""Shared pieces of the `otter vcf2mat` tests: the C++ restatement (tests/vcf2mat_ref.cpp) built with g++, either plain or against the
reference's own seq2kcounts / KmerEncoding / KUSAGE::hsdiv (oracle/_ref/libotter_ref_io.so), a numpy restatement of the per-allele values,
and the synthetic VCF of the golden fixtures."""
import gzip
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "vcf2mat_ref.cpp")
REF_IO_SO = os.path.join(ROOT, "oracle", "_ref", "libotter_ref_io.so")
REF_DIR = os.environ.get("OTTER_REFERENCE", "/root/reference")      # where oracle/Makefile finds the reference (REF)
GOLDEN = os.path.join(ROOT, "tests", "golden")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def build_driver(tmp, with_ref=False):
    """the restatement; with_ref=True links the reference's own functions (needs its headers and oracle/_ref; None when absent)"""
    exe = os.path.join(str(tmp), "vcf2mat_ref" + ("_anseqs" if with_ref else ""))
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, DRIVER_SRC, "-lz"]
    if with_ref:
        if not (os.path.exists(REF_IO_SO) and os.path.isdir(os.path.join(REF_DIR, "src"))):
            return None
        cmd[-2:-2] = ["-DOTG_REF_ANSEQS", "-w", "-I" + os.path.join(REF_DIR, "src")]
        cmd += [REF_IO_SO, "-Wl,-rpath," + os.path.dirname(REF_IO_SO)]
    subprocess.check_call(cmd)
    return exe


def driver_text(exe, k, vcf):
    return subprocess.run([exe, "text", str(k), vcf], capture_output=True, check=True, timeout=600).stdout


def driver_values(exe, k, vcf, tmp):
    """-> (gc, hsd, usage [n, 4^k+1]) from the driver"""
    out = os.path.join(str(tmp), "values_k%d.bin" % k)
    subprocess.run([exe, "values", str(k), vcf, out], check=True, timeout=600)
    v = np.fromfile(out, dtype=np.float64).reshape(-1, 4 ** k + 3)
    return v[:, 0].copy(), v[:, 1].copy(), np.ascontiguousarray(v[:, 2:])


_CODE = np.full(256, 4, dtype=np.int64)
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_c] = _v


def kmer_values(seq, k):
    """numpy restatement of seq2kcounts + KUSAGE + hsdiv + get_gc_content -> (counts, usage, gc, hsd)"""
    s = np.frombuffer(seq, dtype=np.uint8)
    L, nb = len(s), 4 ** k
    counts = np.zeros(nb + 1, dtype=np.int64)
    if L >= k:
        code = _CODE[s]
        nw = L - k + 1
        idx = np.zeros(nw, dtype=np.int64)
        bad = np.zeros(nw, dtype=bool)
        for h in range(k):
            c = code[h:h + nw]
            idx = idx * 4 + (c & 3)
            bad |= c == 4
        idx[bad] = nb
        counts = np.bincount(idx, minlength=nb + 1)
    total = int(counts.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        usage = counts.astype(np.float64) / np.float64(total)
        gc = np.float64(int(np.isin(s, np.frombuffer(b"CGcg", dtype=np.uint8)).sum())) / np.float64(L)
    acc = 0.0
    for v in usage[counts > 0]:
        acc += v * math.log(v)
    acc = -1 * acc
    return counts, usage, gc, math.pow(math.e, acc)


def golden_lines(rng):
    """the synthetic VCF lines of tests/golden/vcf2mat_small.vcf.gz: every case of the vcf2mat contract"""
    def rs(n, alpha=b"ACGT"):
        a = np.frombuffer(alpha, dtype=np.uint8)
        return a[rng.integers(0, len(a), n)].tobytes()
    lines = [b"##fileformat=VCFv4.2", b"##source=vcf2mat_small", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
    row = lambda i, ref, alt, tail=b"\t.\tPASS\t.\tGT\t0/1": b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + ref + b"\t" + alt + tail
    i = 1
    for _ in range(6):                                             # ordinary records, REF + 1-4 ALT
        alts = b",".join(rs(int(rng.integers(20, 400))) for _ in range(int(rng.integers(1, 5))))
        lines.append(row(i, rs(int(rng.integers(20, 400))), alts)); i += 1
    lines += [row(i, rs(80), b"."), row(i + 1, rs(60), b"<DEL>"), row(i + 2, rs(70), b"A,<DEL>"), row(i + 3, rs(50), b"A,,C"),
              row(i + 4, rs(40), b"ACGTACGT,"), row(i + 5, rs(90).lower(), rs(33).lower() + b"," + rs(20)),
              row(i + 6, rs(120, b"ACGTN"), b"NNNNNNNN," + rs(64, b"ACGTNRY")), row(i + 7, b"AC", b"ACGTA,ACGTAC,G"),
              row(i + 8, b"", b"ACGT"), b"", row(i + 9, rs(30), b"", b""), b"chr1\t%d\tchr1:short" % (100 * (i + 10)),
              b"chr1\t%d\tfour_columns\t" % (100 * (i + 11)) + rs(45), b"# a comment in the body", row(i + 12, b"acgtNNacgt", b"AcGt"),
              row(i + 13, rs(200), rs(150) + b"," + rs(150))]
    return lines


def write_golden_vcf(path, lines):
    data = b"\n".join(lines)                                       # the last line has no '\n'
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)
    return data

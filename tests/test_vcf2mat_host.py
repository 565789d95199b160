"""`otter vcf2mat` host layers (no device): the VCF reader and parse_alleles (otg_vcf_read_alleles, src/vcf2mat.cpp:16-36,57-65 and
src/angzipiter.hpp), the row text (otg_vcf2mat_emit, :66-72) against hand-derived rows and against the C++ restatement built on the
reference's own seq2kcounts / KUSAGE (tests/vcf2mat_ref.cpp), the ABI structs and the CLI's argument errors."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import otter_amd
from otter_amd import abi, bamwrite
import vcf2mat_fixtures as F

ROOT = F.ROOT
CLI = os.path.join(ROOT, "tools", "otter_vcf2mat")


def _write(path, data, how):
    if how == "plain":
        open(path, "wb").write(data)
    elif how == "gzip":
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(data)
    else:
        w = bamwrite._Bgzf(path)
        w.write(data)
        w.close()
    return path


def _alleles(r):
    """{region bytes: [allele bytes]} in file order from vcf_read_alleles"""
    out = []
    for rec in r["records"]:
        reg = r["regions"][int(rec["region_off"]):int(rec["region_off"]) + int(rec["region_len"])]
        al = []
        for a in range(int(rec["first_allele"]), int(rec["first_allele"]) + int(rec["n_alleles"])):
            o, n = int(r["seq_off"][a]), int(r["seq_len"][a])
            al.append(r["arena"][o:o + n].tobytes())
        out.append((reg, al))
    return out


def _emit_from_numpy(path, k):
    r = otter_amd.vcf_read_alleles(path)
    n = len(r["seq_len"])
    usage = np.zeros((n, 4 ** k + 1)); gc = np.zeros(n); hsd = np.zeros(n)
    for a in range(n):
        o, ln = int(r["seq_off"][a]), int(r["seq_len"][a])
        _, usage[a], gc[a], hsd[a] = F.kmer_values(r["arena"][o:o + ln].tobytes(), k)
    return otter_amd.vcf2mat_emit(r["records"], r["regions"], r["seq_len"], k, usage, gc, hsd)


def test_abi_structs(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu %d\\n", sizeof(otg_vcf2mat_job), '
                   'offsetof(otg_vcf2mat_job, batch_alleles), sizeof(otg_vcf_record), offsetof(otg_vcf_record, n_alleles), OTG_KMER_MAX);return 0;}\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(abi.Vcf2matJob), abi.Vcf2matJob.batch_alleles.offset, abi.vcf_record_dt.itemsize,
                   abi.vcf_record_dt.fields["n_alleles"][1], abi.KMER_MAX]


@pytest.mark.parametrize("how", ["plain", "gzip", "bgzf"])
def test_reader_compressions(tmp_path, how):
    rng = np.random.default_rng(5)
    lines = F.golden_lines(rng)
    data = b"\n".join(lines)
    r = otter_amd.vcf_read_alleles(_write(str(tmp_path / ("v." + how)), data, how))
    got = _alleles(r)
    # ordinary records and every special case of parse_alleles, in file order
    assert len(got) == 19 and r["bytes_in"] == len(data)
    regs = [g[0] for g in got]
    assert regs[-3:] == [b"four_columns", b"chr1:1900-1950", b"chr1:2000-2050"]
    assert got[6][1][1:] == [] and got[7][1][1:] == [b"N"] and got[8][1][1:] == [b"A", b"<DEL>"] and got[9][1][1:] == [b"A", b"", b"C"]
    assert got[10][1][1:] == [b"ACGTACGT"] and got[13][1] == [b"AC", b"ACGTA", b"ACGTAC", b"G"] and got[14][1] == [b"", b"ACGT"]
    assert [len(a) for a in got[15][1]] == [30] and [len(a) for a in got[16][1]] == [45]     # REF with an empty last column; 4 columns
    assert got[-1][1][1:] and len(got[-1][1]) == 3          # the last line, without '\n', is read


def test_reader_long_lines_and_batches(tmp_path):
    rng = np.random.default_rng(9)
    big = F.ACGT[rng.integers(0, 4, 1_500_000)].tobytes()
    lines = [b"#h", b"c\t1\tr1\tACGT\tA,C", b"c\t2\tr2\t" + big + b"\t" + big[:700_000] + b",GG", b"c\t3\tr3\tTT\t.", b"c\t4\tr4\tA\tC"]
    data = b"\n".join(lines)
    p = _write(str(tmp_path / "long.vcf"), data, "plain")
    r = otter_amd.vcf_read_alleles(p)
    got = _alleles(r)
    assert [g[0] for g in got] == [b"r1", b"r2", b"r3", b"r4"]
    assert got[1][1] == [big, big[:700_000], b"GG"] and got[3][1] == [b"A", b"C"]
    # small buffers: the same records over several batches; a record larger than the buffers is reported, then returned
    r2 = otter_amd.vcf_read_alleles(p, max_alleles=2, max_bytes=1024)
    assert _alleles(r2) == got and r2["batches"] == 3


def test_reader_capacity_protocol(tmp_path):
    L = otter_amd.load()
    p = _write(str(tmp_path / "c.vcf"), b"c\t1\tr1\tACGTACGT\tA,C,G\n", "plain")
    L.otg_vcf_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.otg_vcf_close.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert L.otg_vcf_open(p.encode(), C.byref(h)) == 0
    rec = np.zeros(4, dtype=abi.vcf_record_dt); reg = np.zeros(64, np.uint8); off = np.zeros(8, np.uint64); ln = np.zeros(8, np.uint32)
    ar = np.zeros(64, np.uint8)
    nr, ru, na, au = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    call = lambda cap_a, cap_s: L.otg_vcf_read_alleles(h, abi.ptr(rec), C.c_uint32(4), C.byref(nr), abi.ptr(reg), C.c_uint64(64), C.byref(ru),
                                                        abi.ptr(off), abi.ptr(ln), C.c_uint32(cap_a), C.byref(na), abi.ptr(ar), C.c_uint64(cap_s),
                                                        C.byref(au), None)
    assert call(2, 64) == abi.OTG_ERR_CAPACITY and (nr.value, na.value, au.value, ru.value) == (0, 4, 11, 2)
    assert call(8, 64) == 0 and (nr.value, na.value, au.value) == (1, 4, 11)
    assert list(ln[:4]) == [8, 1, 1, 1] and ar[:11].tobytes() == b"ACGTACGTACG"
    assert call(8, 64) == 0 and nr.value == 0
    L.otg_vcf_close(h)


# hand-derived rows (k = 1: bins A C G T and the non-ACGT bin)
HAND = [
    (b"##x\n#CHROM\n\nc\t1\tr\tACGT\t.\n", 1, b"r\t0\t0.5\t4\t4\t0.25\t0.25\t0.25\t0.25\t0\n"),
    (b"c\t1\tr\tAACG\t<DEL>\n", 1, b"r\t0\t0.5\t4\t2.82843\t0.5\t0.25\t0.25\t0\t0\nr\t1\t0\t1\t1\t0\t0\t0\t0\t1\n"),
    (b"c\t1\tr\tacgt\tA,<DEL>\n", 1, b"r\t0\t0.5\t4\t4\t0.25\t0.25\t0.25\t0.25\t0\nr\t1\t0\t1\t1\t1\t0\t0\t0\t0\nr\t2\t0\t5\t1\t0\t0\t0\t0\t1\n"),
    (b"c\t1\tr\tGG\tA,,C", 1, b"r\t0\t1\t2\t1\t0\t0\t1\t0\t0\nr\t1\t0\t1\t1\t1\t0\t0\t0\t0\n"
                            b"r\t2\t-nan\t0\t1\t-nan\t-nan\t-nan\t-nan\t-nan\nr\t3\t1\t1\t1\t0\t1\t0\t0\t0\n"),
    (b"c\t1\tr\tNN\tN\n", 1, b"r\t0\t0\t2\t1\t0\t0\t0\t0\t1\nr\t1\t0\t1\t1\t0\t0\t0\t0\t1\n"),
    (b"c\t1\tr\t\tG\n", 1, b"r\t0\t-nan\t0\t1\t-nan\t-nan\t-nan\t-nan\t-nan\nr\t1\t1\t1\t1\t0\t0\t1\t0\t0\n"),
    (b"c\t1\tr\tC\t.\n", 2, b"r\t0\t1\t1\t1" + b"\t-nan" * 17 + b"\n"),                        # L < k
    (b"c\t1\tshort\n\nc\t1\tr\tTA\t,\n", 2, b"r\t0\t0\t2\t1" + b"\t0" * 12 + b"\t1" + b"\t0" * 4 + b"\nr\t1\t-nan\t0\t1" + b"\t-nan" * 17 + b"\n"),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_rows(tmp_path, case):
    data, k, want = HAND[case]
    p = _write(str(tmp_path / "h.vcf"), data, "plain")
    assert _emit_from_numpy(p, k) == want


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vcf2mat_ref")
    return {"plain": F.build_driver(tmp), "ref": F.build_driver(tmp, with_ref=True)}


def _random_vcf(path, rng, n):
    lines = [b"##fileformat=VCFv4.2"]
    alpha = np.frombuffer(b"ACGTACGTACGTacgtNRY.<", dtype=np.uint8)
    for i in range(n):
        al = [alpha[rng.integers(0, len(alpha), int(rng.integers(0, 300)))].tobytes().replace(b".", b"A") for _ in range(int(rng.integers(1, 5)))]
        alt = b",".join(al[1:]) if len(al) > 1 else b"."
        lines.append(b"c\t%d\tc:%d-%d\t%s\t%s\t.\tPASS\t." % (i, i, i + 10, al[0], alt))
    return _write(path, b"\n".join(lines) + b"\n", "gzip")


@pytest.mark.parametrize("which", ["plain", "ref"])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_emit_against_the_restatement(drivers, tmp_path, k, which):
    exe = drivers[which]
    if exe is None:
        pytest.skip("oracle/_ref/libotter_ref_io.so or the reference headers are not available")
    p = _random_vcf(str(tmp_path / "r.vcf.gz"), np.random.default_rng(100 + k), 12 if k == 8 else 60)
    gc, hsd, usage = F.driver_values(exe, k, p, tmp_path)
    r = otter_amd.vcf_read_alleles(p)
    assert len(gc) == len(r["seq_len"])
    assert otter_amd.vcf2mat_emit(r["records"], r["regions"], r["seq_len"], k, usage, gc, hsd) == F.driver_text(exe, k, p)
    # the numpy restatement gives the same counts, values and GC (the device tests compare against it)
    for a in range(len(gc)):
        o, ln = int(r["seq_off"][a]), int(r["seq_len"][a])
        _, u, g, h = F.kmer_values(r["arena"][o:o + ln].tobytes(), k)
        assert np.array_equal(u, usage[a], equal_nan=True) and np.array_equal(g, gc[a], equal_nan=True)
        assert abs(h - hsd[a]) <= 1e-12 * hsd[a]


def test_golden_text_is_the_restatement(drivers, tmp_path):
    """the committed golden rows (reference functions) are what the plain restatement prints, and the emit gives them from its values"""
    vcf = os.path.join(F.GOLDEN, "vcf2mat_small.vcf.gz")
    for k in (3, 6):
        want = gzip.open(os.path.join(F.GOLDEN, "vcf2mat_small_k%d.txt.gz" % k)).read()
        assert F.driver_text(drivers["plain"], k, vcf) == want
        gc, hsd, usage = F.driver_values(drivers["plain"], k, vcf, tmp_path)
        r = otter_amd.vcf_read_alleles(vcf)
        assert otter_amd.vcf2mat_emit(r["records"], r["regions"], r["seq_len"], k, usage, gc, hsd) == want


def _cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, timeout=60)


@pytest.mark.parametrize("k", ["0", "13", "-1", "32"])
def test_cli_kmer_size_errors(k):
    r = _cli("-b", "x.bed", "-k", k, "in.vcf")
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr == ("[ERROR] invalid '--kmer-size' (%s). Needs to be 1 <= x <= 12.\n" % k).encode()


def test_cli_other_arguments():
    r = _cli()
    assert r.returncode == 0 and b"Usage:" in r.stdout                     # no input: the help, as the reference
    r = _cli("in.vcf")
    assert r.returncode == 1 and b"Error parsing options" in r.stdout      # -b is required
    r = _cli("-b", "x.bed", "-k", "three", "in.vcf")
    assert r.returncode == 1 and b"Error parsing options" in r.stdout


def test_no_device_no_fallback(tmp_path):
    if otter_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    L = otter_amd.load()
    assert L.otg_kmer_usage_batch(None, None, C.c_uint64(0), None, None, C.c_uint32(1), C.c_int32(3), None, None, None) == abi.OTG_ERR_NO_DEVICE
    bed = tmp_path / "b.bed"
    bed.write_text("c\t1\t10\n")
    vcf = _write(str(tmp_path / "v.vcf"), b"c\t1\tr\tACGT\t.\n", "plain")
    with pytest.raises(otter_amd.OtterGpuError) as e:
        otter_amd.vcf2mat_files(vcf, str(bed), k=3)
    assert "(-1)" in str(e.value)
    r = _cli("-b", str(bed), vcf)
    assert r.returncode == 1 and r.stdout == b""

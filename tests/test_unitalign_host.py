"""CPU: the cyclic unit alignment without a device.

1. the eleven results the rule was prototyped with as literals, through both forms of tests/unitalign_ref.py (the rule restated from
   include/otter_gpu.h);
2. step 2 of the rule as an independent witness: the brute-force shortest-best-substring search == the DP on 400 seeded cases;
3. the properties that follow from the rule on the random set;
4. the kernel's arithmetic (otter_amd/csrc/otg_unitalign_core.hpp) run on the host in the kernel's schedule by
   tests/unitalign_core_host.cpp, a stand-alone program built with -fsanitize=address,undefined, == unitalign_ref: every segment class, both
   key widths, finished neighbours, and the narrow tier at its bound;
5. otg_parse_bed_units on a literal catalogue; 6. otg_unitalign_emit against rows formatted in Python; 7. the refusals that need no device
   and the tool's messages; 8. the ABI mirrors."""
import ctypes as C
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
import motif_cases as Cs
import unitalign_cases as Uc
import unitalign_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


# ---------------------------------------------------------------------------------------------- 1: the rule on literals
def test_reference_on_the_prototype_table():
    assert len(Uc.TABLE) == 11
    for s, u, want in Uc.TABLE:
        assert R.unitalign(s, u) == want + (0,), (s, u)
        assert R.unitalign_np(s, u) == want + (0,), (s, u)
    assert R.unitalign(b"CAG", b"") == (0, 0, 0, R.NO_UNIT) and R.unitalign_np(b"", b"") == (0, 0, 0, R.NO_UNIT)
    assert R.unitalign(b"CAG", b"A" * 257, chained=True) == (0, 0, 0, R.UNIT_TOO_LONG)
    with pytest.raises(ValueError):
        R.unitalign(b"CAG", b"A" * 257)
    assert R.refusal(R.MAX_LEN + 1, 3) == R.TOO_LONG and R.refusal(R.MAX_LEN, 3) == 0


# ---------------------------------------------------------------------------------------------- 2: the witness
def test_brute_force_witness_of_step_2():
    cases = Uc.tiny_set()
    assert len(cases) >= 300 and all(len(u) <= 7 and len(s) <= 14 for s, u in cases)
    assert sum(b"N" in s or b"N" in u for s, u in cases) > 100
    for s, u in cases:
        r = R.unitalign(s, u)
        assert r[:2] == R.unitalign_brute(s, u), (s, u)
        assert r == R.unitalign_np(s, u), (s, u)


# ---------------------------------------------------------------------------------------------- 3: the properties
def test_properties_of_the_rule():
    n_edits = 0
    for s, u in Uc.random_set():
        e, ub, ph, f = R.unitalign(s, u)
        assert f == 0 and e <= len(s) and ub <= len(s) + e and ph < len(u)
        assert (e, ub, ph, f) == R.unitalign_np(s, u)
        for k in (1, len(u) // 2):                                        # a rotated unit changes only the end phase
            rot = u[k % len(u):] + u[:k % len(u)]
            e2, ub2, ph2, _ = R.unitalign(s, rot)
            assert (e2, ub2) == (e, ub)
        assert R.unitalign(s.lower(), u) == (e, ub, ph, f) and R.unitalign(s, u.lower()) == (e, ub, ph, f)
        n_edits += e > 0
    assert n_edits > 200


# ---------------------------------------------------------------------------------------------- 4: the kernel's arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("unitalign_core") / "unitalign_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "unitalign_core_host.cpp")])
    return exe


def _run(exe, pairs, wide=0, seg64=0):
    """one batch -> per task ((edits, unit_bases, end_phase, flags), (tier, class))"""
    text = "batch %d %d %d\n" % (len(pairs), wide, seg64) + "".join("%s %s\n" % (s.hex() or "-", u.hex() or "-") for s, u in pairs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    rows = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]
    assert len(rows) == len(pairs)
    return [(t[:4], t[4:]) for t in rows]


@pytest.fixture(scope="module")
def small_sets():
    pairs = Uc.edge_set() + Uc.random_set() + Uc.tiny_set(n=60)
    for p in (3, 7, 13, 29):                                               # sixteen unequal neighbours in one wave, classes 4 .. 32
        pairs += Uc.one_wave_batch(p)
    return pairs, [R.unitalign_np(s, u) for s, u in pairs]


@pytest.mark.parametrize("wide,seg64", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_core_arithmetic_against_the_rule(harness, small_sets, wide, seg64):
    pairs, want = small_sets
    got = _run(harness, pairs, wide, seg64)
    for (s, u), (g, _), w in zip(pairs, got, want):
        assert g == w, (s[:60], u[:60])
    ran = {tc for (g, tc), (s, u) in zip(got, pairs) if len(s) and len(u)}
    assert ran == {(wide, c) for c in ((4, 5, 6) if seg64 else range(7))}     # every segment class ran, on the tier asked for


def test_short_sets_agree_with_the_plain_reference(small_sets):
    pairs, want = small_sets
    n = 0
    for (s, u), w in zip(pairs, want):
        if len(u) <= 9 and len(s) <= 220:
            assert R.unitalign(s, u) == w, (s, u)
            n += 1
    assert n > 300


def test_narrow_tier_at_its_bound(harness):
    L, p = abi.UNITALIGN_NARROW_LEN, abi.UNITALIGN_MAX_UNIT
    rng = np.random.default_rng(41)
    unit = Cs.rs(rng, p)
    holed = (unit + unit[:100] + unit[101:]) * (L // (2 * p - 1) + 1)        # a deletion in every second copy
    pairs = [(b"N" * L, unit), (Uc.repeat_from(unit, 17, L), unit), (holed[:L], unit)]
    narrow, wide = _run(harness, pairs, 0), _run(harness, pairs, 1)
    assert [tc for _, tc in narrow] == [(0, 6)] * 3 and [tc for _, tc in wide] == [(1, 6)] * 3
    assert [g for g, _ in narrow] == [g for g, _ in wide]
    assert narrow[0][0] == (L, 0, 0, 0)                                     # edits = L
    assert narrow[1][0] == (0, L, (17 + L) % p, 0)                          # unit_bases = L
    e, ub = narrow[2][0][:2]
    assert narrow[2][0] == R.unitalign_np(*pairs[2]) and e >= L // (2 * p) - 1 and ub == L + e      # every edit is a skipped unit base
    # one base more leaves the narrow tier
    assert _run(harness, [(b"A" * (L + 1), b"A")], 0)[0][1] == (1, 0)


# ---------------------------------------------------------------------------------------------- 5: the catalogue reader
CATALOGUE = ("#chrom\tstart\tend\tunits\n"
             "chr1\t100\t160\tCAG\n"
             "chr1\t200\t260\tCAG,CCG\n"
             "\n"
             "chr4\t3074876\t3074933\tID=HTT;MOTIFS=CAG,CCG;STRUC=x\n"
             "chr2\t10\t20\tMOTIFS=cag\n"
             "chr2\t30\t40\tHTT_exon1\n"
             "chr2\t50\t60\tACGTX\n"
             "chr2\t70\t80\t" + "A" * 257 + "\n"
             "chr3\t5\t9\n"
             "#a comment\n"
             "chr3\t1\n"
             "chr3:11-19\n"
             "chr5\t1\t2\tCAG,CAG,\n"
             "chr5\t3\t4\tNAME;MOTIFS=AAG;X=1\textra\n"
             "chr5\t5\t6\t" + "A" * 256 + ",n")


def test_parse_bed_units_on_a_literal_catalogue(tmp_path):
    path = str(tmp_path / "cat.bed")
    open(path, "w").write(CATALOGUE)
    units = otter_amd.parse_bed_units(path)
    beds, arena, skipped = otter_amd.parse_bed_file(path)
    assert len(units) == len(beds) == 12 and skipped == 2                  # the empty line and the two-column line
    regions = otter_amd.bed_tuples(beds, arena)
    assert regions[0] == ("chr1", 100, 160) and regions[8] == ("chr3", 11, 19)
    assert units == [[b"CAG"], [b"CAG", b"CCG"], [b"CAG", b"CCG"], [b"cag"], [], [], [], [], [], [], [b"AAG"], [b"A" * 256, b"n"]]
    # the size protocol: the needs without buffers, then exact buffers
    L = otter_amd.load()
    nr, nu, ab = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    args = lambda first, cr, off, ln, cu, ar, ca: (C.c_char_p(path.encode()), abi.ptr(first), C.c_uint64(cr), C.byref(nr), abi.ptr(off), abi.ptr(ln), C.c_uint64(cu),
                                                   C.byref(nu), abi.ptr(ar), C.c_uint64(ca), C.byref(ab))
    assert L.otg_parse_bed_units(*args(None, 0, None, None, 0, None, 0)) == abi.OTG_ERR_CAPACITY
    assert (nr.value, nu.value, ab.value) == (12, 9, 3 + 6 + 6 + 3 + 3 + 257)
    first, off, ln, ar = np.zeros(13, dtype=np.uint64), np.zeros(9, dtype=np.uint64), np.zeros(9, dtype=np.uint32), np.zeros(ab.value, dtype=np.uint8)
    assert L.otg_parse_bed_units(*args(first, 12, off, ln, 9, ar, ab.value)) == abi.OTG_ERR_CAPACITY      # rec_first needs one entry more
    assert L.otg_parse_bed_units(*args(first, 13, off, ln, 9, ar, ab.value)) == 0
    assert list(first) == [0, 1, 3, 5, 6, 6, 6, 6, 6, 6, 6, 7, 9] and list(ln) == [3, 3, 3, 3, 3, 3, 3, 256, 1]
    with pytest.raises(otter_amd.OtterGpuError, match="cannot open"):
        otter_amd.parse_bed_units(str(tmp_path / "missing.bed"))
    bad = str(tmp_path / "bad.bed")
    open(bad, "w").write("chr1\tx\t5\tCAG\n")
    with pytest.raises(otter_amd.OtterGpuError, match="not a number"):
        otter_amd.parse_bed_units(bad)


# ---------------------------------------------------------------------------------------------- 6: the row text
def test_emit_against_python_rows():
    seqs = [b"CAG" * 10 + b"T" + b"CAG" * 10, b"cag" * 20, b"", b"ACGT", b"A" * 40, b"GATTACA"]
    regions = [b"chr1:100-160", b"", b"chrUn_x:5-9"]
    first, n_al = [0, 3, 4], [3, 1, 2]
    records = np.zeros(3, dtype=abi.vcf_record_dt)
    pos = 0
    for r in range(3):
        records[r] = (pos, len(regions[r]), first[r], n_al[r], 0)
        pos += len(regions[r])
    # allele -> [(source, unit, record)]: two catalogue units, a motif unit, no unit, an empty allele (zero denominator), flagged rows
    tasks = [[(0, b"CAG", R.unitalign(seqs[0], b"CAG")), (0, b"ccg", R.unitalign(seqs[0], b"ccg"))],
             [(1, b"AGC", R.unitalign(seqs[1], b"AGC"))],
             [(0, b"CAG", R.unitalign(seqs[2], b"CAG"))],
             [(1, b"", (0, 0, 0, R.NO_UNIT))],
             [(1, b"A" * 300, (0, 0, 0, R.UNIT_TOO_LONG)), (0, b"A", (0, 0, 0, R.TOO_LONG))],
             []]
    task_first = np.cumsum([0] + [len(t) for t in tasks]).astype(np.uint64)
    flat = [t for ts in tasks for t in ts]
    aligned = np.array([t[2] for t in flat], dtype=abi.unitalign_dt)
    text = otter_amd.unitalign_emit(records, b"".join(regions), [len(s) for s in seqs], task_first, [t[0] for t in flat], [t[1] for t in flat], aligned)
    want = b"".join(R.row(regions[r], i, len(seqs[first[r] + i]), (b"bed", b"motif")[src], unit, rec)
                    for r in range(3) for i in range(n_al[r]) for src, unit, rec in tasks[first[r] + i])
    assert text == want
    lines = want.split(b"\n")
    assert lines[0] == b"chr1:100-160\t0\t61\tbed\tCAG\t1\t60\t20.00\t0.9836" and lines[2] == b"chr1:100-160\t1\t60\tmotif\tAGC\t0\t60\t20.00\t1.0000"
    assert lines[3] == b"chr1:100-160\t2\t0\tbed\tCAG\t0\t0\t0.00\t0.0000" and lines[4] == b"\t0\t4\tmotif\t.\t0\t0\t0.00\t0.0000"
    assert lines[5].endswith(b"\t0\t0\t0.00\t0.0000") and lines[6] == b"chrUn_x:5-9\t0\t40\tbed\tA\t0\t0\t0.00\t0.0000" and len(lines) == 8
    assert otter_amd.unitalign_emit(records[:0], b"", [], [0], [], [], aligned[:0]) == b""
    # the buffer protocol: the length without a buffer, a buffer one byte short
    L = otter_amd.load()
    reg = np.frombuffer(b"".join(regions) + b"\0", dtype=np.uint8)
    ln = np.array([len(s) for s in seqs], dtype=np.uint32)
    src = np.array([t[0] for t in flat], dtype=np.uint8)
    ulen = np.array([len(t[1]) for t in flat], dtype=np.uint32)
    uoff = (np.cumsum(ulen) - ulen).astype(np.uint64)
    uar = np.frombuffer(b"".join(t[1] for t in flat), dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(3), abi.ptr(reg), abi.ptr(ln), abi.ptr(task_first), abi.ptr(src), abi.ptr(uar), abi.ptr(uoff),
                             abi.ptr(ulen), abi.ptr(aligned), out, C.c_uint64(cap), C.byref(need))
    assert L.otg_unitalign_emit(*args(None, 0)) == abi.OTG_ERR_CAPACITY and need.value == len(want)
    buf = C.create_string_buffer(len(want))
    assert L.otg_unitalign_emit(*args(buf, len(want) - 1)) == abi.OTG_ERR_CAPACITY
    assert L.otg_unitalign_emit(*args(buf, len(want))) == 0 and buf.raw == want
    task_first[2] = 1                                                      # fewer tasks behind than in front
    with pytest.raises(otter_amd.OtterGpuError, match="decreases"):
        otter_amd.unitalign_emit(records, b"".join(regions), ln, task_first, src, [t[1] for t in flat], aligned)


# ---------------------------------------------------------------------------------------------- 7: refusals without a device
def test_refusals_without_a_device(tmp_path):
    L = otter_amd.load()
    u, u64 = C.c_uint32, C.c_uint64
    one = np.zeros(1, dtype=np.uint32)
    assert L.otg_unitalign_batch(None, None, u64(0), None, None, u(0), None, u64(0), None, None, u(0), None, None, u(0), None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_unitalign_motifs(None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_unitalign_cohort(None, u(0), u(0), None, u64(0), None, None, u(0), None, None, u(0), None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_unitalign_device_results(None, abi.ptr(one), None) == abi.OTG_ERR_ARG
    assert L.otg_unitalign_last_ms(None, None) == abi.OTG_ERR_ARG
    assert L.otg_unitalign_emit(None, u(0), None, None, None, None, None, None, None, None, None, u64(0), None) == abi.OTG_ERR_ARG
    assert L.otg_parse_bed_units(None, None, u64(0), None, None, None, u64(0), None, None, u64(0), None) == abi.OTG_ERR_ARG
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\tCAG\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    for kw, msg in ((dict(max_period=0), "invalid '--max-period' (0). Needs to be 1 <= x <= 4096."),
                    (dict(max_period=4097), "invalid '--max-period' (4097). Needs to be 1 <= x <= 4096."),
                    (dict(slack=1000), "invalid '--slack' (1000). Needs to be 0 <= x <= 999.")):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.copies_files(vcf, bed, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and msg in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.copies_files(vcf, str(tmp_path / "missing.bed"))
    exe = os.path.join(ROOT, "tools", "otter_copies")
    for args, msg in ((["-p", "0"], b"invalid '--max-period' (0). Needs to be 1 <= x <= 4096."), (["-p", "4097"], b"invalid '--max-period' (4097)"),
                      (["--slack", "1000"], b"invalid '--slack' (1000). Needs to be 0 <= x <= 999."), (["--slack=-1"], b"invalid '--slack' (-1)"),
                      (["-p", "x"], None)):
        r = subprocess.run([exe, "-b", bed] + args + [vcf], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout.count(b"\t") == 0, (args, r)
        assert msg is None or msg in r.stderr
    assert subprocess.run([exe, vcf], capture_output=True, timeout=60).returncode == 1           # no BED
    assert subprocess.run([exe, "-b", str(tmp_path / "missing.bed"), vcf], capture_output=True, timeout=60).returncode == 1
    r = subprocess.run([exe], capture_output=True, timeout=60)                                   # the usage text
    assert r.returncode == 0 and b"Usage:" in r.stdout and b"--max-period" in r.stdout and b"--slack" in r.stdout and b"--batch" in r.stdout


# ---------------------------------------------------------------------------------------------- 8: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: v for k, v in re.findall(r"#define\s+(OTG_UNITALIGN_[A-Z_0-9]+)\s+(\S+)", txt)}
    assert set(defs) == {"OTG_UNITALIGN_MAX_UNIT", "OTG_UNITALIGN_MAX_LEN", "OTG_UNITALIGN_NARROW_LEN", "OTG_UNITALIGN_NO_UNIT", "OTG_UNITALIGN_TOO_LONG",
                         "OTG_UNITALIGN_UNIT_TOO_LONG", "OTG_UNITALIGN_SOURCE_BED", "OTG_UNITALIGN_SOURCE_MOTIF"}
    num = lambda k: int(defs[k].rstrip("u"))
    assert (num("OTG_UNITALIGN_MAX_UNIT"), num("OTG_UNITALIGN_MAX_LEN")) == (abi.UNITALIGN_MAX_UNIT, abi.UNITALIGN_MAX_LEN) == (R.MAX_UNIT, R.MAX_LEN) == (256, 1048575)
    assert (num("OTG_UNITALIGN_NO_UNIT"), num("OTG_UNITALIGN_TOO_LONG"), num("OTG_UNITALIGN_UNIT_TOO_LONG")) == (R.NO_UNIT, R.TOO_LONG, R.UNIT_TOO_LONG) \
        == (abi.UNITALIGN_NO_UNIT, abi.UNITALIGN_TOO_LONG, abi.UNITALIGN_UNIT_TOO_LONG)
    assert (num("OTG_UNITALIGN_SOURCE_BED"), num("OTG_UNITALIGN_SOURCE_MOTIF")) == (abi.UNITALIGN_SOURCE_BED, abi.UNITALIGN_SOURCE_MOTIF)
    # the narrow bound: the largest field a lane can hold, 2 (L - 1) + 2 p, stays under 2^16 - 1 at the bound and not one base above it
    N, P = abi.UNITALIGN_NARROW_LEN, abi.UNITALIGN_MAX_UNIT
    assert 2 * (N - 1) + 2 * P < 65535 <= 2 * N + 2 * P and N < 32767
    assert abi.UNITALIGN_MAX_LEN + 2 * P < 2 ** 31                           # the wide tier's fields have room to spare
    body = re.search(r"typedef struct otg_unitalign \{(.*?)\} otg_unitalign;", txt, flags=re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == list(abi.unitalign_dt.names)
    body = re.search(r"typedef struct otg_copies_job \{(.*?)\} otg_copies_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.CopiesJob._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu %d\\n",sizeof(otg_unitalign),'
                   'offsetof(otg_unitalign,flags),sizeof(otg_copies_job),offsetof(otg_copies_job,batch_alleles),OTG_UNITALIGN_NARROW_LEN);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.unitalign_dt.itemsize, abi.unitalign_dt.fields["flags"][1], C.sizeof(abi.CopiesJob), abi.CopiesJob.batch_alleles.offset, abi.UNITALIGN_NARROW_LEN]
    names = {"otg_unitalign_batch", "otg_unitalign_motifs", "otg_unitalign_cohort", "otg_unitalign_device_results", "otg_unitalign_last_ms",
             "otg_unitalign_emit"}
    assert names | {"otg_parse_bed_units", "otg_copies_files"} <= set(otter_amd.EXPORTS)
    assert {n for n in otter_amd.EXPORTS if n.startswith("otg_unitalign")} == names
    lib = otter_amd.load()
    for n in names | {"otg_parse_bed_units", "otg_copies_files"}:
        assert getattr(lib, n) is not None

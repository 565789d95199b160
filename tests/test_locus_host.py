"""CPU: the locus mode (the joint unit-set parse inside flanked alleles) without a device.

1. the seven results the rule was prototyped with as literals, through both forms of tests/locus_ref.py (the rule restated from
   include/otter_gpu.h), next to what the global joint parse and the single-unit tracts give for the first allele;
2. an independent witness of the score: the largest plain Smith-Waterman score against every word of the enumerated language == the DP on
   240 tiny cases at three score sets;
3. the properties that follow from the rule on a random set;
4. the kernel's arithmetic (otter_amd/csrc/otg_locus_core.hpp) run on the host in the kernel's schedule by tests/locus_core_host.cpp, a
   stand-alone program built with -fsanitize=address,undefined, == locus_ref: every class, both key widths, seg64 on and off, unequal
   neighbours in one wave, other scores, and the narrow tier at its derived bound;
5. otg_locus_emit against rows formatted in Python; 6. the refusals that need no device and the tool's messages; 7. the ABI mirrors."""
import ctypes as C
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
import locus_cases as Lc
import locus_ref as R
import motif_cases as Cs
import tract_ref as T
import unitparse_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


# ---------------------------------------------------------------------------------------------- 1: the rule on literals
def test_reference_on_the_prototype_table():
    assert len(Lc.TABLE) == 7
    for s, units, want, segs in Lc.TABLE:
        for f in (R.locus, R.locus_np):
            rec, got_segs = f(s, units)
            assert rec[:6] == want and rec[6] == want[4] + 1 == len(got_segs) and rec[7] == 0, (s, units)
            assert segs is None or [g[:3] for g in got_segs] == segs
            assert got_segs[0][1] == want[1] and got_segs[-1][2] == want[2] and all(a[2] == b[1] for a, b in zip(got_segs, got_segs[1:]))      # they tile the tract
            assert sum(g[3] for g in got_segs) == want[5] and sum(g[4] for g in got_segs) == want[3]
    # why: what the tools before this one give for the first allele
    s, units = Lc.TABLE[0][:2]
    assert P.unitparse_np(s, units)[0][0:3:2] == Lc.WHY["unitparse"]                # the flanks count as edits there
    cag, ccg = T.tract_np(s, b"CAG"), T.tract_np(s, b"CCG")
    assert (cag[1], cag[2], cag[4]) == Lc.WHY["tract_CAG"] and (ccg[1], ccg[2], ccg[0], ccg[4]) == Lc.WHY["tract_CCG"]
    # either unit alone scores 14 in the fifth row: no tract without the join
    s, units = Lc.TABLE[4][:2]
    assert [T.tract_np(s, u)[0] for u in units] == [14, 14] and [T.tract_np(s, u)[7] for u in units] == [T.NONE, T.NONE]
    assert R.locus(b"", [b"CAG"]) == R.locus_np(b"", [b"CAG"]) == ((0,) * 7 + (R.NONE,), [])
    assert R.locus_np(b"TTTCAGCAGCAGTTT", [b"CAG", b"CCG"]) == ((18, 0, 0, 0, 0, 0, 0, R.NONE), [])
    for bad in ([], [b""], [b"A" * 257], [b"A"] * 9, [b"A" * 200, b"C" * 100]):
        with pytest.raises(ValueError):
            R.locus_np(b"CAG", bad)
    assert R.MAX_LEN == P.MAX_LEN < T.MAX_LEN


# ---------------------------------------------------------------------------------------------- 2: the witness
def test_brute_force_witness_of_the_score():
    cases = Lc.tiny_set()
    assert len(cases) >= 200 and all(len(units) <= 2 and max(len(u) for u in units) <= 3 and len(s) <= 8 for s, units in cases)
    positive = 0
    for k, (s, units) in enumerate(cases):
        sc = Lc.SCORES[k % 3]
        if sc[0] >= sc[2]:
            s = s[:6]                                                       # a skip costs no more than a match gains: words of up to 2 L - 1 bases
        assert R.word_cap(len(s), sc[0], sc[2]) <= max(len(s) + 4, 11)
        loc = R.local(s, units, *sc)
        assert loc == R.local_np(s, units, *sc), (s, units, sc)
        assert loc[0] == R.score_brute(s, units, *sc), (s, units, sc)
        positive += loc[0] > 0
    assert positive >= 0.8 * len(cases)                                     # the witness is not vacuous (0.99 for this set)


# ---------------------------------------------------------------------------------------------- 3: the properties
def test_properties_of_the_rule():
    cases = Lc.random_set()
    n_tract = n_switch = 0
    for k, (s, units) in enumerate(cases):
        rec, segs = R.locus_np(s, units)
        score, b, e, ed, sw, ub, ns, f = rec
        if len(s) <= 150:
            assert R.locus(s, units) == (rec, segs), (s, units)
        nf = 1 + k % 5
        front = R.locus_np(b"N" * nf + s, units)                            # N bytes in front move the positions, behind change nothing
        assert R.locus_np(s + b"N" * nf, units) == (rec, segs)
        assert R.locus_np(s.swapcase(), units) == (rec, segs) and R.locus_np(s, [u.lower() for u in units]) == (rec, segs)
        if f:
            assert f == R.NONE and rec[1:7] == (0,) * 6 and segs == [] and front == (rec, segs)
            continue
        n_tract += 1
        n_switch += len(units) > 1 and sw > 0
        assert front == ((score, b + nf, e + nf, ed, sw, ub, ns, 0), [(u, x + nf, y + nf, n, d, ph) for u, x, y, n, d, ph in segs])
        assert 24 <= score <= 2 * (e - b) and b < e <= len(s) and ns == sw + 1 == len(segs)
        assert segs[0][1] == b and segs[-1][2] == e and all(x[2] == y[1] for x, y in zip(segs, segs[1:]))
        if len(units) == 1:                                                 # K = 1 is the tract mode
            t = T.tract_np(s, units[0])
            assert (t[0], t[1], t[2], t[3], t[4]) == (score, b, e, ed, ub) and sw == 0
    assert n_tract > len(cases) // 2 and n_switch > len(cases) // 4


def test_one_unit_gives_the_tract_mode():
    import tract_cases as Tc
    n = 0
    for s, u in Tc.random_set(n=90) + [(a, b) for a, b, _ in Tc.TABLE]:
        t = T.tract_np(s, u)
        rec, _ = R.locus_np(s, [u])
        assert rec[:4] == t[:4] and rec[5] == t[4] and (rec[7] == R.NONE) == (t[7] == T.NONE), (s, u)
        n += rec[7] == 0
    assert n > 60


# ---------------------------------------------------------------------------------------------- 4: the kernel's arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("locus_core") / "locus_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "locus_core_host.cpp")])
    return exe


def _run(exe, tasks, wide=0, seg64=0, scores=R.DEFAULT):
    """one batch -> per task ((score, begin, end, flags), (tier, class))"""
    text = "batch %d %d %d %d %d %d %d\n" % ((len(tasks), wide, seg64) + tuple(scores)) + \
        "".join("%s %s\n" % (s.hex() or "-", ",".join(u.hex() for u in units)) for s, units in tasks)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    rows = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]
    assert len(rows) == len(tasks)
    return [(t[:4], t[4:]) for t in rows]


def _narrow_len(exe, match, indel, lens):
    return int(subprocess.run([exe], input="narrow %d %d %s\n" % (match, indel, ",".join(str(p) for p in lens)), capture_output=True, text=True, timeout=60).stdout)


def _local_fields(rec):
    return (rec[0], rec[1], rec[2], rec[7])


def _wave_sets():
    rng = np.random.default_rng(97)
    return [[Cs.rs(rng, p) for p in lens] for lens, _ in Lc.CLASS_SETS[:5]]


@pytest.fixture(scope="module")
def small_sets():
    tasks = Lc.edge_set() + Lc.random_set(n=120) + Lc.tiny_set(n=40)
    for units in _wave_sets():                                              # sixteen unequal neighbours, classes 4 .. 64
        tasks += Lc.one_wave_batch(units)
    return tasks, [_local_fields(R.locus_np(s, units)[0]) for s, units in tasks]


@pytest.mark.parametrize("wide,seg64", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_core_arithmetic_against_the_rule(harness, small_sets, wide, seg64):
    tasks, want = small_sets
    got = _run(harness, tasks, wide, seg64)
    for (s, units), (g, _), w in zip(tasks, got, want):
        assert g == w, (s[:60], [u[:20] for u in units])
    ran = {tc for (g, tc), (s, _) in zip(got, tasks) if len(s)}
    assert ran == {(wide, c) for c in ((4, 5, 6) if seg64 else range(7))}     # every class ran, on the tier asked for
    for (s, units), (_, tc) in zip(tasks, got):
        assert not len(s) or tc[1] == R.unit_class([len(u) for u in units], seg64)
    assert sum(w[3] == 0 for w in want) > 250 and sum(w[3] == R.NONE for w in want) > 30


@pytest.mark.parametrize("scores", [(1, 1, 1, 5), (16, 64, 64, 100), (3, 2, 5, 0)])
def test_core_arithmetic_at_other_scores(harness, scores):
    tasks = Lc.edge_set()[::3] + Lc.random_set(n=80) + Lc.one_wave_batch(_wave_sets()[1]) + Lc.one_wave_batch(_wave_sets()[3])
    kw = dict(match=scores[0], mismatch=scores[1], indel=scores[2], min_score=scores[3])
    want = [_local_fields(R.locus_np(s, units, **kw)[0]) for s, units in tasks]
    for wide in (0, 1):
        got = _run(harness, tasks, wide, 0, scores)
        for (s, units), (g, _), w in zip(tasks, got, want):
            assert g == w, (s[:60], units, scores, wide)


@pytest.mark.parametrize("p,scores", [(37, R.DEFAULT), (256, R.DEFAULT), (256, (16, 64, 64, 24))])
def test_narrow_tier_at_its_bound(harness, p, scores):
    m, _, g, _ = scores
    tasks = Lc.bound_set(p, 4000)
    lens = [len(u) for u in tasks[0][1]]
    assert max(lens) == p
    L = _narrow_len(harness, m, g, lens)
    assert L == R.narrow_len(m, g, p) == T.narrow_len(m, g, p) == min(65535, (65535 - (p - 1) * g) // m)
    assert m * L + (p - 1) * g <= 65535 < m * (L + 1) + (p - 1) * g or L == 65535      # the largest score field a lane can hold
    cls = R.unit_class(lens)
    tasks = Lc.bound_set(p, L)
    assert all(len(s) == L for s, _ in tasks)
    narrow, wide = _run(harness, tasks, 0, 0, scores), _run(harness, tasks, 1, 0, scores)
    assert [tc for _, tc in narrow] == [(0, cls)] * 3 and [tc for _, tc in wide] == [(1, cls)] * 3
    assert [r for r, _ in narrow] == [r for r, _ in wide]
    assert narrow[0][0] == (m * L, 0, L, 0)                                 # the largest score
    assert narrow[1][0] == (m * 3 * p, L - 3 * p, L, 0)                     # the largest begin
    sc, b, e = R.local_np(*tasks[2], m, scores[1], g)
    assert narrow[2][0] == (sc, b, e, 0) and sc >= scores[3]
    # one base more leaves the narrow tier
    units = tasks[0][1]
    assert _run(harness, [(tasks[0][0] + units[-1][:1], units)], 0, 0, scores)[0][1] == (1, cls)


# ---------------------------------------------------------------------------------------------- 5: the row text
def test_emit_against_python_rows():
    CAG, CCG = b"CAG", b"CCG"
    seqs = [Lc.TABLE[0][0], Lc.TABLE[1][0].lower(), b"", b"ACGT", Lc.TABLE[3][0], b"TTT" + CAG * 3 + b"TTT", b"GATTACA"]
    sets = [[CAG, CCG], [b"GAA", b"AGAA"], [b"ccg"]]
    aset = [0, 0, 0, None, 1, 2, None]
    regions = [b"chr1:100-160", b"", b"chrUn_x:5-9"]
    first, n_al = [0, 3, 4], [3, 1, 3]
    records = np.zeros(3, dtype=abi.vcf_record_dt)
    pos = 0
    for r in range(3):
        records[r] = (pos, len(regions[r]), first[r], n_al[r], 0)
        pos += len(regions[r])
    res = [R.locus(s, sets[q]) if q is not None else ((0,) * 8, []) for s, q in zip(seqs, aset)]
    res[2] = ((0,) * 7 + (R.TOO_LONG,), [])                                 # a flagged record: zeros
    loci = np.array([r[0] for r in res], dtype=abi.locus_dt)
    seg_off = np.cumsum([0] + [len(r[1]) for r in res]).astype(np.uint64)
    segs = np.array([g for r in res for g in r[1]], dtype=abi.unitparse_seg_dt)
    text = otter_amd.locus_emit(records, b"".join(regions), [len(s) for s in seqs], aset, sets, loci, seg_off, segs)
    want = b"".join(R.row(regions[r], i, len(seqs[first[r] + i]), sets[aset[first[r] + i]] if aset[first[r] + i] is not None else [], *res[first[r] + i])
                    for r in range(3) for i in range(n_al[r]))
    assert text == want
    lines = want.split(b"\n")
    assert lines[0] == b"chr1:100-160\t0\t95\tCAG,CCG\t7\t88\t162\t0\t1\t81\t1.0000\t20.00,7.00\t(CAG)20(CCG)7"
    assert lines[1] == b"chr1:100-160\t1\t96\tCAG,CCG\t7\t89\t155\t1\t1\t81\t0.9878\t20.00,7.00\t(CAG)20~1(CCG)7"
    assert lines[2] == b"chr1:100-160\t2\t0\tCAG,CCG\t0\t0\t0\t0\t0\t0\t0.0000\t0.00,0.00\t."
    assert lines[3] == b"\t0\t4\t.\t0\t0\t0\t0\t0\t0\t0.0000\t.\t."
    assert lines[4] == b"chrUn_x:5-9\t0\t150\tGAA,AGAA\t2\t148\t292\t0\t2\t146\t1.0000\t42.00,5.00\t(GAA)31(AGAA)5(GAA)11"
    assert lines[5] == b"chrUn_x:5-9\t1\t15\tccg\t0\t0\t%d\t0\t0\t0\t0.0000\t0.00\t." % res[5][0][0] and len(lines) == 8
    assert otter_amd.locus_emit(records[:0], b"", [], [], [], loci[:0], [0], segs[:0]) == b""
    # the buffer protocol: the length without a buffer, a buffer one byte short
    L = otter_amd.load()
    reg = np.frombuffer(b"".join(regions) + b"\0", dtype=np.uint8)
    ln = np.array([len(s) for s in seqs], dtype=np.uint32)
    aset_a = np.array([abi.UNITPARSE_NO_SET if q is None else q for q in aset], dtype=np.uint32)
    flat = [u for s in sets for u in s]
    ulen = np.array([len(u) for u in flat], dtype=np.uint32)
    uoff = (np.cumsum(ulen) - ulen).astype(np.uint64)
    uar = np.frombuffer(b"".join(flat), dtype=np.uint8)
    set_first = np.cumsum([0] + [len(s) for s in sets]).astype(np.uint64)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(3), abi.ptr(reg), abi.ptr(ln), abi.ptr(aset_a), abi.ptr(set_first), abi.ptr(uar), abi.ptr(uoff), abi.ptr(ulen),
                             abi.ptr(loci), abi.ptr(seg_off), abi.ptr(segs), out, C.c_uint64(cap), C.byref(need))
    assert L.otg_locus_emit(*args(None, 0)) == abi.OTG_ERR_CAPACITY and need.value == len(want)
    buf = C.create_string_buffer(len(want))
    assert L.otg_locus_emit(*args(buf, len(want) - 1)) == abi.OTG_ERR_CAPACITY
    assert L.otg_locus_emit(*args(buf, len(want))) == 0 and buf.raw == want
    bad = segs.copy(); bad[0]["unit"] = 2                                   # a segment outside its set
    with pytest.raises(otter_amd.OtterGpuError, match="otg_locus_emit: segment 0 of allele 0 of record 0 names unit 2 of 2"):
        otter_amd.locus_emit(records, b"".join(regions), ln, aset, sets, loci, seg_off, bad)
    off = seg_off.copy(); off[1] = off[2] + 1
    with pytest.raises(otter_amd.OtterGpuError, match="decreases"):
        otter_amd.locus_emit(records, b"".join(regions), ln, aset, sets, loci, off, segs)


# ---------------------------------------------------------------------------------------------- 6: refusals without a device
def test_refusals_without_a_device(tmp_path):
    L = otter_amd.load()
    u, u64 = C.c_uint32, C.c_uint64
    one = np.zeros(1, dtype=np.uint32)
    assert L.otg_locus_batch(None, None, u64(0), None, None, u(0), None, u64(0), None, None, u(0), None, u(0), None, None, u(0), None, None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_locus_cohort(None, u(0), u(0), None, u64(0), None, None, u(0), None, u(0), None, None, u(0), None, None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_locus_collect(None, None, u64(0)) == abi.OTG_ERR_ARG
    assert L.otg_locus_device_results(None, abi.ptr(one), None, None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_locus_last_ms(None, None, None) == abi.OTG_ERR_ARG and L.otg_locus_last_tiers(None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_locus_emit(None, u(0), None, None, None, None, None, None, None, None, None, None, None, u64(0), None) == abi.OTG_ERR_ARG
    assert L.otg_loci_files(None, None, None, None) == abi.OTG_ERR_ARG
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\tCAG,CCG\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    for kw, msg in ((dict(match=0), "invalid '--scores' (0,7,7). Needs to be 1 <= match <= 16, 1 <= mismatch <= 64, 1 <= indel <= 64."),
                    (dict(match=17), "invalid '--scores' (17,7,7)"), (dict(mismatch=65), "invalid '--scores' (2,65,7)"), (dict(indel=0), "invalid '--scores' (2,7,0)"),
                    (dict(min_score=(1 << 24) + 1), "invalid '--min-score' (16777217). Needs to be 0 <= x <= 16777216.")):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.loci_files(vcf, bed, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and msg in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.loci_files(vcf, str(tmp_path / "missing.bed"))
    exe = os.path.join(ROOT, "tools", "otter_loci")
    for args, msg in ((["--scores", "0,7,7"], b"invalid '--scores' (0,7,7). Needs to be 1 <= match <= 16, 1 <= mismatch <= 64, 1 <= indel <= 64."),
                      (["--scores=2,7,65"], b"invalid '--scores' (2,7,65)"), (["--min-score", "16777217"], b"invalid '--min-score' (16777217). Needs to be 0 <= x <= 16777216."),
                      (["--min-score=-1"], b"invalid '--min-score' (-1)"), (["--scores", "2,7"], None), (["--scores", "2,x,7"], None), (["--min-score", "x"], None)):
        r = subprocess.run([exe, "-b", bed] + args + [vcf], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout.count(b"\t") == 0, (args, r)
        assert msg is None or msg in r.stderr
    assert subprocess.run([exe, vcf], capture_output=True, timeout=60).returncode == 1           # no BED
    assert subprocess.run([exe, "-b", str(tmp_path / "missing.bed"), vcf], capture_output=True, timeout=60).returncode == 1
    r = subprocess.run([exe], capture_output=True, timeout=60)                                   # the usage text
    assert r.returncode == 0 and b"Usage:" in r.stdout and all(w in r.stdout for w in (b"--bed", b"--scores", b"--min-score", b"--threads", b"--batch"))
    assert b"--max-period" not in r.stdout and b"--slack" not in r.stdout


# ---------------------------------------------------------------------------------------------- 7: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: v for k, v in re.findall(r"#define\s+(OTG_LOCUS_[A-Z_0-9]+)\s+(\S+)", txt)}
    assert set(defs) == {"OTG_LOCUS_MAX_LEN", "OTG_LOCUS_TOO_LONG", "OTG_LOCUS_NONE"}
    assert defs["OTG_LOCUS_MAX_LEN"] == "OTG_UNITPARSE_MAX_LEN" and abi.LOCUS_MAX_LEN == abi.UNITPARSE_MAX_LEN == R.MAX_LEN == 1048320 < abi.TRACT_MAX_LEN
    assert (int(defs["OTG_LOCUS_TOO_LONG"].rstrip("u")), int(defs["OTG_LOCUS_NONE"].rstrip("u"))) == (R.TOO_LONG, R.NONE) == (abi.LOCUS_TOO_LONG, abi.LOCUS_NONE) == (1, 2)
    assert 16 * abi.LOCUS_MAX_LEN + 255 * 64 < 2 ** 32                      # the wide tier's score field holds every task
    body = re.search(r"typedef struct otg_locus \{(.*?)\} otg_locus;", txt, flags=re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == list(abi.locus_dt.names) == ["score", "begin", "end", "edits", "switches", "unit_bases", "n_segments", "flags"]
    body = re.search(r"typedef struct otg_loci_job \{(.*?)\} otg_loci_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.LociJob._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n",sizeof(otg_locus),'
                   'offsetof(otg_locus,flags),sizeof(otg_loci_job),offsetof(otg_loci_job,min_score),offsetof(otg_loci_job,batch_alleles),OTG_LOCUS_MAX_LEN);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.locus_dt.itemsize, abi.locus_dt.fields["flags"][1], C.sizeof(abi.LociJob), abi.LociJob.min_score.offset, abi.LociJob.batch_alleles.offset,
                   abi.LOCUS_MAX_LEN]
    names = {"otg_locus_batch", "otg_locus_collect", "otg_locus_device_results", "otg_locus_last_ms", "otg_locus_last_tiers", "otg_locus_cohort", "otg_locus_emit", "otg_loci_files"}
    assert {n for n in otter_amd.EXPORTS if n.startswith(("otg_locus", "otg_loci"))} == names
    assert not [n for n in names if n.startswith(("otg_tract", "otg_unitparse", "otg_unitalign", "otg_motif", "otg_repeat"))]
    lib = otter_amd.load()
    for n in names:
        assert getattr(lib, n) is not None
    for f in ("locus_batch", "locus_last_ms", "locus_last_tiers", "cohort_loci"):
        assert callable(getattr(otter_amd.Context, f))
    assert callable(otter_amd.locus_emit) and callable(otter_amd.loci_files)

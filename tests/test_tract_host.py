"""CPU: the tract mode of the copy numbers without a device.

1. the nine results the rule was prototyped with as literals, through both forms of tests/tract_ref.py (the rule restated from
   include/otter_gpu.h), next to what the global unit alignment gives for the same alleles;
2. an independent witness of the score: a brute-force local alignment over every start phase == the DP on 360 tiny cases at three score sets;
3. the properties that follow from the rule on a random set;
4. the kernel's arithmetic (otter_amd/csrc/otg_tract_core.hpp) run on the host in the kernel's schedule by tests/tract_core_host.cpp, a
   stand-alone program built with -fsanitize=address,undefined, == tract_ref: every segment class, both key widths, seg64 on and off,
   finished neighbours, other scores, and the narrow tier at its derived bound;
5. otg_tract_emit against rows formatted in Python; 6. the refusals that need no device and the tool's messages; 7. the ABI mirrors."""
import ctypes as C
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
import tract_cases as Tc
import tract_ref as R
import unitalign_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


# ---------------------------------------------------------------------------------------------- 1: the rule on literals
def test_reference_on_the_prototype_table():
    assert len(Tc.TABLE) == 9
    for k, (s, u, want) in enumerate(Tc.TABLE):
        for f in (R.tract, R.tract_np):
            got = f(s, u)
            if isinstance(want, tuple):
                assert got[:6] == want and got[7] == 0 and got[6] == (want[5] - want[4]) % len(u), (s, u)
            else:
                assert got == (want, 0, 0, 0, 0, 0, 0, R.NONE), (s, u)
        if k < len(Tc.GLOBAL):
            assert U.unitalign_np(s, u)[:2] == Tc.GLOBAL[k]                 # the flanks count as edits there
    s, u, _ = Tc.TABLE[7]
    assert R.tract(s, u, min_score=0)[:3] == R.tract_np(s, u, min_score=0)[:3] == (18, 3, 12)
    assert R.tract(b"CAG", b"") == (0,) * 7 + (R.NO_UNIT,) and R.tract_np(b"", b"CAG") == (0,) * 7 + (R.NONE,)
    assert R.tract(b"CAG", b"A" * 257, chained=True) == (0,) * 7 + (R.UNIT_TOO_LONG,)
    with pytest.raises(ValueError):
        R.tract(b"CAG", b"A" * 257)
    assert R.refusal(R.MAX_LEN + 1, 3) == R.TOO_LONG and R.refusal(R.MAX_LEN, 3) == 0


# ---------------------------------------------------------------------------------------------- 2: the witness
def test_brute_force_witness_of_the_score():
    cases = Tc.tiny_set()
    assert len(cases) >= 300 and all(len(u) <= 7 and len(s) <= 14 for s, u in cases)
    positive = 0
    for k, (s, u) in enumerate(cases):
        sc = Tc.SCORES[k % 3]
        loc = R.local(s, u, *sc)
        assert loc == R.local_np(s, u, *sc), (s, u, sc)
        assert loc[0] == R.score_brute(s, u, *sc), (s, u, sc)
        positive += loc[0] > 0
    assert positive >= 0.8 * len(cases)                                     # the witness is not vacuous


# ---------------------------------------------------------------------------------------------- 3: the properties
def test_properties_of_the_rule():
    n_tract = n_edits = 0
    for k, (s, u) in enumerate(Tc.random_set(n=150)):
        rec = R.tract_np(s, u)
        score, b, e, ed, ub, ph, sp, f = rec
        if len(s) <= 120 and len(u) <= 12:
            assert R.tract(s, u) == rec, (s, u)
        nf = 1 + k % 5
        front = R.tract_np(b"N" * nf + s, u)                               # N bytes in front move begin and end, behind change nothing
        assert R.tract_np(s + b"N" * nf, u) == rec
        assert R.tract_np(s.lower(), u) == rec and R.tract_np(s, u.lower()) == rec
        if f:
            assert f == R.NONE and rec[1:7] == (0,) * 6 and front == rec
            continue
        n_tract += 1
        n_edits += ed > 0
        assert front == (score, b + nf, e + nf, ed, ub, ph, sp, 0)
        assert 24 <= score <= 2 * (e - b) and b < e <= len(s) and ph < len(u) and sp == (ph - ub) % len(u)
        cs, cu = U.codes(s), U.codes(u)
        assert cs[b] < 4 and cs[b] == cu[sp] and cs[e - 1] == cu[(ph - 1) % len(u)]      # it begins and ends on a match
        for r in (1, len(u) // 2):                                         # a rotated unit changes only the two phases
            r %= len(u)
            rot = R.tract_np(s, u[r:] + u[:r])
            assert rot[:5] == rec[:5] and rot[7] == 0 and (rot[6] - rot[5]) % len(u) == (sp - ph) % len(u)
            if ed == 0 and all(u[q:] + u[:q] != u for q in range(1, len(u))):      # one path only: the phases turn with the unit
                assert (rot[5] + r) % len(u) == ph and (rot[6] + r) % len(u) == sp
    assert n_tract > 100 and n_edits > 50


# ---------------------------------------------------------------------------------------------- 4: the kernel's arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("tract_core") / "tract_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "tract_core_host.cpp")])
    return exe


def _run(exe, pairs, wide=0, seg64=0, scores=R.DEFAULT):
    """one batch -> per task ((score, begin, end, flags), (tier, class))"""
    text = "batch %d %d %d %d %d %d %d\n" % ((len(pairs), wide, seg64) + tuple(scores)) + "".join("%s %s\n" % (s.hex() or "-", u.hex() or "-") for s, u in pairs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    rows = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]
    assert len(rows) == len(pairs)
    return [(t[:4], t[4:]) for t in rows]


def _narrow_len(exe, match, indel, p):
    return int(subprocess.run([exe], input="narrow %d %d %d\n" % (match, indel, p), capture_output=True, text=True, timeout=60).stdout)


def _local_fields(rec):
    return (rec[0], rec[1], rec[2], rec[7])


@pytest.fixture(scope="module")
def small_sets():
    pairs = Tc.edge_set() + Tc.random_set() + Tc.tiny_set(n=60)
    for p in (3, 7, 13, 29):                                               # sixteen unequal neighbours in one wave, classes 4 .. 32
        pairs += Tc.one_wave_batch(p)
    return pairs, [_local_fields(R.tract_np(s, u)) for s, u in pairs]


@pytest.mark.parametrize("wide,seg64", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_core_arithmetic_against_the_rule(harness, small_sets, wide, seg64):
    pairs, want = small_sets
    got = _run(harness, pairs, wide, seg64)
    for (s, u), (g, _), w in zip(pairs, got, want):
        assert g == w, (s[:60], u[:60])
    ran = {tc for (g, tc), (s, u) in zip(got, pairs) if len(s) and len(u)}
    assert ran == {(wide, c) for c in ((4, 5, 6) if seg64 else range(7))}     # every segment class ran, on the tier asked for
    assert sum(w[3] == 0 for w in want) > 500 and sum(w[3] == R.NONE for w in want) > 50


@pytest.mark.parametrize("scores", [(1, 1, 1, 5), (16, 64, 64, 100), (3, 2, 5, 0)])
def test_core_arithmetic_at_other_scores(harness, scores):
    pairs = Tc.edge_set()[::3] + Tc.random_set(n=120) + Tc.one_wave_batch(7) + Tc.one_wave_batch(29)
    kw = dict(match=scores[0], mismatch=scores[1], indel=scores[2], min_score=scores[3])
    want = [_local_fields(R.tract_np(s, u, **kw)) for s, u in pairs]
    for wide in (0, 1):
        got = _run(harness, pairs, wide, 0, scores)
        for (s, u), (g, _), w in zip(pairs, got, want):
            assert g == w, (s[:60], u[:60], scores, wide)


def test_short_sets_agree_with_the_plain_reference(small_sets):
    pairs, want = small_sets
    n = 0
    for (s, u), w in zip(pairs, want):
        if len(u) <= 9 and len(s) <= 160:
            assert _local_fields(R.tract(s, u)) == w, (s, u)
            n += 1
    assert n > 250


@pytest.mark.parametrize("p,scores", [(37, R.DEFAULT), (256, R.DEFAULT), (256, (16, 64, 64, 24))])
def test_narrow_tier_at_its_bound(harness, p, scores):
    m, _, g, _ = scores
    L = _narrow_len(harness, m, g, p)
    assert L == R.narrow_len(m, g, p) == min(65535, (65535 - (p - 1) * g) // m)
    assert m * L + (p - 1) * g <= 65535 < m * (L + 1) + (p - 1) * g or L == 65535      # the largest score field a lane can hold
    cls = abi_class(p)
    pairs = Tc.bound_set(p, L)
    assert all(len(s) == L for s, _ in pairs)
    narrow, wide = _run(harness, pairs, 0, 0, scores), _run(harness, pairs, 1, 0, scores)
    assert [tc for _, tc in narrow] == [(0, cls)] * 3 and [tc for _, tc in wide] == [(1, cls)] * 3
    assert [r for r, _ in narrow] == [r for r, _ in wide]
    assert narrow[0][0] == (m * L, 0, L, 0)                                 # the largest score
    assert narrow[1][0] == (m * 3 * p, L - 3 * p, L, 0)                     # the largest begin
    kw = dict(match=m, mismatch=scores[1], indel=g, min_score=scores[3])
    assert narrow[2][0] == _local_fields(R.tract_np(*pairs[2], **kw))
    # one base more leaves the narrow tier
    unit = pairs[0][1]
    assert _run(harness, [(pairs[0][0] + unit[:1], unit)], 0, 0, scores)[0][1] == (1, cls)


def abi_class(p):
    return 6 if p > 128 else 5 if p > 64 else 4 if p > 32 else 3 if p > 16 else 2 if p > 8 else 1 if p > 4 else 0


# ---------------------------------------------------------------------------------------------- 5: the row text
def test_emit_against_python_rows():
    seqs = [Tc.TABLE[1][0], b"ttt" + b"cag" * 20 + b"gg", b"", b"ACGT", b"A" * 40, b"GATTACA"]
    regions = [b"chr1:100-160", b"", b"chrUn_x:5-9"]
    first, n_al = [0, 3, 4], [3, 1, 2]
    records = np.zeros(3, dtype=abi.vcf_record_dt)
    pos = 0
    for r in range(3):
        records[r] = (pos, len(regions[r]), first[r], n_al[r], 0)
        pos += len(regions[r])
    # allele -> [(source, unit, record)]: two catalogue units, a motif unit, an empty allele, no unit, flagged rows, no tract
    tasks = [[(0, b"CAG", R.tract(seqs[0], b"CAG")), (0, b"ccg", R.tract(seqs[0], b"ccg"))],
             [(1, b"AGC", R.tract(seqs[1], b"AGC"))],
             [(0, b"CAG", R.tract(seqs[2], b"CAG"))],
             [(1, b"", (0,) * 7 + (R.NO_UNIT,))],
             [(1, b"A" * 300, (0,) * 7 + (R.UNIT_TOO_LONG,)), (0, b"A", (0,) * 7 + (R.TOO_LONG,)), (0, b"A", R.tract(seqs[4], b"A"))],
             []]
    task_first = np.cumsum([0] + [len(t) for t in tasks]).astype(np.uint64)
    flat = [t for ts in tasks for t in ts]
    tracts = np.array([t[2] for t in flat], dtype=abi.tract_dt)
    text = otter_amd.tract_emit(records, b"".join(regions), [len(s) for s in seqs], task_first, [t[0] for t in flat], [t[1] for t in flat], tracts)
    want = b"".join(R.row(regions[r], i, len(seqs[first[r] + i]), (b"bed", b"motif")[src], unit, rec)
                    for r in range(3) for i in range(n_al[r]) for src, unit, rec in tasks[first[r] + i])
    assert text == want
    lines = want.split(b"\n")
    assert lines[0] == b"chr1:100-160\t0\t75\tbed\tCAG\t7\t68\t113\t1\t60\t20.00\t0.9836"
    assert lines[1] == b"chr1:100-160\t0\t75\tbed\tccg\t0\t0\t%d\t0\t0\t0.00\t0.0000" % R.tract(seqs[0], b"ccg")[0]
    assert lines[2] == b"chr1:100-160\t1\t65\tmotif\tAGC\t3\t63\t120\t0\t60\t20.00\t1.0000"
    assert lines[3] == b"chr1:100-160\t2\t0\tbed\tCAG\t0\t0\t0\t0\t0\t0.00\t0.0000" and lines[4] == b"\t0\t4\tmotif\t.\t0\t0\t0\t0\t0\t0.00\t0.0000"
    assert lines[7] == b"chrUn_x:5-9\t0\t40\tbed\tA\t0\t40\t80\t0\t40\t40.00\t1.0000" and len(lines) == 9
    assert otter_amd.tract_emit(records[:0], b"", [], [0], [], [], tracts[:0]) == b""
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
                             abi.ptr(ulen), abi.ptr(tracts), out, C.c_uint64(cap), C.byref(need))
    assert L.otg_tract_emit(*args(None, 0)) == abi.OTG_ERR_CAPACITY and need.value == len(want)
    buf = C.create_string_buffer(len(want))
    assert L.otg_tract_emit(*args(buf, len(want) - 1)) == abi.OTG_ERR_CAPACITY
    assert L.otg_tract_emit(*args(buf, len(want))) == 0 and buf.raw == want
    task_first[2] = 1                                                      # fewer tasks behind than in front
    with pytest.raises(otter_amd.OtterGpuError, match="decreases"):
        otter_amd.tract_emit(records, b"".join(regions), ln, task_first, src, [t[1] for t in flat], tracts)


# ---------------------------------------------------------------------------------------------- 6: refusals without a device
def test_parameter_rule():
    q = abi.TractParams(9, 9, 9, 9)
    otter_amd.load().otg_tract_params_default(C.byref(q))
    assert (q.match, q.mismatch, q.indel, q.min_score) == R.DEFAULT == (2, 7, 7, 24)
    assert R.params_ok(*R.DEFAULT) and R.params_ok(1, 1, 1, 0) and R.params_ok(16, 64, 64, 1 << 24)
    for bad in ((0, 7, 7, 24), (17, 7, 7, 24), (2, 0, 7, 24), (2, 65, 7, 24), (2, 7, 0, 24), (2, 7, 65, 24), (2, 7, 7, (1 << 24) + 1)):
        assert not R.params_ok(*bad)


def test_refusals_without_a_device(tmp_path):
    L = otter_amd.load()
    u, u64 = C.c_uint32, C.c_uint64
    one = np.zeros(1, dtype=np.uint32)
    assert L.otg_tract_batch(None, None, u64(0), None, None, u(0), None, u64(0), None, None, u(0), None, None, u(0), None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_tract_motifs(None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_tract_cohort(None, u(0), u(0), None, u64(0), None, None, u(0), None, None, u(0), None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_tract_device_results(None, abi.ptr(one), None) == abi.OTG_ERR_ARG
    assert L.otg_tract_last_ms(None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_tract_emit(None, u(0), None, None, None, None, None, None, None, None, None, u64(0), None) == abi.OTG_ERR_ARG
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\tCAG\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    for kw, msg in ((dict(max_period=0), "invalid '--max-period' (0). Needs to be 1 <= x <= 4096."),
                    (dict(slack=1000), "invalid '--slack' (1000). Needs to be 0 <= x <= 999."),
                    (dict(match=0), "invalid '--scores' (0,7,7). Needs to be 1 <= match <= 16, 1 <= mismatch <= 64, 1 <= indel <= 64."),
                    (dict(match=17), "invalid '--scores' (17,7,7)"), (dict(mismatch=65), "invalid '--scores' (2,65,7)"), (dict(indel=0), "invalid '--scores' (2,7,0)"),
                    (dict(min_score=(1 << 24) + 1), "invalid '--min-score' (16777217). Needs to be 0 <= x <= 16777216.")):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.tracts_files(vcf, bed, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and msg in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.tracts_files(vcf, str(tmp_path / "missing.bed"))
    exe = os.path.join(ROOT, "tools", "otter_tracts")
    for args, msg in ((["-p", "0"], b"invalid '--max-period' (0). Needs to be 1 <= x <= 4096."), (["--slack", "1000"], b"invalid '--slack' (1000). Needs to be 0 <= x <= 999."),
                      (["--scores", "0,7,7"], b"invalid '--scores' (0,7,7). Needs to be 1 <= match <= 16, 1 <= mismatch <= 64, 1 <= indel <= 64."),
                      (["--scores=2,7,65"], b"invalid '--scores' (2,7,65)"), (["--min-score", "16777217"], b"invalid '--min-score' (16777217). Needs to be 0 <= x <= 16777216."),
                      (["--min-score=-1"], b"invalid '--min-score' (-1)"), (["--scores", "2,7"], None), (["--scores", "2,x,7"], None), (["--min-score", "x"], None)):
        r = subprocess.run([exe, "-b", bed] + args + [vcf], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout.count(b"\t") == 0, (args, r)
        assert msg is None or msg in r.stderr
    assert subprocess.run([exe, vcf], capture_output=True, timeout=60).returncode == 1           # no BED
    assert subprocess.run([exe, "-b", str(tmp_path / "missing.bed"), vcf], capture_output=True, timeout=60).returncode == 1
    r = subprocess.run([exe], capture_output=True, timeout=60)                                   # the usage text
    assert r.returncode == 0 and b"Usage:" in r.stdout and all(w in r.stdout for w in (b"--max-period", b"--slack", b"--scores", b"--min-score", b"--batch"))


# ---------------------------------------------------------------------------------------------- 7: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: v for k, v in re.findall(r"#define\s+(OTG_TRACT_[A-Z_0-9]+)\s+(\S+)", txt)}
    assert set(defs) == {"OTG_TRACT_MAX_LEN", "OTG_TRACT_NO_UNIT", "OTG_TRACT_TOO_LONG", "OTG_TRACT_UNIT_TOO_LONG", "OTG_TRACT_NONE"}
    num = lambda k: int(defs[k].rstrip("u"))
    assert num("OTG_TRACT_MAX_LEN") == abi.TRACT_MAX_LEN == R.MAX_LEN == 1048575
    assert (num("OTG_TRACT_NO_UNIT"), num("OTG_TRACT_TOO_LONG"), num("OTG_TRACT_UNIT_TOO_LONG"), num("OTG_TRACT_NONE")) == (R.NO_UNIT, R.TOO_LONG, R.UNIT_TOO_LONG, R.NONE) \
        == (abi.TRACT_NO_UNIT, abi.TRACT_TOO_LONG, abi.TRACT_UNIT_TOO_LONG, abi.TRACT_NONE) == (1, 2, 4, 8)
    assert 16 * abi.TRACT_MAX_LEN + 255 * 64 < 2 ** 32                      # the wide tier's score field holds every task
    body = re.search(r"typedef struct otg_tract \{(.*?)\} otg_tract;", txt, flags=re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == list(abi.tract_dt.names) == ["score", "begin", "end", "edits", "unit_bases", "end_phase", "start_phase", "flags"]
    body = re.search(r"typedef struct otg_tract_params \{(.*?)\} otg_tract_params;", txt, flags=re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == [n for n, _ in abi.TractParams._fields_]
    body = re.search(r"typedef struct otg_tracts_job \{(.*?)\} otg_tracts_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.TractsJob._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(otg_tract),'
                   'offsetof(otg_tract,flags),sizeof(otg_tract_params),offsetof(otg_tract_params,min_score),sizeof(otg_tracts_job),'
                   'offsetof(otg_tracts_job,batch_alleles));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.tract_dt.itemsize, abi.tract_dt.fields["flags"][1], C.sizeof(abi.TractParams), abi.TractParams.min_score.offset, C.sizeof(abi.TractsJob),
                   abi.TractsJob.batch_alleles.offset]
    names = {"otg_tract_params_default", "otg_tract_batch", "otg_tract_motifs", "otg_tract_cohort", "otg_tract_device_results", "otg_tract_last_ms", "otg_tract_emit",
             "otg_tracts_files"}
    assert {n for n in otter_amd.EXPORTS if n.startswith("otg_tract")} == names
    assert not [n for n in names if n.startswith(("otg_unitalign", "otg_unitparse", "otg_motif", "otg_repeat"))]
    lib = otter_amd.load()
    for n in names:
        assert getattr(lib, n) is not None

"""CPU: the repeat structure of alleles without a device.

1. tests/repeat_ref.py (the rule restated from include/otter_gpu.h) on the hand-derived table;
2. the three invariants of the rule on the edge and random sets under six parameter sets;
3. the kernels' arithmetic (otter_amd/csrc/otg_repeat_core.hpp: the run walk, the candidate order, the unit compare) run on the host in the
   kernels' schedule by tests/repeat_core_host.cpp, a stand-alone program built with -fsanitize=address,undefined, == repeat_ref;
4. otg_repeat_emit against rows formatted in Python; 5. the refusals that need no device; 6. the ABI mirrors."""
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
import repeat_cases as Rc
import repeat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


# ---------------------------------------------------------------------------------------------- 1: the rule on literals
def test_reference_on_the_hand_derived_table():
    for seq, segs, text in Rc.TABLE:
        r = R.structure(seq)
        assert r["segs"] == segs and R.text(seq, segs) == text, seq
        assert R.structure(seq.lower())["segs"] == segs
        assert (r["n_segments"], r["n_repeats"], r["covered"], r["flags"]) == (len(segs), sum(1 for s in segs if s[1]), sum(s[3] for s in segs if s[1]), 0)
        R.check_invariants(seq, r["segs"])
    assert R.structure(b"CAG" * 10 + b"CTG" + b"CAG" * 9)["moved"] == 1     # (CAG)9 begins at 33, not at the run's first base 31
    assert R.structure(b"AC")["segs"] == [(0, 0, 0, 2)] and R.structure(b"A")["segs"] == [(0, 0, 0, 1)]
    # min_copies / min_span raised until a run drops out
    s = b"CAG" * 10 + b"CTG" + b"CAG" * 9
    assert R.structure(s, min_copies=10)["segs"] == [(0, 3, 10, 30), (30, 0, 0, 30)]
    assert R.structure(s, min_copies=11)["segs"] == [(0, 0, 0, 60)]
    assert R.structure(s, min_span=28)["segs"] == [(0, 3, 10, 30), (30, 0, 0, 30)]     # the second run covers [31, 60): 9 copies, 27 bases
    assert R.structure(s, min_span=31)["segs"] == [(0, 0, 0, 60)]
    assert R.structure(b"T" * 12 + b"GATTACAG" + b"CAG" * 100, min_span=13)["segs"] == [(0, 0, 0, 17), (17, 3, 101, 303)]
    assert R.structure(b"CAG" * 20, max_period=2)["segs"] == [(0, 0, 0, 60)]           # CAG has no match at 1 or 2
    rng = np.random.default_rng(5)
    unit = bytearray(Cs.rs(rng, 30)); unit[9:21] = b"A" * 12
    assert R.structure(bytes(unit) * 10)["segs"] == [(0, 30, 10, 300)]                 # the whole beats the A-run inside every copy
    long = R.structure(b"A" * (R.MAX_LEN + 1))
    assert long["segs"] == [(0, 0, 0, R.MAX_LEN + 1)] and long["flags"] == R.TOO_LONG and long["n_repeats"] == 0
    deep = R.structure(Rc.deep_stack())
    assert deep["depth"] >= 3 and [s[1] for s in deep["segs"]] == [0, 1, 0, 1, 0, 1, 0, 1]


# ---------------------------------------------------------------------------------------------- 2: the invariants
@pytest.mark.parametrize("params", Rc.PARAM_SETS)
def test_invariants_of_the_rule(params):
    n_multi = 0
    for seq in Cs.edge_set() + Cs.random_set():
        r = R.structure_cached(seq, *params)
        R.check_invariants(seq, r["segs"])
        assert r["n_segments"] <= 2 * r["n_runs"] + 1 and r["depth"] <= r["n_runs"]          # what the device sizes its scratch and its stack from
        for b, p, k, ln in r["segs"]:
            assert p <= params[0] and (p == 0 or (k >= params[1] and ln >= params[2]))
        n_multi += r["n_segments"] > 1
    assert params != (256, 2, 12) or n_multi >= 150


# ---------------------------------------------------------------------------------------------- 3: the kernels' arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("repeat_core") / "repeat_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "repeat_core_host.cpp")])
    return exe


def _run(exe, cases):
    """cases: (seq, max_period, min_copies, min_span) -> (flags, n_repeats, covered, segments) per case"""
    text = "".join("%d %d %d %s\n" % (mp, mc, ms, seq.hex() or "-") for seq, mp, mc, ms in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    out = []
    for l in r.stdout.splitlines():
        f = l.split()
        segs = [tuple(int(x) for x in g.split(",")) for g in f[4:]]
        assert len(segs) == int(f[3])
        out.append((int(f[0]), int(f[1]), int(f[2]), segs))
    assert len(out) == len(cases)
    return out


def test_core_arithmetic_against_the_rule(harness):
    cases = [(s, 256, 2, 12) for s in Cs.edge_set() + Cs.random_set() + [t[0] for t in Rc.TABLE] + [Rc.deep_stack()]]
    cases += [(s, mp, mc, ms) for s in Rc.word_edge_set() for mp in Rc.EDGE_PERIODS for mc, ms in Rc.EDGE_ENOUGH]
    cases += [(s, *p) for s in Cs.edge_set()[::2] for p in Rc.PARAM_SETS[1:]]
    rng = np.random.default_rng(3)
    unit = Cs.rs(rng, 300)
    cases += [(unit * 4, 4096, 2, 12), (unit * 4, 299, 2, 12), (Cs.rs(rng, 700) * 3, 4096, 2, 12),
              (Cs.substitute(rng, Cs.rs(rng, 700) * 3, 5), 4096, 2, 12)]      # periods beyond one workgroup's threads
    got = _run(harness, cases)
    moved = 0
    for (seq, mp, mc, ms), g in zip(cases, got):
        r = R.structure_cached(seq, mp, mc, ms)
        assert g == (r["flags"], r["n_repeats"], r["covered"], r["segs"]), (seq, mp, mc, ms)
        moved += r["moved"]
    assert moved > 20 and sum(any(s[1] > 256 for s in g[3]) for g in got) >= 2


# ---------------------------------------------------------------------------------------------- 4: the row text
def _pack(seqs):
    off = np.cumsum([0] + [len(s) for s in seqs])[:-1].astype(np.uint64)
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:-1].copy(), off, np.array([len(s) for s in seqs], dtype=np.uint32)


def _results(exp):
    sums = np.zeros(len(exp), dtype=abi.repeat_sum_dt)
    for i, e in enumerate(exp):
        sums[i] = (e["n_segments"], e["n_repeats"], e["covered"], e["flags"])
    seg_off = np.cumsum([0] + [e["n_segments"] for e in exp]).astype(np.uint64)
    segs = np.array([s for e in exp for s in e["segs"]], dtype=abi.repeat_seg_dt) if seg_off[-1] else np.zeros(0, dtype=abi.repeat_seg_dt)
    return sums, seg_off, segs


def test_emit_against_python_rows():
    seqs = [b"CAG" * 20 + b"CCG" * 20, b"cag" * 10 + b"ctg" + b"cag" * 9, b"AC", b"", b"A" * 24 + b"CGT" * 8 + b"AGTC",
            b"ACGTTGCATTGACCTGAACGTGCAT" + b"GA" * 9, b"ACGTTGCATTGACCTGAACGTGCC" + b"GA" * 9]
    exp = [R.structure(s) for s in seqs]
    assert exp[5]["segs"][0] == (0, 0, 0, 25) and exp[6]["segs"][0] == (0, 0, 0, 24)             # a literal of 25 and of 24 bytes
    arena, off, ln = _pack(seqs)
    regions = [b"chr1:100-150", b"", b"chrUn_x:5-9"]
    records = np.zeros(3, dtype=abi.vcf_record_dt)
    first, n_al, pos = [0, 3, 4], [3, 1, 3], 0
    for r in range(3):
        records[r] = (pos, len(regions[r]), first[r], n_al[r], 0)
        pos += len(regions[r])
    sums, seg_off, segs = _results(exp)
    text = otter_amd.repeat_emit(records, b"".join(regions), arena, off, ln, sums, seg_off, segs)
    want = b"".join(R.row(regions[r], i, seqs[first[r] + i], exp[first[r] + i]) for r in range(3) for i in range(n_al[r]))
    assert text == want
    lines = want.split(b"\n")
    assert lines[0] == b"chr1:100-150\t0\t120\t2\t120\t(CAG)20(CCG)20" and lines[1] == b"chr1:100-150\t1\t60\t2\t57\t(CAG)10ctg(CAG)9"
    assert lines[2].endswith(b"\t2\t0\t0\tAC") and lines[3] == b"\t0\t0\t0\t0\t." and lines[5].endswith(b"\t[25](GA)9")
    assert lines[6].endswith(b"\tACGTTGCATTGACCTGAACGTGCC(GA)9")
    assert otter_amd.repeat_emit(records[:0], b"", arena[:0], off[:0], ln[:0], sums[:0], seg_off[:1], segs[:0]) == b""
    # the buffer protocol: the length without a buffer, a buffer one byte short
    L = otter_amd.load()
    reg = np.frombuffer(b"".join(regions) + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(3), abi.ptr(reg), abi.ptr(arena), abi.ptr(off), abi.ptr(ln), abi.ptr(sums), abi.ptr(seg_off),
                             abi.ptr(segs), out, C.c_uint64(cap), C.byref(need))
    assert L.otg_repeat_emit(*args(None, 0)) == abi.OTG_ERR_CAPACITY and need.value == len(want)
    buf = C.create_string_buffer(len(want))
    assert L.otg_repeat_emit(*args(buf, len(want) - 1)) == abi.OTG_ERR_CAPACITY
    assert L.otg_repeat_emit(*args(buf, len(want))) == 0 and buf.raw == want
    segs[0]["length"] = 121                                                # a segment that leaves its allele
    with pytest.raises(otter_amd.OtterGpuError, match="outside the allele"):
        otter_amd.repeat_emit(records, b"".join(regions), arena, off, ln, sums, seg_off, segs)


# ---------------------------------------------------------------------------------------------- 5: refusals without a device
def test_refusals_without_a_device(tmp_path):
    L = otter_amd.load()
    one = np.zeros(1, dtype=np.uint32)
    u = C.c_uint32
    assert L.otg_repeat_batch(None, None, C.c_uint64(0), None, None, u(1), u(256), u(2), u(12), None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_repeat_cohort(None, u(0), u(0), u(256), u(2), u(12), None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_repeat_collect(None, None, C.c_uint64(0)) == abi.OTG_ERR_ARG
    assert L.otg_repeat_device_results(None, abi.ptr(one), None, None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_repeat_last_ms(None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_repeat_emit(None, u(0), None, None, None, None, None, None, None, None, C.c_uint64(0), None) == abi.OTG_ERR_ARG
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    for kw, msg in ((dict(max_period=0), "invalid '--max-period' (0). Needs to be 1 <= x <= 4096."),
                    (dict(max_period=4097), "invalid '--max-period' (4097). Needs to be 1 <= x <= 4096."),
                    (dict(min_copies=1), "invalid '--min-copies' (1). Needs to be 2 <= x <= 1024."),
                    (dict(min_copies=1025), "invalid '--min-copies' (1025). Needs to be 2 <= x <= 1024."),
                    (dict(min_span=1), "invalid '--min-span' (1). Needs to be 2 <= x <= 65535."),
                    (dict(min_span=65536), "invalid '--min-span' (65536). Needs to be 2 <= x <= 65535.")):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.repeats_files(vcf, bed, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and msg in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError, match="cannot open"):
        otter_amd.repeats_files(str(tmp_path / "missing.vcf"), bed)
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.repeats_files(vcf, str(tmp_path / "missing.bed"))
    exe = os.path.join(ROOT, "tools", "otter_repeats")
    for args, msg in ((["-p", "0"], b"invalid '--max-period' (0). Needs to be 1 <= x <= 4096."), (["-p", "4097"], b"invalid '--max-period' (4097)"),
                      (["--min-copies", "1"], b"invalid '--min-copies' (1). Needs to be 2 <= x <= 1024."), (["--min-copies=1025"], b"invalid '--min-copies' (1025)"),
                      (["--min-span", "1"], b"invalid '--min-span' (1). Needs to be 2 <= x <= 65535."), (["--min-span=65536"], b"invalid '--min-span' (65536)"),
                      (["--min-span=-1"], b"invalid '--min-span' (-1)"), (["-p", "x"], None)):
        r = subprocess.run([exe, "-b", bed] + args + [vcf], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout.count(b"\t") == 0, (args, r)
        assert msg is None or msg in r.stderr
    assert subprocess.run([exe, vcf], capture_output=True, timeout=60).returncode == 1           # no BED
    assert subprocess.run([exe, "-b", str(tmp_path / "missing.bed"), vcf], capture_output=True, timeout=60).returncode == 1
    r = subprocess.run([exe], capture_output=True, timeout=60)                                   # the usage text
    assert r.returncode == 0 and b"Usage:" in r.stdout and b"--min-copies" in r.stdout and b"--min-span" in r.stdout and b"--batch" in r.stdout


# ---------------------------------------------------------------------------------------------- 6: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(OTG_REPEAT_[A-Z_]+)\s+(\d+u?)", txt)}
    assert defs == {"OTG_REPEAT_MAX_PERIOD": abi.REPEAT_MAX_PERIOD, "OTG_REPEAT_MAX_LEN": abi.REPEAT_MAX_LEN, "OTG_REPEAT_TOO_LONG": abi.REPEAT_TOO_LONG,
                    "OTG_REPEAT_TEXT_LITERAL": abi.REPEAT_TEXT_LITERAL}
    assert (R.MAX_PERIOD, R.MAX_LEN, R.TOO_LONG, R.TEXT_LITERAL) == (abi.REPEAT_MAX_PERIOD, abi.REPEAT_MAX_LEN, abi.REPEAT_TOO_LONG, abi.REPEAT_TEXT_LITERAL)
    # step 4 stays inside 64 bits (g, w <= MAX_LEN + MAX_PERIOD); the planes are the motif annotation's
    assert (abi.REPEAT_MAX_LEN + abi.REPEAT_MAX_PERIOD) ** 2 < 2 ** 63 and (abi.REPEAT_MAX_LEN, abi.REPEAT_MAX_PERIOD) == (abi.MOTIF_MAX_LEN, abi.MOTIF_MAX_PERIOD)
    for name, dt in (("otg_repeat_seg", abi.repeat_seg_dt), ("otg_repeat_sum", abi.repeat_sum_dt)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
        assert re.findall(r"uint32_t\s+(\w+);", body) == list(dt.names)
    body = re.search(r"typedef struct otg_repeats_job \{(.*?)\} otg_repeats_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.RepeatsJob._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(otg_repeat_seg),'
                   'sizeof(otg_repeat_sum),sizeof(otg_repeats_job),offsetof(otg_repeats_job,batch_alleles));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.repeat_seg_dt.itemsize, abi.repeat_sum_dt.itemsize, C.sizeof(abi.RepeatsJob), abi.RepeatsJob.batch_alleles.offset]
    names = {"otg_repeat_batch", "otg_repeat_collect", "otg_repeat_device_results", "otg_repeat_last_ms", "otg_repeat_cohort", "otg_repeat_emit",
             "otg_repeats_files"}
    assert names <= set(otter_amd.EXPORTS) and {n for n in otter_amd.EXPORTS if n.startswith("otg_repeat")} == names
    lib = otter_amd.load()
    for n in names:
        assert getattr(lib, n) is not None

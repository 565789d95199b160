"""CPU: the joint unit parse without a device.

1. the eight records the rule was prototyped with as literals, through both forms of tests/unitparse_ref.py (the rule restated from
   include/otter_gpu.h);
2. step 1 of the rule as an independent witness: the enumerated language == the DP on 300 seeded tasks with L <= 4, K <= 2, p <= 3;
3. the invariants of step 4 on 300 seeded tasks with L <= 40, K <= 3; 4. K = 1 == tests/unitalign_ref.py;
5. the kernel's arithmetic and its backward walk (otter_amd/csrc/otg_unitparse_core.hpp) run on the host in the kernel's schedule by
   tests/unitparse_core_host.cpp, a stand-alone program built with -fsanitize=address,undefined, == unitparse_ref: every lane layout, the
   ballot words, unequal neighbours in a wave;
6. otg_unitparse_emit against rows formatted in Python; 7. the refusals that need no device and the tool's messages; 8. the ABI mirrors."""
import ctypes as C
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
import unitalign_ref as Ua
import unitparse_cases as Uc
import unitparse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


# ---------------------------------------------------------------------------------------------- 1: the rule on literals
def test_reference_on_the_prototype_table():
    assert len(Uc.TABLE) == 8
    for s, units, key, segs, end in Uc.TABLE:
        for f in (R.unitparse, R.unitparse_np):
            rec, got = f(s, units)
            assert rec[:3] == key and rec[4:6] == end and rec[3] == len(got) == key[1] + 1 and rec[6] == 0, (s, units)
            assert len(got) == segs if isinstance(segs, int) else got == segs, (s, units)
    assert R.unitparse(b"", [b"CAG"]) == ((0,) * 7, []) == R.unitparse_np(b"", [b"CAG", b"C"])
    for bad in ([], [b"A"] * 9, [b"A" * 257], [b""], [b"A" * 256, b"C"]):
        with pytest.raises(ValueError):
            R.unitparse(b"CAG", bad)
    R.check_units([b"A" * 252, b"C" * 4])                                  # 63 + 1 lanes at four positions each


# ---------------------------------------------------------------------------------------------- 2: the witness
def test_brute_force_witness_of_step_1():
    tasks = Uc.tiny_set()
    assert len(tasks) >= 300 and all(len(s) <= 4 and len(us) <= 2 and max(len(u) for u in us) <= 3 for s, us in tasks)
    assert sum(b"N" in s or any(b"N" in u for u in us) for s, us in tasks) > 100 and sum(len(us) == 2 for _, us in tasks) > 100
    for s, us in tasks:
        r = R.unitparse(s, us)
        assert r[0][:3] == R.unitparse_brute(s, us), (s, us)
        assert r == R.unitparse_np(s, us), (s, us)


# ---------------------------------------------------------------------------------------------- 3: the invariants of the segments
def test_invariants_of_the_segments():
    tasks = Uc.random_set()
    assert len(tasks) >= 300 and all(len(s) <= 40 and len(us) <= 4 for s, us in tasks)
    n_sw = n_ed = 0
    for s, us in tasks:
        rec, segs = R.unitparse(s, us)
        assert (rec, segs) == R.unitparse_np(s, us), (s, us)
        e, sw, ub, n, eu, ep, f = rec
        assert f == 0 and e <= len(s) and ub <= len(s) + e
        if not s:
            assert rec == (0,) * 7 and segs == []
            continue
        assert n == len(segs) == sw + 1 and eu < len(us) and ep < len(us[eu]) and segs[-1][0] == eu
        assert segs[0][1] == 0 and segs[-1][2] == len(s) and all(a[2] == b[1] for a, b in zip(segs, segs[1:]))      # they tile [0, L)
        assert all(a[0] != b[0] for a, b in zip(segs, segs[1:])) and all(g[5] == 0 for g in segs[1:]) and segs[0][5] < len(us[segs[0][0]])
        assert sum(g[3] for g in segs) == ub and sum(g[4] for g in segs) == e
        assert all((g[5] + g[3]) % len(us[g[0]]) == 0 for g in segs[:-1]) and (segs[-1][5] + segs[-1][3]) % len(us[eu]) == ep
        assert R.unitparse(s.lower(), [u.lower() for u in us]) == (rec, segs)
        n_sw += sw > 0; n_ed += e > 0
    assert n_sw > 60 and n_ed > 150


# ---------------------------------------------------------------------------------------------- 4: one unit
def test_one_unit_is_the_unit_alignment():
    n = 0
    for s, us in Uc.random_set(seed=10) + Uc.tiny_set(seed=6):
        rec, segs = R.unitparse(s, us[:1])
        assert (rec[0], rec[2], rec[5], 0) == Ua.unitalign(s, us[0]) and rec[1] == 0 and rec[4] == 0, (s, us[0])
        n += 1
    assert n >= 600


# ---------------------------------------------------------------------------------------------- 5: the kernel's arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("unitparse_core") / "unitparse_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "unitparse_core_host.cpp")])
    return exe


def _run(exe, tasks):
    """one batch -> per task ((record, segments), class)"""
    text = "batch %d\n" % len(tasks) + "".join("%s %d %s\n" % (s.hex() or "-", len(us), " ".join(u.hex() for u in us)) for s, us in tasks)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    rows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    assert len(rows) == len(tasks)
    return [((tuple(x[:7]), [tuple(x[8 + 6 * i:14 + 6 * i]) for i in range((len(x) - 8) // 6)]), x[7]) for x in rows]


def test_core_arithmetic_and_walk_against_the_rule(harness):
    tasks = [(s, us) for s, us, _, _, _ in Uc.TABLE] + Uc.layout_set() + Uc.random_set() + Uc.tiny_set(60) + Uc.shared_wave_set()
    got = _run(harness, tasks)
    for (s, us), (g, _) in zip(tasks, got):
        assert g == R.unitparse_np(s, us), (s[:60], [u[:40] for u in us])
    assert {c for (_, c), (s, _) in zip(got, tasks) if s} == set(range(7))      # every lane layout ran
    per = len(Uc.layout_set()) // len(Uc.LAYOUTS)
    want = {(4, 1): 0, (8, 1): 1, (16, 1): 2, (32, 1): 3, (64, 1): 4, (64, 2): 5, (64, 4): 6}
    for i, (_, lanes, regs) in enumerate(Uc.LAYOUTS):
        assert {c for (_, c), (s, _) in zip(got[8 + i * per:8 + (i + 1) * per], tasks[8 + i * per:8 + (i + 1) * per]) if s} == {want[lanes, regs]}


def test_short_tasks_agree_with_the_plain_reference():
    n = 0
    for s, us in Uc.layout_set() + Uc.shared_wave_set():
        if sum(len(u) for u in us) <= 16 and len(s) <= 64:
            assert R.unitparse(s, us) == R.unitparse_np(s, us), (s, us)
            n += 1
    assert n > 60


# ---------------------------------------------------------------------------------------------- 6: the row text
def test_emit_against_python_rows():
    sets = [[b"CAG", b"CCG"], [b"gaa", b"AGAA"], [b"A"]]
    seqs = [b"CAG" * 10 + b"T" + b"CAG" * 10 + b"CCG" * 7, b"cag" * 20, b"", b"GAA" * 31 + b"AGAA" * 5 + b"GAA" * 10 + b"GA", b"ACGT", b"A" * 40, b"GATTACA"]
    aset = [0, 0, 0, 1, None, 2, None]
    regions = [b"chr1:100-160", b"", b"chrUn_x:5-9"]
    first, n_al = [0, 3, 5], [3, 2, 2]
    records = np.zeros(3, dtype=abi.vcf_record_dt)
    pos = 0
    for r in range(3):
        records[r] = (pos, len(regions[r]), first[r], n_al[r], 0)
        pos += len(regions[r])
    res = [R.unitparse(s, sets[q]) if q is not None else ((0,) * 7, []) for s, q in zip(seqs, aset)]
    res[5] = ((0, 0, 0, 0, 0, 0, R.TOO_LONG), [])                          # a flagged row
    sums = np.array([r[0] + (0,) for r in res], dtype=abi.unitparse_sum_dt)
    seg_off = np.cumsum([0] + [len(r[1]) for r in res]).astype(np.uint64)
    segs = np.array([g for r in res for g in r[1]], dtype=abi.unitparse_seg_dt)
    text = otter_amd.unitparse_emit(records, b"".join(regions), [len(s) for s in seqs], aset, sets, sums, seg_off, segs)
    want = b"".join(R.row(regions[r], i, len(seqs[first[r] + i]), sets[aset[first[r] + i]] if aset[first[r] + i] is not None else [], *res[first[r] + i])
                    for r in range(3) for i in range(n_al[r]))
    assert text == want
    lines = want.split(b"\n")
    assert lines[0] == b"chr1:100-160\t0\t82\tCAG,CCG\t1\t1\t81\t0.9878\t20.00,7.00\t(CAG)20~1(CCG)7"
    assert lines[1] == b"chr1:100-160\t1\t60\tCAG,CCG\t0\t0\t60\t1.0000\t20.00,0.00\t(CAG)20"
    assert lines[2] == b"chr1:100-160\t2\t0\tCAG,CCG\t0\t0\t0\t0.0000\t0.00,0.00\t."
    assert lines[3] == b"\t0\t145\tgaa,AGAA\t0\t2\t145\t1.0000\t41.67,5.00\t(gaa)31(AGAA)5(gaa)10.67"
    assert lines[4] == b"\t1\t4\t.\t0\t0\t0\t0.0000\t.\t." and lines[5] == b"chrUn_x:5-9\t0\t40\tA\t0\t0\t0\t0.0000\t0.00\t." and len(lines) == 8
    assert otter_amd.unitparse_emit(records[:0], b"", [], [], [], sums[:0], [0], segs[:0]) == b""
    # the buffer protocol: the length without a buffer, a buffer one byte short
    L = otter_amd.load()
    reg = np.frombuffer(b"".join(regions) + b"\0", dtype=np.uint8)
    ln = np.array([len(s) for s in seqs], dtype=np.uint32)
    qa = np.array([abi.UNITPARSE_NO_SET if q is None else q for q in aset], dtype=np.uint32)
    flat = [u for q in sets for u in q]
    ulen = np.array([len(u) for u in flat], dtype=np.uint32)
    uoff = (np.cumsum(ulen) - ulen).astype(np.uint64)
    uar = np.frombuffer(b"".join(flat), dtype=np.uint8)
    sf = np.array([0, 2, 4, 5], dtype=np.uint64)
    need = C.c_uint64(0)
    args = lambda out, cap, g=segs: (abi.ptr(records), C.c_uint32(3), abi.ptr(reg), abi.ptr(ln), abi.ptr(qa), abi.ptr(sf), abi.ptr(uar), abi.ptr(uoff), abi.ptr(ulen),
                                     abi.ptr(sums), abi.ptr(seg_off), abi.ptr(g), out, C.c_uint64(cap), C.byref(need))
    assert L.otg_unitparse_emit(*args(None, 0)) == abi.OTG_ERR_CAPACITY and need.value == len(want)
    buf = C.create_string_buffer(len(want))
    assert L.otg_unitparse_emit(*args(buf, len(want) - 1)) == abi.OTG_ERR_CAPACITY
    assert L.otg_unitparse_emit(*args(buf, len(want))) == 0 and buf.raw == want
    bad = segs.copy()
    bad[0]["unit"] = 2                                                     # a unit outside the allele's set
    assert L.otg_unitparse_emit(*args(buf, len(want), bad)) == abi.OTG_ERR_ARG and b"names unit 2 of 2" in L.otg_last_error(None)


# ---------------------------------------------------------------------------------------------- 7: refusals without a device
def test_refusals_without_a_device(tmp_path):
    L = otter_amd.load()
    u, u64 = C.c_uint32, C.c_uint64
    one = np.zeros(1, dtype=np.uint32)
    assert L.otg_unitparse_batch(None, None, u64(0), None, None, u(0), None, u64(0), None, None, u(0), None, u(0), None, None, u(0), None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_unitparse_cohort(None, u(0), u(0), None, u64(0), None, None, u(0), None, u(0), None, None, u(0), None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_unitparse_collect(None, None, u64(0)) == abi.OTG_ERR_ARG
    assert L.otg_unitparse_device_results(None, abi.ptr(one), None, None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_unitparse_last_ms(None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_unitparse_emit(None, u(0), None, None, None, None, None, None, None, None, None, None, None, u64(0), None) == abi.OTG_ERR_ARG
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\tCAG,CCG\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    with pytest.raises(otter_amd.OtterGpuError, match="cannot open"):
        otter_amd.unitparse_files(vcf, str(tmp_path / "missing.bed"))
    fn = L.otg_unitparse_files
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(None, None, None, None) == abi.OTG_ERR_ARG and b"otg_unitparse_files: NULL job, writer, VCF or BED path" in L.otg_last_error(None)
    exe = os.path.join(ROOT, "tools", "otter_unitparse")
    for args, msg in ((["-t", "x"], b"invalid integer argument"), (["--batch=-1"], b"invalid integer argument"), (["--batch"], b"Option 'batch' is missing an argument")):
        r = subprocess.run([exe, "-b", bed] + args + ([vcf] if len(args) != 1 or "=" in args[0] else []), capture_output=True, timeout=60)
        assert r.returncode == 1 and msg in r.stdout and r.stdout.count(b"\t") == 0, (args, r)
    r = subprocess.run([exe, vcf], capture_output=True, timeout=60)           # no BED
    assert r.returncode == 1 and b"Option 'bed' has no value" in r.stdout
    r = subprocess.run([exe, "-b", str(tmp_path / "missing.bed"), vcf], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"otter_unitparse: " in r.stderr
    r = subprocess.run([exe], capture_output=True, timeout=60)                # the usage text
    assert r.returncode == 0 and b"Usage:" in r.stdout and b"--bed" in r.stdout and b"--threads" in r.stdout and b"--batch" in r.stdout


# ---------------------------------------------------------------------------------------------- 8: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: v for k, v in re.findall(r"#define\s+(OTG_UNITPARSE_[A-Z_0-9]+)\s+(.+?)\s*(?:/\*|$)", txt, flags=re.M)}
    assert set(defs) == {"OTG_UNITPARSE_MAX_UNITS", "OTG_UNITPARSE_MAX_LANES", "OTG_UNITPARSE_MAX_LEN", "OTG_UNITPARSE_TOO_LONG", "OTG_UNITPARSE_NO_SET"}
    assert (int(defs["OTG_UNITPARSE_MAX_UNITS"]), int(defs["OTG_UNITPARSE_MAX_LANES"]), int(defs["OTG_UNITPARSE_TOO_LONG"].rstrip("u"))) \
        == (abi.UNITPARSE_MAX_UNITS, abi.UNITPARSE_MAX_LANES, abi.UNITPARSE_TOO_LONG) == (R.MAX_UNITS, R.MAX_LANES, R.TOO_LONG) == (8, 64, 1)
    assert int(defs["OTG_UNITPARSE_NO_SET"].rstrip("u"), 16) == abi.UNITPARSE_NO_SET
    # the bound of the key: the largest low field a lane can hold, 2 (L - 1) + 2 p, stays under 2^21 - 1 at the bound and not one base above it
    N, P = abi.UNITPARSE_MAX_LEN, abi.UNITALIGN_MAX_UNIT
    assert N == R.MAX_LEN == 1048320 >= 262143 and 2 * (N - 1) + 2 * P < 2 ** 21 - 1 <= 2 * N + 2 * P and N + 2 * P < 2 ** 22
    assert (R.E, R.SW, R.W) == (1 << 42, 1 << 21, (1 << 42) + 1)
    for name, dt in (("otg_unitparse_sum", abi.unitparse_sum_dt), ("otg_unitparse_seg", abi.unitparse_seg_dt)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
        assert re.findall(r"uint32_t\s+(\w+);", body) == list(dt.names)
    body = re.search(r"typedef struct otg_unitparse_job \{(.*?)\} otg_unitparse_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.UnitparseJob._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu %d\\n",sizeof(otg_unitparse_sum),'
                   'sizeof(otg_unitparse_seg),sizeof(otg_unitparse_job),offsetof(otg_unitparse_job,batch_alleles),OTG_UNITPARSE_MAX_LEN);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.unitparse_sum_dt.itemsize, abi.unitparse_seg_dt.itemsize, C.sizeof(abi.UnitparseJob), abi.UnitparseJob.batch_alleles.offset, abi.UNITPARSE_MAX_LEN]
    names = {"otg_unitparse_batch", "otg_unitparse_collect", "otg_unitparse_device_results", "otg_unitparse_last_ms", "otg_unitparse_cohort", "otg_unitparse_emit",
             "otg_unitparse_files"}
    assert {n for n in otter_amd.EXPORTS if n.startswith("otg_unitparse")} == names
    lib = otter_amd.load()
    for n in names:
        assert getattr(lib, n) is not None

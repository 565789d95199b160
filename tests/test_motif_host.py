"""CPU: the tandem-repeat motif annotation without a device.

1. tests/motif_ref.py (the rule restated from include/otter_gpu.h) on hand-derived literals;
2. the kernels' arithmetic (otter_amd/csrc/otg_motif_core.hpp: bit-planes, shifted compares, the orders of the two reductions) run on the host
   in the kernels' schedule by tests/motif_core_host.cpp, a stand-alone program built with -fsanitize=address,undefined, == motif_ref on the
   edge and random sets the GPU test uses;
3. otg_motif_emit against rows formatted in Python; 4. the refusals that need no device; 5. the ABI mirrors."""
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
import motif_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


# ---------------------------------------------------------------------------------------------- 1: the rule on literals
def _m(seq, **kw):
    r = R.motif(seq, **kw)
    return r["period"], r["unit"], r["matches"], r["compared"], r["best_period"]


def test_reference_on_hand_derived_literals():
    assert _m(b"CAG" * 20) == (3, b"AGC", 57, 57, 3)
    # one substitution: the window of p = 30 avoids the mismatch twice (29 / 30 against 55 / 57), the slack brings 3 back
    assert _m(b"CAG" * 10 + b"CTG" + b"CAG" * 9) == (3, b"AGC", 55, 57, 30)
    assert _m(b"CAG" * 10 + b"CTG" + b"CAG" * 9, slack=0)[0] == 30
    assert _m(b"CAG" * 10 + b"CTG" + b"CAG" * 9, slack=999)[0] == 3
    assert _m(b"CAG" * 20 + b"CCG" * 20) == (3, b"AGC", 116, 117, 3)       # A and C tie in phase 1: the lower code
    assert _m(b"A" * 30)[:4] == (1, b"A", 29, 29)
    assert _m(b"AAAG" * 25)[:2] == (4, b"AAAG")
    assert _m(b"ACAC") == (2, b"AC", 2, 2, 2)
    for s in (b"AC", b"A", b"", b"N" * 20):
        assert R.motif(s) == dict(period=0, matches=0, compared=0, best_period=0, flags=0, unit=b"")
    for s in Cs.LITERALS:
        assert R.motif(s.lower()) == R.motif(s)
    assert _m(b"ANGTANGTANGT")[:2] == (4, b"ANGT")                         # a phase without an ACGT byte; N sorts between G and T
    assert _m(b"CAG" * 20, max_period=2)[0] == 0                           # max_period below the true period: CAG has no match at 1 or 2
    assert _m(b"AAAG" * 25, max_period=3) == (1, b"A", 50, 99, 1)          # 50 / 99 at 1 against 49 / 98 at 2 and 48 / 97 at 3
    long = R.motif(b"A" * (R.MAX_LEN + 1))
    assert long == dict(period=0, matches=0, compared=0, best_period=0, flags=R.TOO_LONG, unit=b"")


# ---------------------------------------------------------------------------------------------- 2: the kernels' arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("motif_core") / "motif_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "motif_core_host.cpp")])
    return exe


def _run(exe, cases):
    """cases: (seq, max_period, slack) -> the harness's results in motif_ref's form"""
    text = "".join("%d %d %s\n" % (mp, sl, seq.hex() or "-") for seq, mp, sl in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    out = []
    for l in r.stdout.splitlines():
        f = l.split()
        out.append(dict(period=int(f[0]), matches=int(f[1]), compared=int(f[2]), best_period=int(f[3]), flags=int(f[4]),
                        unit=b"" if f[5] == "-" else bytes.fromhex(f[5])))
    assert len(out) == len(cases)
    return out


def test_core_arithmetic_against_the_rule(harness):
    cases = [(s, 256, 50) for s in Cs.edge_set() + Cs.random_set()]
    cases += [(s, mp, 50) for s in Cs.edge_set()[::3] for mp in (1, 2, 63, 64, 65)]
    cases += [(s, 256, sl) for s in Cs.edge_set()[::2] for sl in (0, 999)]
    rng = np.random.default_rng(3)
    unit = Cs.rs(rng, 300)
    cases += [(unit * 4, 4096, 50), (unit * 4, 299, 50), (Cs.substitute(rng, Cs.rs(rng, 700) * 3, 5), 4096, 50)]      # periods beyond one workgroup's threads
    got = _run(harness, cases)
    for (seq, mp, sl), g in zip(cases, got):
        assert g == R.motif_cached(seq, mp, sl), (seq, mp, sl)
    assert sum(g["period"] > 256 for g in got) >= 2 and sum(g["period"] != g["best_period"] for g in got) > 5


# ---------------------------------------------------------------------------------------------- 3: the row text
def test_emit_against_python_rows():
    seqs = [b"CAG" * 20, b"CAG" * 10 + b"CTG" + b"CAG" * 9, b"AC", b"", b"AAAG" * 25 + b"A", b"N" * 9, b"ACGTTGCA" * 3 + b"ACG"]
    exp = [R.motif(s) for s in seqs]
    stride = 8
    rec = np.zeros(len(seqs), dtype=abi.motif_dt)
    units = np.zeros((len(seqs), stride), dtype=np.uint8)
    for i, e in enumerate(exp):
        for k in ("period", "matches", "compared", "best_period", "flags"):
            rec[i][k] = e[k]
        units[i, :e["period"]] = np.frombuffer(e["unit"], dtype=np.uint8)
    regions = [b"chr1:100-150", b"", b"chrUn_x:5-9"]
    records = np.zeros(3, dtype=abi.vcf_record_dt)
    first = [0, 3, 4]
    n_al = [3, 1, 3]
    pos = 0
    for r in range(3):
        records[r] = (pos, len(regions[r]), first[r], n_al[r], 0)
        pos += len(regions[r])
    text = otter_amd.motif_emit(records, b"".join(regions), [len(s) for s in seqs], rec, units)
    want = b"".join(R.row(regions[r], i, seqs[first[r] + i], exp[first[r] + i]) for r in range(3) for i in range(n_al[r]))
    assert text == want
    assert want.split(b"\n")[0] == b"chr1:100-150\t0\t60\t3\tAGC\t20.00\t1.0000" and b"\t2\t2\t0\t.\t0.00\t0.0000\n" in want
    assert otter_amd.motif_emit(records[:0], b"", [], rec[:0], units[:0]) == b""
    rec[0]["period"] = stride + 1                                          # a unit that cannot lie in its slot
    with pytest.raises(otter_amd.OtterGpuError, match="unit_stride"):
        otter_amd.motif_emit(records, b"".join(regions), [len(s) for s in seqs], rec, units)


# ---------------------------------------------------------------------------------------------- 4: refusals without a device
def test_refusals_without_a_device(tmp_path):
    L = otter_amd.load()
    one = np.zeros(1, dtype=np.uint32)
    assert L.otg_motif_batch(None, None, C.c_uint64(0), None, None, C.c_uint32(1), C.c_uint32(256), C.c_uint32(50), None, None, C.c_uint32(0)) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_motif_cohort(None, C.c_uint32(0), C.c_uint32(0), C.c_uint32(256), C.c_uint32(50), None, None, C.c_uint32(0)) == abi.OTG_ERR_NO_DEVICE
    assert L.otg_motif_device_results(None, abi.ptr(one), None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_motif_last_ms(None, None, None) == abi.OTG_ERR_ARG
    assert L.otg_motif_emit(None, C.c_uint32(0), None, None, None, None, C.c_uint32(0), None, C.c_uint64(0), None) == abi.OTG_ERR_ARG
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    for kw, msg in ((dict(max_period=0), "invalid '--max-period' (0). Needs to be 1 <= x <= 4096."),
                    (dict(max_period=4097), "invalid '--max-period' (4097). Needs to be 1 <= x <= 4096."),
                    (dict(slack=1000), "invalid '--slack' (1000). Needs to be 0 <= x <= 999.")):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.motifs_files(vcf, bed, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and msg in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError, match="cannot open"):
        otter_amd.motifs_files(str(tmp_path / "missing.vcf"), bed)
    exe = os.path.join(ROOT, "tools", "otter_motifs")
    for args, msg in ((["-p", "0"], b"invalid '--max-period' (0)"), (["-p", "4097"], b"invalid '--max-period' (4097)"), (["--slack", "1000"], b"invalid '--slack' (1000)"),
                      (["--slack=-1"], b"invalid '--slack' (-1)"), (["-p", "x"], None)):
        r = subprocess.run([exe, "-b", bed] + args + [vcf], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout.count(b"\t") == 0, (args, r)
        assert msg is None or msg in r.stderr
    assert subprocess.run([exe, vcf], capture_output=True, timeout=60).returncode == 1           # no BED
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 0                # the usage text


# ---------------------------------------------------------------------------------------------- 5: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define\s+(OTG_MOTIF_[A-Z_]+)\s+(\d+u?)", txt)}
    assert defs == {"OTG_MOTIF_MAX_PERIOD": abi.MOTIF_MAX_PERIOD, "OTG_MOTIF_MAX_LEN": abi.MOTIF_MAX_LEN, "OTG_MOTIF_LDS_LEN": abi.MOTIF_LDS_LEN,
                    "OTG_MOTIF_TOO_LONG": abi.MOTIF_TOO_LONG}
    assert (R.MAX_PERIOD, R.MAX_LEN, R.TOO_LONG) == (abi.MOTIF_MAX_PERIOD, abi.MOTIF_MAX_LEN, abi.MOTIF_TOO_LONG)
    # step 5 stays inside 64 bits: m, L - p <= MAX_LEN
    assert abi.MOTIF_MAX_LEN ** 2 * 1000 < 2 ** 63 and abi.MOTIF_LDS_LEN % 32 == 0
    body = re.search(r"typedef struct otg_motif \{(.*?)\} otg_motif;", txt, flags=re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == list(abi.motif_dt.names)
    body = re.search(r"typedef struct otg_motifs_job \{(.*?)\} otg_motifs_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.MotifsJob._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(otg_motif),'
                   'sizeof(otg_motifs_job),offsetof(otg_motifs_job,batch_alleles));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.motif_dt.itemsize, C.sizeof(abi.MotifsJob), abi.MotifsJob.batch_alleles.offset]
    names = {"otg_motif_batch", "otg_motif_device_results", "otg_motif_last_ms", "otg_motif_cohort", "otg_motif_emit", "otg_motifs_files"}
    assert names <= set(otter_amd.EXPORTS) and {n for n in otter_amd.EXPORTS if n.startswith("otg_motif")} == names
    lib = otter_amd.load()
    for n in names:
        assert getattr(lib, n) is not None

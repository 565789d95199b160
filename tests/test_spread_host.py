"""CPU: the spread operator (per-read copy numbers behind each consensus allele) without a device.

1. the two forms of the statistics in tests/spread_ref.py (by counting, and sorted() with indexing) agree on random member sets, and the
   quantile indices are the stated ones for m = 1..9;
2. the consequences the header states, on synthetic read records through spread_ref;
3. the selection routine of otter_amd/csrc/otg_spread_core.hpp run on the host in the kernel's schedule by tests/spread_core_host.cpp, a
   stand-alone program built with -fsanitize=address,undefined, == std::sort: both tiers, the member counts around every boundary;
4. otg_spread_emit against rows formatted in Python; 5. the ABI mirrors and the refusal that needs no device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
import spread_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


# ---------------------------------------------------------------------------------------------- 1: the statistics, twice
def test_two_forms_agree_on_random_member_sets():
    rng = np.random.default_rng(5)
    assert S.quantiles_sorted([]) == S.quantiles_count([]) == [0] * 5
    for trial in range(400):
        m = int(rng.integers(1, 70))
        hi = int(rng.choice([3, 40, 70000, 2 ** 21 - 1]))
        v = [int(x) for x in rng.integers(0, hi + 1, m)]
        a, b = S.quantiles_sorted(v), S.quantiles_count(v)
        assert a == b, (v, a, b)
        assert a == sorted(a) and a[0] == min(v) and a[4] == max(v)


def test_quantile_indices():
    want = {1: [0, 0, 0, 0, 0], 2: [0, 0, 0, 0, 1], 3: [0, 0, 1, 1, 2], 4: [0, 0, 1, 2, 3], 5: [0, 1, 2, 3, 4], 6: [0, 1, 2, 3, 5], 7: [0, 1, 3, 4, 6],
            8: [0, 1, 3, 5, 7], 9: [0, 2, 4, 6, 8]}
    for m in range(1, 10):
        assert [S.rank(j, m) for j in range(5)] == want[m] == [j * (m - 1) // 4 for j in range(5)]
        v = list(range(100, 100 + m))
        assert S.quantiles_sorted(v) == [v[i] for i in want[m]] == S.quantiles_count(v)


# ---------------------------------------------------------------------------------------------- 2: the consequences of the rule
def _batch(rows, labels, spans, consensus, region_of_read, n_regions):
    """a resident batch by hand: rows = the reads' bytes, consensus = [(region, label, bytes)] -> (arena, reads, res, regions)"""
    arena = np.frombuffer(b"".join(rows) + b"\0" * 64, dtype=np.uint8)
    reads = np.zeros(len(rows), dtype=abi.spread_read_dt)
    off = 0
    for i, s in enumerate(rows):
        reads[i] = (off, len(s), labels[i], 0, abi.SPREAD_NONE)
        off += len(s)
    regions = np.zeros(n_regions, dtype=abi.region_dt)
    for r in range(n_regions):
        mine = [i for i in range(len(rows)) if region_of_read[i] == r]
        regions[r]["first_read"] = mine[0] if mine else 0
        regions[r]["n_reads"] = len(mine)
    res = {"regions": np.zeros(n_regions, dtype=abi.region_result_dt), "alleles": np.zeros(len(consensus), dtype=abi.allele_dt),
           "seqs": np.frombuffer(b"".join(c[2] for c in consensus) + b"\0", dtype=np.uint8)}
    off = 0
    for a, (r, lab, s) in enumerate(consensus):
        res["alleles"][a]["seq_off"] = off; res["alleles"][a]["seq_len"] = len(s); res["alleles"][a]["region"] = r; res["alleles"][a]["label"] = lab
        off += len(s)
    for r in range(n_regions):
        mine = [a for a, c in enumerate(consensus) if c[0] == r]
        res["regions"][r]["first_allele"] = mine[0] if mine else 0
        res["regions"][r]["n_alleles"] = len(mine)
    t = 0
    for i in range(len(rows)):
        if labels[i] >= 0 and spans[i]:
            reads[i]["counted"] = 1; reads[i]["task"] = t
            t += 1
    return arena, reads, res, regions


def _flanked(rng, body):
    f = lambda n: bytes(b"TA"[int(x)] for x in rng.integers(0, 2, n))      # (neither base extends a CAG / CCG tract across the T next to it)
    return f(24) + b"T" + body + b"T" + f(24)


def test_consequences_of_the_rule():
    rng = np.random.default_rng(9)
    copies = [18, 20, 20, 21, 25, 20, 19]
    rows = [_flanked(rng, b"CAG" * c) for c in copies] + [_flanked(rng, b"CAG" * 30 + b"CCG" * c) for c in (8, 9, 12)] + [_flanked(rng, b"")]
    labels = [0, 0, 0, 0, 0, -1, 0] + [0, 0, 0] + [0]
    spans = [1, 1, 1, 1, 1, 1, 0] + [1, 1, 1] + [1]
    region_of = [0] * 7 + [1] * 3 + [2]
    cons = [(0, 0, _flanked(rng, b"CAG" * 20)), (1, 0, _flanked(rng, b"CAG" * 30 + b"CCG" * 9)), (2, 0, _flanked(rng, b""))]
    arena, reads, res, regions = _batch(rows, labels, spans, cons, region_of, 3)
    sets = [[b"CAG"], [b"CAG", b"CCG"]]
    rec, uoff, units, rr = S.spread(arena, reads, res, regions, [0, 1, 0], sets)
    both = S.spread(arena, reads, res, regions, [0, 1, 0], sets, quantiles=S.quantiles_count)
    assert rec.tobytes() == both[0].tobytes() and units.tobytes() == both[2].tobytes()
    # region 0: five counted reads (one unlabelled, one not spanning), one unit: the unit record is the total
    assert (rec[0]["n_reads"], rec[0]["n_called"], rec[0]["ref_bases"], rec[0]["flags"]) == (5, 5, 60, 0)
    assert list(rec[0]["q"]) == [54, 60, 60, 63, 75] and (rec[0]["n_below"], rec[0]["n_above"], rec[0]["sum_below"], rec[0]["sum_above"]) == (1, 2, 6, 18)
    assert list(uoff) == [0, 1, 3, 4] and units[0]["ref_bases"] == 60 and list(units[0]["q"]) == list(rec[0]["q"])
    # region 1: two units, each series on its own
    assert list(units[1]["q"]) == [90] * 5 and list(units[2]["q"]) == [24, 24, 27, 27, 36] and (units[1]["ref_bases"], units[2]["ref_bases"]) == (90, 27)
    assert list(rec[1]["q"]) == [114, 114, 117, 117, 126]
    # region 2: random sequence: counted, none called, no reference tract
    assert (rec[2]["n_reads"], rec[2]["n_called"], rec[2]["flags"]) == (1, 0, abi.SPREAD_NO_CALLS | abi.SPREAD_REF_NONE) and not rec[2]["q"].any()
    for r in rec:
        assert list(r["q"]) == sorted(r["q"]) and r["n_below"] + r["n_above"] <= r["n_called"] <= r["n_reads"] and r["reserved"] == 0
    # letter case changes nothing; a region without a set
    lower = np.frombuffer(arena.tobytes().lower(), dtype=np.uint8)
    assert S.spread(lower, reads, res, regions, [0, 1, 0], sets)[0].tobytes() == rec.tobytes()
    none = S.spread(arena, reads, res, regions, [0, None, 0], sets)
    assert none[0][1]["flags"] == abi.SPREAD_NO_SET and not none[0][1]["q"].any() and none[0][1]["n_reads"] == 0 and list(none[1]) == [0, 1, 1, 2]
    # identical members
    rows2 = [rows[1]] * 6
    a2 = _batch(rows2, [0] * 6, [1] * 6, [(0, 0, rows[1])], [0] * 6, 1)
    r2 = S.spread(*a2, [0], sets)[0][0]
    assert list(r2["q"]) == [60] * 5 and (r2["n_below"], r2["n_above"], r2["sum_below"], r2["sum_above"], r2["ref_bases"]) == (0, 0, 0, 0, 60)


# ---------------------------------------------------------------------------------------------- 3: the kernel's selection on the host
def test_selection_routine_against_sort(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the sanitized run of the selection routine cannot be skipped"
    exe = str(tmp_path / "spread_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "spread_core_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    ok, n_reg, n_load = r.stdout.split()
    assert ok == "ok" and int(n_load) == 12 * 3 * 5 and 0 < int(n_reg) < int(n_load)
    core = open(os.path.join(ROOT, "otter_amd", "csrc", "otg_spread_core.hpp")).read()
    assert re.search(r"SP_BITS = (\d+);", core).group(1) == "21" and 2 * abi.LOCUS_MAX_LEN < 2 ** 21
    assert re.search(r"SP_REG_STRIDES = (\d+);", core).group(1) == "4"


# ---------------------------------------------------------------------------------------------- 4: the row text
def test_emit_against_python_rows():
    regions = [("chr1", 100, 160), ("chr2", 5, 50), ("chrX", 7, 9), ("chr3", 1, 2)]
    beds, carena = abi.make_beds(regions)
    res = {"regions": np.zeros(4, dtype=abi.region_result_dt), "alleles": np.zeros(4, dtype=abi.allele_dt), "seqs": np.zeros(1, dtype=np.uint8)}
    res["regions"]["first_allele"] = [0, 2, 3, 3]
    res["regions"]["n_alleles"] = [2, 1, 0, 1]
    res["alleles"]["label"] = [0, 1, 0, 0]
    res["alleles"]["seq_len"] = [130, 141, 77, 60]
    res["alleles"]["region"] = [0, 0, 1, 3]
    sets = [[b"CAG", b"CCG"], [b"AAAAG"]]
    region_set = [0, None, 1, 1]
    rec = np.zeros(4, dtype=abi.spread_dt)
    rec[0] = (30, 29, 120, [100, 117, 120, 121, 400], 9, 12, 77, 2 ** 33 + 5, 0, 0)
    rec[1] = (2, 0, 0, [0] * 5, 0, 0, 0, 0, abi.SPREAD_NO_CALLS | abi.SPREAD_REF_NONE, 0)
    rec[2]["flags"] = abi.SPREAD_NO_SET
    rec[3] = (7, 7, 52, [50, 50, 51, 53, 58], 3, 2, 4, 7, 0, 0)
    unit_off = np.array([0, 2, 4, 4, 5], dtype=np.uint64)
    units = np.zeros(5, dtype=abi.spread_unit_dt)
    units[0] = (90, [70, 88, 90, 91, 370]); units[1] = (30, [29, 29, 30, 31, 32]); units[4] = (52, [50, 50, 51, 53, 58])
    text = otter_amd.spread_emit(beds, carena, res, region_set, sets, rec, unit_off, units)
    want = S.row(b"chr1:100-160", 0, 130, sets[0], rec[0], units[0:2]) + S.row(b"chr1:100-160", 1, 141, sets[0], rec[1], units[2:4]) + \
        S.row(b"chr2:5-50", 0, 77, None, rec[2], []) + S.row(b"chr3:1-2", 0, 60, sets[1], rec[3], units[4:5])
    assert text == want
    assert want.splitlines()[0] == b"chr1:100-160\t0\t130\tCAG,CCG\t30\t29\t120\t100\t117\t120\t121\t400\t9\t12\t77\t8589934597\t" \
        b"CAG:30.00:23.33/29.33/30.00/30.33/123.33,CCG:10.00:9.67/9.67/10.00/10.33/10.67"
    assert want.splitlines()[2] == b"chr2:5-50\t0\t77\t.\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t."
    # an allele whose unit records do not match its set is refused
    bad = unit_off.copy(); bad[1] = 1
    with pytest.raises(otter_amd.OtterGpuError, match="unit records"):
        otter_amd.spread_emit(beds, carena, res, region_set, sets, rec, bad, units)


# ---------------------------------------------------------------------------------------------- 5: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: v for k, v in re.findall(r"#define\s+(OTG_SPREAD_[A-Z_0-9]+)\s+(\S+)", txt)}
    assert {k: int(v.rstrip("u"), 0) for k, v in defs.items()} == {"OTG_SPREAD_NONE": abi.SPREAD_NONE, "OTG_SPREAD_NO_SET": abi.SPREAD_NO_SET,
                                                                    "OTG_SPREAD_NO_CALLS": abi.SPREAD_NO_CALLS, "OTG_SPREAD_REF_NONE": abi.SPREAD_REF_NONE}
    for name, dt in (("otg_spread", abi.spread_dt), ("otg_spread_unit", abi.spread_unit_dt), ("otg_spread_read", abi.spread_read_dt)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
        assert re.findall(r"(\w+)(?:\[5\])?;", body) == list(dt.names), name
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",sizeof(otg_spread),'
                   'offsetof(otg_spread,q),offsetof(otg_spread,n_below),offsetof(otg_spread,sum_below),offsetof(otg_spread,sum_above),offsetof(otg_spread,flags),'
                   'sizeof(otg_spread_unit),offsetof(otg_spread_unit,q),sizeof(otg_spread_read),offsetof(otg_spread_read,label),offsetof(otg_spread_read,task));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    f, u, r = abi.spread_dt.fields, abi.spread_unit_dt.fields, abi.spread_read_dt.fields
    assert got == [abi.spread_dt.itemsize, f["q"][1], f["n_below"][1], f["sum_below"][1], f["sum_above"][1], f["flags"][1], abi.spread_unit_dt.itemsize, u["q"][1],
                   abi.spread_read_dt.itemsize, r["label"][1], r["task"][1]]
    assert got[0] == 64 and got[6] == 24 and got[8] == 24
    names = {"otg_assemble_spread", "otg_spread_collect", "otg_spread_collect_reads", "otg_spread_device_results", "otg_spread_last_ms", "otg_spread_emit", "otg_spread_files"}
    assert {n for n in otter_amd.EXPORTS if "spread" in n} == names
    lib = otter_amd.load()
    for n in names:
        assert getattr(lib, n) is not None
    for fn in ("assemble_spread", "spread_last_ms", "locus_last"):
        assert callable(getattr(otter_amd.Context, fn))
    assert callable(otter_amd.spread_files) and callable(otter_amd.spread_emit)
    body = re.search(r"typedef struct otg_spread_job \{(.*?)\} otg_spread_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.SpreadJob._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(otg_spread_job),'
                   'offsetof(otg_spread_job,match),offsetof(otg_spread_job,min_score));return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(abi.SpreadJob), abi.SpreadJob.match.offset, abi.SpreadJob.min_score.offset]
    # without a context the operator refuses with a message
    rc = lib.otg_assemble_spread(None, None, C.c_uint64(0), None, None, C.c_uint32(0), None, C.c_uint32(0), None, C.c_uint32(0), None, None, None, None)
    assert rc == abi.OTG_ERR_NO_DEVICE and b"otg_assemble_spread" in lib.otg_last_error(None)

"""CPU: the unit-set discovery (the repeat units of a region from the repeat structure of its alleles) without a device.

1. the seven prototype groups of the rule through both forms of tests/unitset_ref.py (the rule restated from include/otter_gpu.h), and the
   locus mode with the discovered set against the recorded rows;
2. the two forms against each other on random groups, the smallest rotation against a witness that sorts every rotation, and the
   properties that follow from the rule: the order of the segments, a permutation of the alleles, a rotation of every copy;
3. recovery: planted loci at three error rates, at least 190 of 200 each;
4. the kernels' arithmetic (otter_amd/csrc/otg_unitset_core.hpp) run on the host in the kernels' schedule by tests/unitset_core_host.cpp, a
   stand-alone program built with -fsanitize=address,undefined, == unitset_ref: both table sizes, truncated hashes (the compare on a hash
   match decides), shuffled insertion orders, the class cap;
5. otg_unitset_emit against rows formatted in Python, and the emitted catalogue read back by otg_parse_bed_units;
6. the refusals that need no device; 7. the ABI mirrors."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
import locus_ref as L
import repeat_ref as Rp
import unitset_cases as Uc
import unitset_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")


def _triples(res):
    return [u[:3] for u in res["units"]]


# ---------------------------------------------------------------------------------------------- 1: the rule on the prototype rows
def test_reference_on_the_prototype_rows():
    assert sorted(Uc.PROTOTYPES) == list("ABCDEFG")
    for name, (alleles, units, n_classes, loci) in Uc.PROTOTYPES.items():
        for f in (S.unitset_dict, S.unitset_sort):
            res = f(alleles)
            assert _triples(res) == units and res["record"][1] == n_classes, name
            assert res["record"][0] == len(units) and res["record"][3] == (0 if units else S.NONE)
            assert res["record"][4] == sum(c["weight"] for c in res["classes"])
        if units:
            got = [L.locus_np(a, [u[0] for u in res["units"]])[0][:6] for a in alleles]
            assert got == loci, name
    # the representative, not the smallest rotation: group A parses at 0 edits with the set as written, and the smallest rotations
    # {AGC, CCG} cost an edit at the junction.  (Group B does not show it: {AAG, AAAG} happen to stay in one phase and parse at 0 edits too.)
    a0, b0 = Uc.PROTOTYPES["A"][0][0], Uc.PROTOTYPES["B"][0][0]
    assert L.locus_np(a0, [b"CAG", b"CCG"])[0][3:5] == (0, 1) and L.locus_np(a0, [b"AGC", b"CCG"])[0][3:5] == (1, 1)
    assert L.locus_np(b0, [b"AGA", b"AAGA"])[0][3:5] == L.locus_np(b0, [b"AAG", b"AAAG"])[0][3:5] == (0, 2)
    # two copies, so that the junction counts
    assert S.U.unitalign_np(b"AGAA", b"GAA")[0] == 0 and S.U.unitalign_np(b"AGAAAGAA", b"GAA")[0] == 1
    # kept and dropped pairs of the rule's text
    assert not S._redundant(b"CAA", b"CAG", 100) and not S._redundant(b"AAAGG", b"AAAAG", 100)
    assert S.unitset_dict([]) == S.unitset_sort([]) and S.unitset_dict([])["record"] == (0, 0, 0, S.NONE, 0)
    for bad in ((0, 50, 100), ((1 << 24) + 1, 50, 100), (12, 1001, 100), (12, 50, 1001)):
        assert not S.params_ok(*bad)
    assert S.params_ok(*S.DEFAULT) and S.params_ok(1, 0, 0) and S.params_ok(1 << 24, 1000, 1000) and not S.params_ok(12, 50, 100, 1)


def test_edge_cases_agree_between_the_forms():
    for name, alleles, kw in Uc.ranking_cases() + Uc.threshold_cases() + Uc.budget_cases():
        a, b = S.unitset_dict(alleles, **kw), S.unitset_sort(alleles, **kw)
        assert a["record"] == b["record"] and a["units"] == b["units"], name
    want = {"three rotations, one class": [(b"GCA", 75, 3)], "representative: the lower begin wins a tie": [(b"ACG", 51, 3)],
            "representative: the lower allele wins a tie": [(b"CGA", 51, 3)], "equal weight: the shorter first": [(b"AT", 18, 1), (b"ACG", 18, 1)],
            "equal weight and length: the smaller rotation first": [(b"GCA", 18, 1), (b"GTA", 18, 1), (b"TCA", 18, 1)]}
    for name, alleles, kw in Uc.ranking_cases():
        if name in want:
            assert _triples(S.unitset_dict(alleles, **kw)) == want[name], name
    th = {name: S.unitset_dict(alleles, **kw) for name, alleles, kw in Uc.threshold_cases()}
    assert th["weight = min_bases"]["record"][:4] == (1, 1, 1, 0) and th["weight = min_bases - 1"]["record"][:4] == (0, 1, 0, S.NONE)
    assert th["share = min_permille"]["record"][:3] == (2, 2, 2) and th["share just under, by the parameter"]["record"][:3] == (1, 2, 1)
    assert th["share just under, by the input"]["record"][:3] == (1, 2, 1)
    assert th["2 edits in 20 bases: redundant"]["redundant"] == [False, True, True] and th["2 edits in 18 bases: kept"]["redundant"] == [False, False]
    assert th["2 edits in 18 bases at 112: redundant"]["redundant"] == [False, True]
    bu = {name: S.unitset_dict(alleles, **kw) for name, alleles, kw in Uc.budget_cases()}
    assert bu["twenty classes: sixteen ranked"]["record"][:3] == (8, 20, 16) and bu["ten 3-base units: eight taken"]["record"][:3] == (8, 10, 10)
    assert [u[3] for u in bu["200 + 100 + 40 bases: the second does not fit"]["units"]] == [200, 40]
    over = S.unitset_dict(Uc.overflow_group())
    assert over["record"] == S.unitset_sort(Uc.overflow_group())["record"] == (0, S.MAX_CLASSES + 1, 0, S.NONE | S.OVERFLOW, 2100 * 16)


# ---------------------------------------------------------------------------------------------- 2: the forms, the witness, the properties
def test_smallest_rotation_against_the_witness():
    rng = random.Random(3)
    for k in range(600):
        p = 1 + k % 40
        u = tuple(rng.randrange(4) for _ in range(p)) if k % 3 else tuple(rng.randrange(2) for _ in range(p))
        r, rot = S.min_rotation(u)
        assert rot == S.rotation_witness(u)[1] == u[r:] + u[:r]
        if S.primitive(u):
            assert r == S.rotation_witness(u)[0]
    assert S.min_rotation((1, 0, 2))[1] == S.min_rotation((0, 2, 1))[1] == S.min_rotation((2, 1, 0))[1] == (0, 2, 1)       # CAG, AGC, GCA
    assert S.primitive((0, 1, 0)) and not S.primitive((0, 1, 0, 1)) and S.primitive((0,))


@pytest.fixture(scope="module")
def random_groups():
    groups = Uc.random_groups(7, [0, 1, 2, 5, 3, 8, 2, 1, 4, 6] * 6, lower=0.2)
    return groups, [S.unitset_dict(g) for g in groups]


def test_two_forms_agree_on_random_groups(random_groups):
    groups, res = random_groups
    n_sets = n_two = 0
    for g, a in zip(groups, res):
        b = S.unitset_sort(g)
        assert a["record"] == b["record"] and a["units"] == b["units"]
        assert [(c["rot"], c["weight"], c["segments"], c["rep"]) for c in a["ranked"]] == [(c["rot"], c["weight"], c["segments"], c["rep"]) for c in b["ranked"]]
        n_sets += bool(a["units"]); n_two += len(a["units"]) > 1
        lanes = sum((u[3] + 3) // 4 for u in a["units"])
        assert len(a["units"]) <= S.MAX_UNITS and lanes <= S.MAX_LANES and a["record"][2] <= S.TOP
        L.P.check_units([u[0] for u in a["units"]]) if a["units"] else None                 # the joint parse accepts every discovered set
    assert n_sets > 40 and n_two > 10


def test_properties_of_the_rule(random_groups):
    groups, res = random_groups
    rng = random.Random(19)
    for g, a in zip(groups, res):
        # the order in which the segments are processed
        n = len(S.candidates(g))
        order = list(range(n)); rng.shuffle(order)
        b = S.unitset_dict(g, order=order)
        assert a["record"] == b["record"] and a["units"] == b["units"]
        # a permutation of the alleles: at most another, equally long segment gives a representative
        perm = list(g); rng.shuffle(perm)
        c = S.unitset_dict(perm)
        assert a["record"][:3] == c["record"][:3] and a["record"][4] == c["record"][4]
        assert sorted((cl["rot"], cl["weight"], cl["segments"]) for cl in a["classes"]) == sorted((cl["rot"], cl["weight"], cl["segments"]) for cl in c["classes"])
        assert [(cl["rot"], cl["weight"]) for cl in a["ranked"]] == [(cl["rot"], cl["weight"]) for cl in c["ranked"]]
    # a rotation of every copy of a unit in every allele changes only the representatives
    for k in range(40):
        units = [Uc.primitive_unit(rng, rng.randrange(2, 8)) for _ in range(3)]
        plan = [[(rng.randrange(3), rng.randrange(4, 12)) for _ in range(rng.randrange(1, 4))] for _ in range(3)]
        rots = [rng.randrange(len(u)) for u in units]
        plain = [Uc.blocks(*[(units[i], n) for i, n in al]) for al in plan]
        turned = [Uc.blocks(*[(units[i][rots[i]:] + units[i][:rots[i]], n) for i, n in al]) for al in plan]
        x, y = S.unitset_dict(plain, redundant_permille=0), S.unitset_dict(turned, redundant_permille=0)
        assert x["record"] == y["record"] and [u[1:] for u in x["units"]] == [u[1:] for u in y["units"]]
        assert [c["rot"] for c in x["ranked"]] == [c["rot"] for c in y["ranked"]]


# ---------------------------------------------------------------------------------------------- 3: recovery
@pytest.mark.parametrize("rate", sorted(Uc.RECOVERY_SEEDS))
def test_recovery_of_planted_units(rate):
    """Measured with the committed generator (DESIGN_LOG.md): 198 / 197 / 199 of 200 at 0 / 1 % / 3 %."""
    rng = random.Random(Uc.RECOVERY_SEEDS[rate])
    equal = subset = superset = 0
    for _ in range(200):
        alleles, units = Uc.planted_locus(rng, rate)
        assert 1 <= len(units) <= 3 and len(alleles) == 4 and all(2 <= len(u) <= 12 and S.primitive(tuple(u)) for u in units)
        want = {S.letters(S.min_rotation(S.U.codes(u))[1]) for u in units}
        got = S.class_set(S.unitset_dict(alleles))
        equal += got == want; subset += got < want; superset += got > want
    print("recovery at %g: %d equal, %d strict subsets, %d strict supersets of 200" % (rate, equal, subset, superset))
    assert equal >= 190


# ---------------------------------------------------------------------------------------------- 4: the kernels' arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("unitset_core") / "unitset_core_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "unitset_core_host.cpp")])
    return exe


def _run(exe, groups, params=S.DEFAULT, hash_bits=64, slots=128, threads=64, seed=0):
    """-> per group (record, units, hash matches the compare told apart)"""
    text = []
    for g in groups:
        text.append("group %d %d %d %d %d %d %d %d" % ((len(g),) + tuple(params) + (hash_bits, slots, threads, seed)))
        for s in g:
            segs = [x for x in Rp.structure_cached(bytes(s))["segs"] if 0 < x[1] <= S.MAX_UNIT]
            text.append("%s %d %s" % (bytes(s).hex() or "-", len(segs), " ".join("%d %d %d" % (b, p, ln) for b, p, _, ln in segs)))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines, out = r.stdout.splitlines(), []
    while lines:
        head = lines.pop(0).split()
        assert head[0] == "set"
        rec = tuple(int(x) for x in head[1:6])
        units = []
        for _ in range(rec[0]):
            h, w, sg, ln = lines.pop(0).split()
            units.append((bytes.fromhex(h), int(w), int(sg), int(ln)))
        out.append((rec, units, int(head[6])))
    assert len(out) == len(groups)
    return out


def _params(kw):
    d = dict(min_bases=12, min_permille=50, redundant_permille=100); d.update(kw)
    return d["min_bases"], d["min_permille"], d["redundant_permille"]


def test_core_on_the_prototype_rows_and_the_edge_cases(harness):
    groups = [v[0] for v in Uc.PROTOTYPES.values()]
    for (rec, units, _), g in zip(_run(harness, groups), groups):
        want = S.unitset_dict(g)
        assert rec == want["record"] and units == want["units"]
    for name, alleles, kw in Uc.ranking_cases() + Uc.threshold_cases() + Uc.budget_cases():
        want = S.unitset_dict(alleles, **kw)
        for slots, threads in ((128, 64), (2560, 256)):
            (rec, units, _), = _run(harness, [alleles], _params(kw), slots=slots, threads=threads, seed=1)
            assert rec == want["record"] and units == want["units"], (name, slots)


@pytest.mark.parametrize("hash_bits,slots,threads,seed", [(64, 128, 64, 0), (64, 2560, 256, 5), (3, 128, 64, 6), (1, 2560, 256, 7), (2, 128, 64, 0)])
def test_core_on_random_groups(harness, random_groups, hash_bits, slots, threads, seed):
    groups, res = random_groups
    groups = [g for g in groups if sum(len([x for x in Rp.structure_cached(bytes(s))["segs"] if x[1]]) for s in g) <= 64 or slots > 128]
    got = _run(harness, groups, hash_bits=hash_bits, slots=slots, threads=threads, seed=seed)
    for g, (rec, units, _) in zip(groups, got):
        want = S.unitset_dict(g)
        assert rec == want["record"] and units == want["units"], g
    told = sum(t for _, _, t in got)
    assert hash_bits < 64 or told == 0
    # few hash bits: ten classes of one length share two hash values, so at least eight insertions pass another class's slot, and the
    # compare on the bases tells them apart
    name, alleles, kw = Uc.budget_cases()[1]
    (rec, units, told), = _run(harness, [alleles], _params(kw), hash_bits=1, slots=slots, threads=threads, seed=seed)
    want = S.unitset_dict(alleles, **kw)
    assert rec == want["record"] and units == want["units"] and told >= 8 and rec[1] == 10


def test_core_on_one_large_group_and_the_class_cap(harness):
    big = Uc.random_groups(23, [300], n_units=3, p_max=7)[0]
    want = S.unitset_dict(big)
    assert len(S.candidates(big)) > 64 and want["record"][1] > 8            # more segments than one wave votes on; the noisy copies add classes
    for bits, seed in ((64, 0), (4, 9)):
        (rec, units, told), = _run(harness, [big], hash_bits=bits, slots=2560, threads=256, seed=seed)
        assert rec == want["record"] and units == want["units"] and (bits < 64 or told == 0)
    over = Uc.overflow_group()
    (rec, units, _), = _run(harness, [over], slots=2560, threads=256, seed=3)
    assert rec == S.unitset_dict(over)["record"] == (0, 2049, 0, 3, 33600) and units == []
    (rec, units, _), = _run(harness, [Uc.overflow_group(2048, 64)], slots=2560, threads=256, seed=4)      # exactly the cap: no overflow
    assert rec[1:4] == (2048, 16, 0) and rec[0] == 8


# ---------------------------------------------------------------------------------------------- 5: the catalogue text
def _emit_inputs():
    groups = [Uc.PROTOTYPES[k][0] for k in "ABF"] + [Uc.PROTOTYPES["G"][0]]
    res = [S.unitset_dict(g) for g in groups]
    regions = [b"chr1:100-160", b"chr2:5-9", b"chrUn_x:0-77", b"chr1:100-160"]
    beds = [(b"chr2", 5, 9), (b"chr1", 100, 160), (b"chr1", 100, 160), (b"chrUn_x", 0, 77)]
    records = np.zeros(len(groups), dtype=abi.vcf_record_dt)
    pos = first = 0
    for r, g in enumerate(groups):
        records[r] = (pos, len(regions[r]), first, len(g), 0)
        pos += len(regions[r]); first += len(g)
    sets = np.array([r["record"] for r in res], dtype=abi.unitset_dt)
    return groups, res, regions, beds, records, sets


def test_emit_against_python_rows(tmp_path):
    groups, res, regions, beds, records, sets = _emit_inputs()
    units = [r["units"] for r in res]
    text = otter_amd.unitset_emit(records, b"".join(regions), beds, sets, units)
    where = {b"chr1:100-160": (b"chr1", 100, 160), b"chr2:5-9": (b"chr2", 5, 9), b"chrUn_x:0-77": (b"chrUn_x", 0, 77)}
    want = b"".join(S.row(*where[regions[r]], res[r], len(groups[r])) for r in range(len(groups)))
    assert text == want
    lines = want.split(b"\n")
    assert lines[0] == b"chr1\t100\t160\tMOTIFS=CAG,CCG;BASES=120,48;SEGMENTS=3,2;ALLELES=2"
    assert lines[1] == b"chr2\t5\t9\tMOTIFS=AGA,AAGA;BASES=153,20;SEGMENTS=3,1;ALLELES=2"
    assert lines[2] == b"chrUn_x\t0\t77\t." and lines[3] == b"chr1\t100\t160\tMOTIFS=ACGGTCATTG;BASES=60;SEGMENTS=1;ALLELES=3" and len(lines) == 5
    assert otter_amd.unitset_emit(records[:0], b"", beds, sets[:0], []) == b""
    # the emitted catalogue is what every catalogue tool reads: the same sets come back
    path = str(tmp_path / "units.bed")
    open(path, "wb").write(text)
    assert otter_amd.parse_bed_units(path) == [[u[0] for u in r["units"]] for r in res]
    assert [(c, s, e) for c, s, e in otter_amd.bed_tuples(*otter_amd.parse_bed_file(path)[:2])] == [("chr1", 100, 160), ("chr2", 5, 9), ("chrUn_x", 0, 77), ("chr1", 100, 160)]
    # a record without a BED record is refused by name
    with pytest.raises(otter_amd.OtterGpuError, match="no BED record for the region chr2:5-9"):
        otter_amd.unitset_emit(records, b"".join(regions), [b for b in beds if b[0] != b"chr2"], sets, units)
    bad = sets.copy(); bad[0]["n_units"] = 1
    with pytest.raises(otter_amd.OtterGpuError, match="set 0 has 1 units"):
        otter_amd.unitset_emit(records, b"".join(regions), beds, bad, units)


# ---------------------------------------------------------------------------------------------- 6: refusals without a device
def test_refusals_without_a_device():
    lib = otter_amd.load()
    u, u64 = C.c_uint32, C.c_uint64
    gf = np.zeros(2, dtype=np.uint32)
    q = abi.UnitsetParams()
    lib.otg_unitset_params_default(C.byref(q))
    assert (q.min_bases, q.min_permille, q.redundant_permille, q.reserved) == S.DEFAULT + (0,)
    lib.otg_unitset_params_default(None)
    assert lib.otg_unitset_repeats(None, abi.ptr(gf), u(1), None, None, None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert lib.otg_unitset_repeats(None, None, u(1), None, None, None, None, None) == abi.OTG_ERR_ARG
    assert b"NULL group_first" in lib.otg_last_error(None)
    assert lib.otg_unitset_repeats(None, abi.ptr(gf), u((1 << 24) + 1), None, None, None, None, None) == abi.OTG_ERR_CAPACITY
    for bad in ((0, 50, 100, 0), ((1 << 24) + 1, 50, 100, 0), (12, 1001, 100, 0), (12, 50, 1001, 0), (12, 50, 100, 1)):
        p = abi.UnitsetParams(*bad)
        assert lib.otg_unitset_repeats(None, abi.ptr(gf), u(1), C.byref(p), None, None, None, None) == abi.OTG_ERR_ARG
        assert b"outside 1..16777216, 0..1000, 0..1000, 0" in lib.otg_last_error(None)
    assert lib.otg_unitset_collect(None, None, None, None, u64(0), None, u64(0)) == abi.OTG_ERR_ARG
    assert lib.otg_unitset_device_results(None, None, None, None, None, None, None, None, None, None) == abi.OTG_ERR_ARG
    assert lib.otg_unitset_last_ms(None, None, None) == abi.OTG_ERR_ARG
    assert lib.otg_unitset_locus(None, None, None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert lib.otg_unitset_emit(None, u(0), None, None, None, u(0), None, None, None, None, None, None, None, u64(0), None) == abi.OTG_ERR_ARG


# ---------------------------------------------------------------------------------------------- 7: the mirrors
def test_abi_mirrors(tmp_path):
    txt = open(HEADER).read()
    defs = {k: v for k, v in re.findall(r"#define\s+(OTG_UNITSET_[A-Z_0-9]+)\s+(\S+)", txt)}
    assert set(defs) == {"OTG_UNITSET_TOP", "OTG_UNITSET_MAX_CLASSES", "OTG_UNITSET_NONE", "OTG_UNITSET_OVERFLOW", "OTG_UNITSET_LOCUS_NO_SET"}
    assert (int(defs["OTG_UNITSET_TOP"]), int(defs["OTG_UNITSET_MAX_CLASSES"])) == (abi.UNITSET_TOP, abi.UNITSET_MAX_CLASSES) == (S.TOP, S.MAX_CLASSES) == (16, 2048)
    assert tuple(int(defs[k].rstrip("u")) for k in ("OTG_UNITSET_NONE", "OTG_UNITSET_OVERFLOW", "OTG_UNITSET_LOCUS_NO_SET")) == \
        (abi.UNITSET_NONE, abi.UNITSET_OVERFLOW, abi.UNITSET_LOCUS_NO_SET) == (S.NONE, S.OVERFLOW, 4)
    assert abi.UNITSET_LOCUS_NO_SET & (abi.LOCUS_TOO_LONG | abi.LOCUS_NONE) == 0
    assert (S.MAX_UNITS, S.MAX_LANES, S.MAX_UNIT) == (abi.UNITPARSE_MAX_UNITS, abi.UNITPARSE_MAX_LANES, abi.UNITALIGN_MAX_UNIT)
    for name, dt in (("otg_unitset", abi.unitset_dt), ("otg_unitset_unit", abi.unitset_unit_dt)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
        assert re.findall(r"uint(?:32|64)_t\s+(\w+);", body) == list(dt.names)
    body = re.search(r"typedef struct otg_unitset_params \{(.*?)\} otg_unitset_params;", txt, flags=re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == [n for n, _ in abi.UnitsetParams._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",sizeof(otg_unitset),'
                   'offsetof(otg_unitset,weight_total),sizeof(otg_unitset_unit),offsetof(otg_unitset_unit,segments),sizeof(otg_unitset_params));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.unitset_dt.itemsize, abi.unitset_dt.fields["weight_total"][1], abi.unitset_unit_dt.itemsize, abi.unitset_unit_dt.fields["segments"][1],
                   C.sizeof(abi.UnitsetParams)] == [24, 16, 16, 8, 16]
    names = {"otg_unitset_params_default", "otg_unitset_repeats", "otg_unitset_collect", "otg_unitset_device_results", "otg_unitset_last_ms", "otg_unitset_locus",
             "otg_unitset_emit"}
    assert {n for n in otter_amd.EXPORTS if n.startswith("otg_unitset")} == names
    lib = otter_amd.load()
    for n in names:
        assert getattr(lib, n) is not None
    for f in ("unitset_repeats", "unitset_last_ms", "locus_unitsets", "cohort_unitsets"):
        assert callable(getattr(otter_amd.Context, f))
    assert callable(otter_amd.unitset_emit)


def test_units_job_refusals_and_the_tools_messages(tmp_path):
    lib = otter_amd.load()
    assert lib.otg_units_files(None, None, None, None) == abi.OTG_ERR_ARG and lib.otg_units_loci_files(None, None, None, None, None) == abi.OTG_ERR_ARG
    txt = open(HEADER).read()
    body = re.search(r"typedef struct otg_units_job \{(.*?)\} otg_units_job;", txt, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.UnitsJob._fields_] and C.sizeof(abi.UnitsJob) == 56
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    for kw, msg in ((dict(max_period=0), "invalid '--max-period' (0)"), (dict(min_copies=1), "invalid '--min-copies' (1)"), (dict(min_span=1), "invalid '--min-span' (1)"),
                    (dict(min_bases=0), "invalid '--min-bases' (0). Needs to be 1 <= x <= 16777216."), (dict(min_bases=(1 << 24) + 1), "invalid '--min-bases' (16777217)"),
                    (dict(min_share=1001), "invalid '--min-share' (1001). Needs to be 0 <= x <= 1000."), (dict(redundant=1001), "invalid '--redundant' (1001). Needs to be 0 <= x <= 1000.")):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.units_files(vcf, bed, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and msg in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.units_files(vcf, str(tmp_path / "missing.bed"))
    exe = os.path.join(ROOT, "tools", "otter_units")
    for args, msg in ((["--min-bases", "0"], b"invalid '--min-bases' (0). Needs to be 1 <= x <= 16777216."), (["--min-share=1001"], b"invalid '--min-share' (1001)"),
                      (["--redundant", "-1"], b"invalid '--redundant' (-1)"), (["-p", "4097"], b"invalid '--max-period' (4097)"), (["--min-copies", "1"], b"invalid '--min-copies' (1)"),
                      (["--min-span", "x"], None), (["--min-bases"], None)):
        r = subprocess.run([exe, "-b", bed] + ([vcf] if args != ["--min-bases"] else []) + args, capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout.count(b"\t") == 0, (args, r)
        assert msg is None or msg in r.stderr
    assert subprocess.run([exe, vcf], capture_output=True, timeout=60).returncode == 1           # no BED
    assert subprocess.run([exe, "-b", str(tmp_path / "missing.bed"), vcf], capture_output=True, timeout=60).returncode == 1
    r = subprocess.run([exe], capture_output=True, timeout=60)                                   # the usage text
    assert r.returncode == 0 and b"Usage:" in r.stdout
    assert all(w in r.stdout for w in (b"--bed", b"--max-period", b"--min-copies", b"--min-span", b"--min-bases", b"--min-share", b"--redundant", b"--threads", b"--batch"))


def test_loci_tool_discovery_switches(tmp_path):
    exe = os.path.join(ROOT, "tools", "otter_loci")
    bed, vcf = str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    open(bed, "w").write("chr1\t100\t150\n")
    open(vcf, "w").write("chr1\t100\tchr1:100-150\tACGT\tA\n")
    for args, msg in ((["--discover", "--min-bases", "0"], b"invalid '--min-bases' (0). Needs to be 1 <= x <= 16777216."), (["--discover", "--min-share=1001"], b"invalid '--min-share' (1001)"),
                      (["--discover", "--redundant", "-1"], b"invalid '--redundant' (-1)"), (["--discover", "-p", "4097"], b"invalid '-p' (4097). Needs to be 1 <= x <= 4096."),
                      (["--discover", "--min-copies", "1"], b"invalid '--min-copies' (1)"), (["--discover", "--min-span", "1"], b"invalid '--min-span' (1)"),
                      (["--discover", "--scores", "0,7,7"], b"invalid '--scores' (0,7,7)"), (["--discover", "--min-span", "x"], None)):
        r = subprocess.run([exe, "-b", bed] + args + [vcf], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout.count(b"\t") == 0, (args, r)
        assert msg is None or msg in r.stderr
    r = subprocess.run([exe, "-b", bed, "--min-bases", "20", vcf], capture_output=True, timeout=60)      # a discovery switch without --discover
    assert r.returncode == 1 and b"needs '--discover'" in r.stdout and b"Usage:" in r.stdout
    r = subprocess.run([exe], capture_output=True, timeout=60)
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--discover", b"-p <n>", b"--min-copies", b"--min-span", b"--min-bases", b"--min-share", b"--redundant"))
    lib = otter_amd.load()
    job, dj = abi.LociJob(), abi.UnitsJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode(); job.match, job.mismatch, job.indel, job.min_score = 2, 7, 7, 24
    dj.max_period, dj.min_copies, dj.min_span, dj.min_bases, dj.min_share, dj.redundant = 256, 2, 12, 12, 50, 1001
    cb = abi.WRITE_FN(lambda u, d, n: 0)
    assert lib.otg_units_loci_files(C.byref(job), C.byref(dj), cb, None, None) == abi.OTG_ERR_ARG and b"invalid '--redundant' (1001)" in lib.otg_last_error(None)
    assert lib.otg_units_loci_files(C.byref(job), None, cb, None, None) == abi.OTG_ERR_ARG

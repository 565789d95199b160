"""GPU: the unit-set discovery (otg_unitset_repeats / otg_unitset_locus).  Records, units and the locus records behind them must equal
tests/unitset_ref.py and tests/locus_ref.py (the rules of include/otter_gpu.h restated in plain Python) record for record and byte for byte,
on the smallest shapes at which the kernels can go wrong: empty groups, one-allele groups, a group larger than one wave votes on, every
threshold at equality, every budget, the class cap and one class under it, a truncated hash."""
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, synth
import cohort_matrix_helpers as M
import locus_cases as Lc
import locus_ref as L
import unitset_cases as Uc
import unitset_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _discover(gpu, groups, kw=None, repeat=S.REPEAT_DEFAULT, **more):
    alleles, first = Uc.flat(groups)
    gpu.repeat_batch(*abi.pack_seqs(alleles), *repeat)
    return gpu.unitset_repeats(first, **(kw or {}), **more)


def _check(gpu, groups, kw=None, repeat=S.REPEAT_DEFAULT):
    kw = kw or {}
    sets, units = _discover(gpu, groups, kw, repeat)
    assert sets.shape == (len(groups),) and len(units) == len(groups)
    want = [S.unitset_dict(g, repeat=repeat, **kw) for g in groups]
    for g, w in enumerate(want):
        assert tuple(int(x) for x in sets[g]) == w["record"] and units[g] == w["units"], (g, groups[g][:3], sets[g], units[g], w["record"], w["units"])
    return sets, units, want


# ---------------------------------------------------------------------------------------------- 1: the prototype rows and the locus chain
def test_prototype_rows_and_the_locus_chain(gpu):
    names = sorted(Uc.PROTOTYPES)
    groups = [Uc.PROTOTYPES[k][0] for k in names]
    sets, units, want = _check(gpu, groups)
    for g, k in enumerate(names):
        _, table_units, n_classes, _ = Uc.PROTOTYPES[k]
        assert [u[:3] for u in units[g]] == table_units and int(sets[g]["n_classes"]) == n_classes
    assert int(sets[names.index("F")]["flags"]) == abi.UNITSET_NONE and sum(int(f) for f in sets["flags"]) == abi.UNITSET_NONE
    vote, select = gpu.unitset_last_ms()
    assert vote > 0 and select > 0
    # the same results where they lie in HBM
    dev = gpu.unitset_repeats(Uc.flat(groups)[1], device_tensor=True)
    assert np.array_equal(dev[0].cpu().numpy().view(np.uint32).reshape(-1), sets.view(np.uint32).reshape(-1))
    assert dev[1].cpu().numpy().tolist() == np.cumsum([0] + [len(u) for u in units]).tolist()
    flat = [u for g in units for u in g]
    assert dev[5].cpu().numpy().tobytes() == b"".join(u[0] for u in flat) and dev[4].cpu().numpy().tolist() == [u[3] for u in flat]
    assert [int(x) for x in dev[2].cpu().numpy().view(np.uint64).reshape(-1, 2)[:, 0]] == [u[1] for u in flat]
    # the locus mode of every allele against the set of its group, the alleles read in place
    alleles, first = Uc.flat(groups)
    recs, seg_off, segs = gpu.locus_unitsets()
    assert recs.shape == (len(alleles),) and seg_off.shape == (len(alleles) + 1,) and int(seg_off[-1]) == len(segs)
    a = 0
    for g, k in enumerate(names):
        loci = Uc.PROTOTYPES[k][3]
        for i, s in enumerate(groups[g]):
            got = recs[a], segs[int(seg_off[a]):int(seg_off[a + 1])]
            if units[g]:
                assert tuple(int(x) for x in got[0])[:6] == loci[i]
                Lc.check(*got, L.locus_np(s, [u[0] for u in units[g]]))
            else:
                assert tuple(int(x) for x in got[0]) == (0,) * 7 + (abi.UNITSET_LOCUS_NO_SET,) and len(got[1]) == 0
            a += 1
    both, local = gpu.locus_last_ms()
    assert 0 < local < both and sum(gpu.locus_last_tiers()) == sum(len(g) for g, u in zip(groups, units) if u and all(len(s) for s in g))
    dev = gpu.locus_unitsets(device_tensor=True)
    assert np.array_equal(dev[0].cpu().numpy().astype(np.uint32), recs.view(np.uint32).reshape(-1, 8)) and dev[1].cpu().numpy().tolist() == seg_off.tolist()
    assert np.array_equal(dev[2].cpu().numpy().astype(np.uint32), segs.view(np.uint32).reshape(-1, 6))
    with pytest.raises(otter_amd.OtterGpuError, match="min_score|scores"):
        gpu.locus_unitsets(indel=0)


# ---------------------------------------------------------------------------------------------- 2: random groups, three groupings
@pytest.fixture(scope="module")
def random_groups():
    return Uc.random_groups(7, [0, 1, 2, 5, 3, 8, 2, 1, 4, 6] * 5 + [1000, 0, 2], lower=0.2)


def test_random_groups_as_given(gpu, random_groups):
    sets, units, want = _check(gpu, random_groups)
    big = max(range(len(random_groups)), key=lambda g: len(random_groups[g]))
    assert len(random_groups[big]) == 1000 and len(S.candidates(random_groups[big])) > 4 * 64 and units[big]     # more than one wave votes on it
    assert sum(1 for u in units if len(u) > 1) > 10 and sum(1 for u in units if not u) >= 6
    # the locus chain: every allele against the set of its group
    recs, seg_off, segs = gpu.locus_unitsets()
    a = n_tract = 0
    for g, grp in enumerate(random_groups):
        for s in grp:
            if a % 7 == 0 or len(grp) <= 8:                                 # (the reference of the large group: every seventh allele)
                if units[g]:
                    Lc.check(recs[a], segs[int(seg_off[a]):int(seg_off[a + 1])], L.locus_np(s, [u[0] for u in units[g]]))
                    n_tract += int(recs[a]["flags"]) == 0
                else:
                    assert int(recs[a]["flags"]) == abi.UNITSET_LOCUS_NO_SET and seg_off[a] == seg_off[a + 1]
            a += 1
    assert a == len(recs) and n_tract > 200


def test_random_groups_as_one_group_and_one_by_one(gpu, random_groups):
    alleles, _ = Uc.flat(random_groups)
    alleles = alleles[:200] + alleles[-300:]
    _check(gpu, [alleles])
    sets, units, _ = _check(gpu, [[s] for s in alleles])
    assert len(sets) == len(alleles)


def test_other_repeat_parameters(gpu, random_groups):
    _check(gpu, random_groups[:40], dict(min_bases=20, min_permille=200, redundant_permille=250), repeat=(6, 3, 8))


# ---------------------------------------------------------------------------------------------- 3: ranks, thresholds, budgets
def test_ranking_threshold_and_budget_cases(gpu):
    cases = Uc.ranking_cases() + Uc.threshold_cases() + Uc.budget_cases()
    by_kw = {}
    for name, alleles, kw in cases:
        by_kw.setdefault(tuple(sorted(kw.items())), []).append((name, alleles))
    seen = {}
    for kw, lst in by_kw.items():
        sets, units, want = _check(gpu, [al for _, al in lst], dict(kw))
        for (name, _), s, u in zip(lst, sets, units):
            seen[name] = (tuple(int(x) for x in s), u)
    assert [u[:3] for u in seen["three rotations, one class"][1]] == [(b"GCA", 75, 3)]
    assert seen["representative: the lower begin wins a tie"][1][0][0] == b"ACG" and seen["representative: the lower allele wins a tie"][1][0][0] == b"CGA"
    assert [u[0] for u in seen["equal weight: the shorter first"][1]] == [b"AT", b"ACG"]
    assert [u[0] for u in seen["equal weight and length: the smaller rotation first"][1]] == [b"GCA", b"GTA", b"TCA"]
    assert seen["weight = min_bases"][0][:4] == (1, 1, 1, 0) and seen["weight = min_bases - 1"][0][:4] == (0, 1, 0, abi.UNITSET_NONE)
    assert seen["share = min_permille"][0][:3] == (2, 2, 2) and seen["share just under, by the parameter"][0][:3] == (1, 2, 1)
    assert seen["share just under, by the input"][0][:3] == (1, 2, 1)
    assert seen["2 edits in 20 bases: redundant"][0][:3] == (1, 3, 3) and seen["2 edits in 18 bases: kept"][0][:3] == (2, 2, 2)
    assert seen["twenty classes: sixteen ranked"][0][:3] == (8, 20, 16) and seen["ten 3-base units: eight taken"][0][:3] == (8, 10, 10)
    assert [u[3] for u in seen["200 + 100 + 40 bases: the second does not fit"][1]] == [200, 40]


def test_class_cap(gpu):
    groups = [Uc.PROTOTYPES["A"][0], Uc.overflow_group(), Uc.overflow_group(2048, 64), Uc.PROTOTYPES["B"][0]]
    sets, units, _ = _check(gpu, groups)
    assert tuple(int(x) for x in sets[1]) == (0, 2049, 0, abi.UNITSET_NONE | abi.UNITSET_OVERFLOW, 2100 * 16) and units[1] == []
    assert tuple(int(x) for x in sets[2])[:4] == (8, 2048, 16, 0)
    recs, seg_off, _ = gpu.locus_unitsets()                                   # the group over the cap has no set; its neighbours keep theirs
    n0, n1 = len(groups[0]), len(groups[1])
    assert all(int(f) == abi.UNITSET_LOCUS_NO_SET for f in recs["flags"][n0:n0 + n1]) and all(int(f) == 0 for f in recs["flags"][:n0])


def test_truncated_hash_in_a_fresh_process():
    env = dict(os.environ, OTG_UNITSET_HASH_BITS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unitset_hash_child.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- 4: refusals on a context
def test_refusals(gpu):
    fresh = otter_amd.Context(0)
    try:
        with pytest.raises(otter_amd.OtterGpuError, match="no repeat results"):
            fresh.unitset_repeats([0, 1])
        with pytest.raises(otter_amd.OtterGpuError, match="no unit set results"):
            fresh.locus_unitsets()
    finally:
        fresh.close()
    alleles = Uc.PROTOTYPES["A"][0] + Uc.PROTOTYPES["C"][0]
    gpu.repeat_batch(*abi.pack_seqs(alleles))
    for bad in ([0, 2, 4], [1, 2, 5], [0, 3, 2, 5], [0, 6]):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.unitset_repeats(bad)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "group_first" in str(e.value), bad
    for kw in (dict(min_bases=0), dict(min_permille=1001), dict(redundant_permille=1001)):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.unitset_repeats([0, 2, 5], **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), kw
    with pytest.raises(otter_amd.OtterGpuError, match="no unit set results"):    # a refused discovery leaves none behind
        gpu.locus_unitsets()
    sets, units = gpu.unitset_repeats([0, 2, 5])
    assert [u[0] for u in units[0]] == [b"CAG", b"CCG"] and [u[0] for u in units[1]] == [b"AGC"]
    gpu.repeat_batch(*abi.pack_seqs(alleles[:2]))                             # a repeat call between the discovery and the locus chain
    with pytest.raises(otter_amd.OtterGpuError, match="a repeat call lies between"):
        gpu.locus_unitsets()
    L_ = otter_amd.load()
    import ctypes as C
    assert L_.otg_unitset_collect(gpu._h, None, None, None, C.c_uint64(0), None, C.c_uint64(0)) == abi.OTG_ERR_CAPACITY
    assert b"3 units and 9 bytes" in L_.otg_last_error(gpu._h)


# ---------------------------------------------------------------------------------------------- 5: the rows of a cohort
def test_cohort_rows(gpu):
    B, Sn = 4, 2
    P = abi.default_params(max_alleles=4)
    other = otter_amd.Context(0)
    try:
        gpu.cohort_begin(B, Sn)
        for k in range(Sn):                                                # staged as tests/test_gpu_locus.py stages them
            b = synth.make_batch(B, len_range=(150, 400), reads_range=(8, 14), err="hifi", seed=911 + k, frac_partial=0.1, frac_het=0.8)
            ctx = other if (k % 2) else gpu
            ctx.assemble_submit(P, b)
            ctx.assemble_run()
            ctx.assemble_collect()
            gpu.cohort_stage(k, src=ctx)
    finally:
        other.close()
    rng = np.random.default_rng(4)
    import motif_cases as Cs
    units = [Cs.rs(rng, int(rng.integers(2, 7))) for _ in range(B)]
    refs = [Cs.rs(rng, 9) + Cs.substitute(rng, units[k] * int(rng.integers(20, 40)), 2) + units[(k + 1) % B] * 6 + Cs.rs(rng, 11) for k in range(B)]
    gpu.cohort_regroup(*abi.pack_seqs(refs))
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    rows = gpu.cohort_kmer_rows()
    seqs = M.row_seqs(rows, got)
    first = [int(x) for x in rows["row_first"]]
    assert len(first) == B + 1 and first[-1] == len(seqs) >= 6
    sets, found = gpu.cohort_unitsets()
    groups = [seqs[first[g]:first[g + 1]] for g in range(B)]
    n_sets = 0
    for g, grp in enumerate(groups):
        want = S.unitset_dict(grp)
        assert tuple(int(x) for x in sets[g]) == want["record"] and found[g] == want["units"], g
        n_sets += bool(found[g])
    assert n_sets >= 1
    recs, seg_off, segs = gpu.locus_unitsets()                                # the cohort's alleles, read in the cohort arena in place
    for g, grp in enumerate(groups):
        for i, s in enumerate(grp):
            a = first[g] + i
            if found[g]:
                Lc.check(recs[a], segs[int(seg_off[a]):int(seg_off[a + 1])], L.locus_np(s, [u[0] for u in found[g]]))
            else:
                assert int(recs[a]["flags"]) == abi.UNITSET_LOCUS_NO_SET
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no longer on the device"):
        gpu.unitset_repeats(first)


# ---------------------------------------------------------------------------------------------- 6: files and the tool
def _vcf(tmp_path):
    names = "ABCDEFG"
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
    groups, beds = [], []
    for i, k in enumerate(names):
        al = [a if a else b"<DEL>" for a in Uc.PROTOTYPES[k][0]]
        lines.append(b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + al[0] + b"\t" + (b",".join(al[1:]) or b".") + b"\t.\tPASS\t.\tGT\t0/1")
        groups.append([a if a != b"<DEL>" else b"N" for a in al])           # (<DEL> is the allele N)
        beds.append((b"chr1", 100 * i, 100 * i + 50))
    vcf, bed = str(tmp_path / "calls.vcf"), str(tmp_path / "regions.bed")
    open(vcf, "wb").write(b"\n".join(lines) + b"\n")
    open(bed, "wb").write(b"".join(b"%s\t%d\t%d\n" % b for b in reversed(beds)))
    return vcf, bed, groups, beds


def test_units_files_and_the_tool(gpu, tmp_path):
    vcf, bed, groups, beds = _vcf(tmp_path)
    want = b"".join(S.row(*beds[g], S.unitset_dict(grp), len(grp)) for g, grp in enumerate(groups))
    text, stats = otter_amd.units_files(vcf, bed)
    assert text == want and stats["n_regions"] == len(groups) and stats["n_alleles"] == sum(len(g) for g in groups)
    assert text.split(b"\n")[0] == b"chr1\t0\t50\tMOTIFS=CAG,CCG;BASES=120,48;SEGMENTS=3,2;ALLELES=2" and text.split(b"\n")[5] == b"chr1\t500\t550\t."
    for kw in (dict(batch_alleles=2, threads=3), dict(batch_alleles=1), dict(batch_alleles=5, threads=2)):     # batches end at record boundaries
        assert otter_amd.units_files(vcf, bed, **kw)[0] == want, kw
    kw = dict(min_bases=30, min_share=200, redundant=99)
    other = b"".join(S.row(*beds[g], S.unitset_dict(grp, 30, 200, 99), len(grp)) for g, grp in enumerate(groups))
    assert otter_amd.units_files(vcf, bed, **kw)[0] == other != want
    r = subprocess.run([os.path.join(ROOT, "tools", "otter_units"), "-b", bed, "--min-bases", "30", "--min-share=200", "--redundant", "99", "-t", "2", vcf],
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == other, r.stderr[-2000:]
    # the output is a catalogue: the locus mode over files reads it and gives the rows of the table
    cat = str(tmp_path / "units.bed")
    open(cat, "wb").write(want)
    rows = otter_amd.loci_files(vcf, cat)[0].split(b"\n")
    first = rows[0].split(b"\t")
    assert first[3] == b"CAG,CCG" and tuple(int(x) for x in (first[6], first[4], first[5], first[7], first[8], first[9])) == Uc.PROTOTYPES["A"][3][0]
    # a VCF record without a BED record is refused by name
    short = str(tmp_path / "short.bed")
    open(short, "wb").write(b"chr1\t0\t50\n")
    with pytest.raises(otter_amd.OtterGpuError, match="no BED record for the region chr1:100-150"):
        otter_amd.units_files(vcf, short)


def test_loci_files_with_discovery(gpu, tmp_path):
    vcf, bed, groups, beds = _vcf(tmp_path)
    # the catalogue gives group A other units than the discovery would and group C a name; every other region has three columns
    cat = str(tmp_path / "cat.bed")
    open(cat, "wb").write(b"".join(b"%s\t%d\t%d" % b + (b"\tCAG,CCG,T" if g == 0 else b"\tlocus_c" if g == 2 else b"") + b"\n" for g, b in enumerate(beds)))
    want = []
    for g, grp in enumerate(groups):
        units = [b"CAG", b"CCG", b"T"] if g == 0 else [u[0] for u in S.unitset_dict(grp)["units"]]
        region = b"chr1:%d-%d" % beds[g][1:]
        for i, s in enumerate(grp):
            want.append(L.row(region, i, len(s), units, *(L.locus_np(s, units) if units else ((0,) * 8, []))))
    want = b"".join(want)
    text, stats = otter_amd.loci_files(vcf, cat, discover=True)
    assert text == want and stats["n_alleles"] == sum(len(g) for g in groups)
    for kw in (dict(batch_alleles=2, threads=3), dict(batch_alleles=1)):
        assert otter_amd.loci_files(vcf, cat, discover=True, **kw)[0] == want, kw
    plain = otter_amd.loci_files(vcf, cat)[0]                                 # without the switch: as before, only group A has units
    assert plain != want and plain.split(b"\n")[0] == want.split(b"\n")[0] and plain.split(b"\n")[2].split(b"\t")[3] == b"."
    assert want.split(b"\n")[2].split(b"\t")[3] == b"AGA,AAGA"
    exe = os.path.join(ROOT, "tools", "otter_loci")
    r = subprocess.run([exe, "-b", cat, "--discover", "-t", "2", "--batch", "3", vcf], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == want, r.stderr[-2000:]
    assert subprocess.run([exe, "-b", cat, vcf], capture_output=True, timeout=120).stdout == plain          # without the switch: as before
    kw = dict(min_bases=30, min_share=200, redundant=99)
    r = subprocess.run([exe, "-b", cat, "--discover", "--min-bases", "30", "--min-share=200", "--redundant", "99", "-p", "64", vcf], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == otter_amd.loci_files(vcf, cat, discover=True, max_period=64, **kw)[0] != want, r.stderr[-2000:]
    with pytest.raises(otter_amd.OtterGpuError, match="invalid '--min-share'"):
        otter_amd.loci_files(vcf, cat, discover=True, min_share=1001)
    with pytest.raises(otter_amd.OtterGpuError, match="invalid '--scores'"):
        otter_amd.loci_files(vcf, cat, discover=True, indel=0)

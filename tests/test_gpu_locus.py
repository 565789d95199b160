"""GPU: the locus mode (otg_locus_batch / _cohort / otg_loci_files, tools/otter_loci).  Records and segments must equal tests/locus_ref.py (the
rule of include/otter_gpu.h restated in plain Python) record for record and segment for segment, on the smallest shapes at which the kernel
can go wrong: every class of unit set, tracts that start and end on both sides of a 16-byte load, unequal tasks in one wave, min_score at a
tract's score, other scores, the boundary between the two key widths, the length cap."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, synth
import cohort_matrix_helpers as M
import locus_cases as Lc
import locus_ref as R
import motif_cases as Cs
import tract_cases as Tc
import unitalign_cases as Uc
import unitparse_cases as Pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "otter_loci")
_REF = {}


def ref(s, units, scores=R.DEFAULT):
    key = (s, tuple(units), scores)
    if key not in _REF:
        _REF[key] = R.locus_np(s, units, *scores)
    return _REF[key]


def _kw(scores):
    return dict(match=scores[0], mismatch=scores[1], indel=scores[2], min_score=scores[3])


def _run(gpu, tasks, scores=R.DEFAULT, **kw):
    seqs, sets, ts, tq = Lc.pack(tasks)
    arena, off, ln = abi.pack_seqs(seqs)
    return gpu.locus_batch(arena, off, ln, sets, ts, tq, **_kw(scores), **kw)


def _check(gpu, tasks, scores=R.DEFAULT):
    recs, seg_off, segs = _run(gpu, tasks, scores)
    assert recs.shape == (len(tasks),) and seg_off.shape == (len(tasks) + 1,) and seg_off[0] == 0 and int(seg_off[-1]) == len(segs)
    for t, (s, units) in enumerate(tasks):
        try:
            Lc.check(recs[t], segs[int(seg_off[t]):int(seg_off[t + 1])], ref(s, units, scores))
        except AssertionError:
            raise AssertionError((t, s[:100], [u[:40] for u in units], recs[t], segs[int(seg_off[t]):int(seg_off[t + 1])], ref(s, units, scores)))
    return recs, seg_off, segs


def _per_task(res):
    recs, seg_off, segs = res
    return [(recs[t].tobytes(), segs[int(seg_off[t]):int(seg_off[t + 1])].tobytes()) for t in range(len(recs))]


# ---------------------------------------------------------------------------------------------- 1: the table and the edge set
def test_table(gpu):
    recs, seg_off, segs = _check(gpu, [(s, u) for s, u, _, _ in Lc.TABLE])
    for t, (_, _, want, want_segs) in enumerate(Lc.TABLE):
        got = tuple(int(x) for x in recs[t])
        assert got[:6] == want and got[6] == want[4] + 1 and got[7] == 0
        if want_segs is not None:
            assert [tuple(int(x) for x in g)[:3] for g in segs[int(seg_off[t]):int(seg_off[t + 1])]] == want_segs
    both, local = gpu.locus_last_ms()
    assert 0 < local < both
    assert gpu.locus_last_tiers() == (len(Lc.TABLE), 0)
    empty = _run(gpu, [])
    assert empty[0].shape == (0,) and list(empty[1]) == [0] and empty[2].shape == (0,)


def test_edge_set(gpu):
    tasks = Lc.edge_set()
    classes = {R.unit_class([len(u) for u in units]) for _, units in tasks}
    assert classes == set(range(7)) and [R.unit_class(lens) for lens, _ in Lc.CLASS_SETS] == [c for _, c in Lc.CLASS_SETS]
    assert any(len(units) == 8 for _, units in tasks) and {len(s) for s, _ in tasks} >= {0, 2}
    recs, _, _ = _check(gpu, tasks)
    flags = [int(f) for f in recs["flags"]]
    assert flags.count(0) > 120 and flags.count(abi.LOCUS_NONE) >= 2 * len(Lc.CLASS_SETS)
    assert (recs["switches"] > 0).sum() > 60 and (recs["edits"] > 0).sum() > 40
    has = recs["flags"] == 0                                               # tracts begin and end on both sides of a 16-byte load
    assert {0, 1, 15, 16, 17} <= {int(b) for b in recs["begin"][has]} and {0, 1, 15} <= {int(e) % 16 for e in recs["end"][has]}


def test_random_set_and_task_order(gpu):
    tasks = Lc.random_set() + Lc.tiny_set(n=60)
    res = _check(gpu, tasks)
    perm = np.random.default_rng(3).permutation(len(tasks))
    per = _per_task(res)
    assert _per_task(_run(gpu, [tasks[i] for i in perm])) == [per[i] for i in perm]


# ---------------------------------------------------------------------------------------------- 2: one wave, unequal neighbours
@pytest.mark.parametrize("lens", [[3], [1, 3], [3, 5]])                     # sixteen tasks in one wave (twice), eight to a wave
def test_one_wave_of_unequal_neighbours(gpu, lens):
    rng = np.random.default_rng(97)
    units = [Cs.rs(rng, p) for p in lens]
    tasks = Lc.one_wave_batch(units)
    ln = sorted(len(s) for s, _ in tasks)
    assert len(tasks) == 16 and ln[:4] == [0, 1, 2, 5] and ln[-1] >= 3000 and all(35 <= x <= 75 for x in ln[4:15])
    per = _per_task(_check(gpu, tasks))
    long = max(range(16), key=lambda t: len(tasks[t][0]))
    assert _per_task(_run(gpu, [tasks[long]])) == [per[long]]                # alone in its wave or beside finished neighbours


# ---------------------------------------------------------------------------------------------- 3: one unit is the tract mode
def test_one_unit_against_the_tract_mode(gpu):
    pairs = Tc.random_set(n=120) + [(s, u) for s, u, _ in Tc.TABLE] + Tc.one_wave_batch(7)
    recs, _, _ = _check(gpu, [(s, [u]) for s, u in pairs])
    seqs, units, ts, tu = Tc.pack(pairs)
    tr = gpu.tract_batch(*abi.pack_seqs(seqs), units, ts, tu)
    for f, g in (("score", "score"), ("begin", "begin"), ("end", "end"), ("edits", "edits"), ("unit_bases", "unit_bases")):
        assert np.array_equal(recs[f], tr[g]), f
    assert np.array_equal(recs["flags"] == abi.LOCUS_NONE, tr["flags"] == abi.TRACT_NONE) and (recs["flags"] == 0).sum() > 80


# ---------------------------------------------------------------------------------------------- 4: the switches
@pytest.mark.parametrize("switch", ["OTG_LOCUS_WIDE", "OTG_LOCUS_SEG64"])
def test_switch_in_a_fresh_process(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("OTG_LOCUS_")}
    env[switch] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "locus_switch_child.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- 5: min_score and other scores
def test_min_score_at_a_tracts_score(gpu):
    rng = np.random.default_rng(5)
    u40 = Cs.rs(rng, 40)
    tasks = [Lc.TABLE[0][:2], Lc.TABLE[4][:2], Lc.TABLE[3][:2], (b"TTT" + u40 * 3 + b"CAGCAG" + b"GG", [u40, b"CAG"])]
    for s, units in tasks:
        score = ref(s, units, (2, 7, 7, 0))[0][0]
        assert score > 0
        for ms, none in ((score - 1, False), (score, False), (score + 1, True)):
            recs, seg_off, segs = _run(gpu, [(s, units)], (2, 7, 7, ms))
            Lc.check(recs[0], segs, ref(s, units, (2, 7, 7, ms)))
            assert (int(recs[0]["flags"]) == abi.LOCUS_NONE) == none and int(recs[0]["score"]) == score and (len(segs) == 0) == none, (s, units, ms)


@pytest.mark.parametrize("scores", [(1, 1, 1, 5), (16, 64, 64, 100), (3, 2, 5, 0)])
def test_other_scores(gpu, scores):
    rng = np.random.default_rng(97)
    _check(gpu, Lc.edge_set()[::3] + Lc.random_set(n=80) + Lc.one_wave_batch([Cs.rs(rng, 3), Cs.rs(rng, 5)]), scores)
    for bad in (dict(match=0), dict(match=17), dict(mismatch=0), dict(mismatch=65), dict(indel=0), dict(indel=65), dict(min_score=(1 << 24) + 1)):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.locus_batch(*abi.pack_seqs([b"CAG" * 20]), [[b"CAG"]], [0], [0], **bad)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), bad


# ---------------------------------------------------------------------------------------------- 6: the boundary between the key widths
@pytest.mark.parametrize("p", [37, 256])
def test_tier_boundary(gpu, p):
    N = R.narrow_len(2, 7, p)
    assert 31000 < N < 33000
    at, noisy = Lc.bound_set(p, N)[::2]                                     # a pure repeat (the score field at its largest) and noisy tracts
    units = at[1]
    assert max(len(u) for u in units) == p and len(at[0]) == len(noisy[0]) == N
    small = (b"GATTACA" + b"CAG" * 9 + b"TT", [b"CAG"])
    over = (Uc.repeat_from(units[-1], 5 % p, N + 1), units)
    for tasks, tiers in (([small, at, noisy], (3, 0)), ([small, over], (1, 1))):
        recs, _, _ = _check(gpu, tasks)
        assert gpu.locus_last_tiers() == tiers                             # at the bound: narrow; one base over: wide
        assert tuple(int(x) for x in recs[1])[:4] == (2 * len(tasks[1][0]), 0, len(tasks[1][0]), 0)
    assert int(recs[1]["score"]) == 2 * (N + 1) > 65535 - (p - 1) * 7      # (the narrow score field could not have held its biased cells)


# ---------------------------------------------------------------------------------------------- 7: the length cap and the refusals
def test_length_cap(gpu):
    too_long = np.tile(np.frombuffer(b"CAG", dtype=np.uint8), abi.LOCUS_MAX_LEN // 3 + 2)[:abi.LOCUS_MAX_LEN + 1].tobytes()
    tasks = [Lc.TABLE[0][:2], (too_long, [b"CAG", b"CCG"]), Lc.TABLE[3][:2], (b"", [b"CAG"]), Lc.TABLE[1][:2]]
    recs, seg_off, segs = _run(gpu, tasks)
    assert tuple(int(x) for x in recs[1]) == (0,) * 7 + (abi.LOCUS_TOO_LONG,) and tuple(int(x) for x in recs[3]) == (0,) * 7 + (abi.LOCUS_NONE,)
    assert seg_off[1] == seg_off[2] and seg_off[3] == seg_off[4] and gpu.locus_last_tiers() == (3, 0)
    for t in (0, 2, 4):
        Lc.check(recs[t], segs[int(seg_off[t]):int(seg_off[t + 1])], ref(*tasks[t]))


def test_refusals_on_the_device(gpu):
    arena, off, ln = abi.pack_seqs([b"CAG" * 20, b"ACGT" * 50])
    wide = [b"A" * 256, b"C" * 4]                                            # 64 + 1 lanes at four positions each
    for sets, ts, tq in (([[b"CAG"]], [2], [0]), ([[b"CAG"]], [0], [1]), ([[b"A" * 257]], [0], [0]), ([[]], [0], [0]), ([[b"CAG", b""]], [0], [0]),
                         ([[b"A"] * 9], [0], [0]), ([wide], [0], [0]), ([], [0], [0])):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.locus_batch(arena, off, ln, sets, ts, tq)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "otg_locus_batch" in str(e.value), (sets, ts, tq)
    with pytest.raises(otter_amd.OtterGpuError, match="does not fit one wave"):
        gpu.locus_batch(arena, off, ln, [wide], [0], [0])
    with otter_amd.Context(0) as fresh:
        assert _no_locus_results(fresh)


# ---------------------------------------------------------------------------------------------- 8: results in HBM, the unit parse beside them
def test_device_tensors_and_the_unit_parse_beside_them(gpu):
    import torch
    tasks = Lc.random_set(n=50) + [(b"", [b"CAG"]), (b"ACGTTGCA", [b"CAG", b"CCG"])]
    n = len(tasks)
    seqs, sets, ts, tq = Lc.pack(tasks)
    arena, off, ln = abi.pack_seqs(seqs)
    before = gpu.unitparse_batch(arena, off, ln, sets, ts, tq)
    recs, seg_off, segs = gpu.locus_batch(arena, off, ln, sets, ts, tq)
    d_recs, d_off, d_segs = gpu.locus_batch(arena, off, ln, sets, ts, tq, device_tensor=True)
    assert d_recs.device == torch.device("cuda", gpu.device) and d_recs.dtype == torch.int32 and tuple(d_recs.shape) == (n, 8) and tuple(d_segs.shape) == (len(segs), 6)
    assert np.array_equal(d_recs.cpu().numpy().astype(np.uint32), recs.view(np.uint32).reshape(-1, 8))
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), seg_off)
    assert np.array_equal(d_segs.cpu().numpy().astype(np.uint32), segs.view(np.uint32).reshape(-1, 6))
    # the call counts as a unit parse on the context: the summaries of the sub-rows, the segments in allele coordinates
    u_sums, u_off, u_segs = _unitparse_device(gpu, n)
    u_sums = u_sums.cpu().numpy().astype(np.uint32)
    assert np.array_equal(u_off.cpu().numpy().astype(np.uint64), seg_off) and np.array_equal(u_segs.cpu().numpy().astype(np.uint32), segs.view(np.uint32).reshape(-1, 6))
    has = recs["flags"] == 0
    assert has.sum() > 25 and (~has).sum() >= 2
    assert np.array_equal(u_sums[:, :4], np.stack([recs["edits"], recs["switches"], recs["unit_bases"], recs["n_segments"]], axis=1)) and not u_sums[~has].any()
    for i in np.flatnonzero(has)[:10]:
        s, units = tasks[i]
        want, _ = Pc_ref(s[int(recs[i]["begin"]):int(recs[i]["end"])], units)
        assert tuple(int(x) for x in u_sums[i])[:7] == want
    # and either operator still returns what it returned before
    again = gpu.unitparse_batch(arena, off, ln, sets, ts, tq)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, before))
    assert _no_locus_results(gpu)                                          # a unit parse of its own ends the locus results: the segments were its slot's
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gpu.locus_batch(arena, off, ln, sets, ts, tq), (recs, seg_off, segs)))
    e = _run(gpu, [], device_tensor=True)
    assert tuple(e[0].shape) == (0, 8) and tuple(e[1].shape) == (1,) and tuple(e[2].shape) == (0, 6)


def Pc_ref(s, units):
    import unitparse_ref
    return unitparse_ref.unitparse_np(s, units)


def _unitparse_device(gpu, n):
    """what otg_unitparse_device_results holds on the context, as device tensors"""
    m, t, ps, po, pg = C.c_uint32(0), C.c_uint64(0), C.c_void_p(), C.c_void_p(), C.c_void_p()
    gpu._check(gpu._L.otg_unitparse_device_results(gpu._h, C.byref(m), C.byref(ps), C.byref(po), C.byref(pg), C.byref(t)), "otg_unitparse_device_results")
    assert m.value == n and t.value > 0
    return gpu._wrap_device(ps.value, (n, 8), "<i4"), gpu._wrap_device(po.value, (n + 1,), "<i8"), gpu._wrap_device(pg.value, (t.value, 6), "<i4")


def _no_locus_results(ctx):
    rc = ctx._L.otg_locus_device_results(ctx._h, None, None, None, None, None)
    return rc == abi.OTG_ERR_ARG and ctx._L.otg_locus_collect(ctx._h, None, C.c_uint64(0)) == abi.OTG_ERR_ARG


# ---------------------------------------------------------------------------------------------- 9: the cohort rows
def test_cohort_rows(gpu):
    B, S = 4, 2
    P = abi.default_params(max_alleles=4)
    other = otter_amd.Context(0)
    try:
        gpu.cohort_begin(B, S)
        for k in range(S):                                                 # staged as tests/test_gpu_unitparse.py stages them
            b = synth.make_batch(B, len_range=(150, 400), reads_range=(8, 14), err="hifi", seed=911 + k, frac_partial=0.1, frac_het=0.8)
            ctx = other if (k % 2) else gpu
            ctx.assemble_submit(P, b)
            ctx.assemble_run()
            ctx.assemble_collect()
            gpu.cohort_stage(k, src=ctx)
    finally:
        other.close()
    rng = np.random.default_rng(4)
    units = [Cs.rs(rng, int(rng.integers(2, 7))) for _ in range(B)]
    refs = [Cs.rs(rng, 9) + Cs.substitute(rng, units[k] * int(rng.integers(20, 40)), 2) + units[(k + 1) % B] * 6 + Cs.rs(rng, 11) for k in range(B)]
    gpu.cohort_regroup(*abi.pack_seqs(refs))
    sets = [[units[0], units[1]], [b"CAG"], [units[2], b"T", units[3]]]
    with pytest.raises(otter_amd.OtterGpuError, match="has not been clustered"):
        gpu.cohort_loci(sets, [0], [0])
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    rows = gpu.cohort_kmer_rows()
    n = rows["n_rows"]
    seqs = M.row_seqs(rows, got)
    assert n == len(seqs) >= 6
    ts = np.repeat(np.arange(n - 1, dtype=np.uint32), 3)
    tq = np.tile(np.arange(3, dtype=np.uint32), n - 1)
    res = gpu.cohort_loci(sets, ts, tq, row_begin=1, min_score=16)
    arena, off, ln = abi.pack_seqs(seqs[1:])
    want = gpu.locus_batch(arena, off, ln, sets, ts, tq, min_score=16)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res, want)) and (res[0]["flags"] == 0).sum() >= 1
    for t in range(0, len(ts), 4):
        Lc.check(res[0][t], res[2][int(res[1][t]):int(res[1][t + 1])], ref(seqs[1 + int(ts[t])], sets[int(tq[t])], (2, 7, 7, 16)))
    dev = gpu.cohort_loci(sets, ts, tq, row_begin=1, min_score=16, device_tensor=True)
    assert np.array_equal(dev[0].cpu().numpy().astype(np.uint32), res[0].view(np.uint32).reshape(-1, 8))
    for kw in (dict(row_begin=n, n=1), dict(task_seq=[n]), dict(indel=0)):
        args = dict(unit_sets=sets, task_seq=[0], task_set=[0])
        args.update(kw)
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.cohort_loci(**args)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), kw
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
        gpu.cohort_loci(sets, [0], [0])


# ---------------------------------------------------------------------------------------------- 10: files and the tool
def _vcf_lines(rng):
    row = lambda i, ref_, alt: b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + ref_ + b"\t" + alt + b"\t.\tPASS\t.\tGT\t0/1"
    htt = Pc.HTT
    fl = lambda core: Cs.rs(rng, int(rng.integers(3, 30))) + core + Cs.rs(rng, int(rng.integers(3, 30)))
    return [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
            row(1, Lc.TABLE[0][0], Lc.TABLE[1][0] + b"," + Lc.TABLE[2][0].lower()),                                       # a region with two units
            row(2, b"GATTACA" * 9, fl(Pc.tracts(rng, [b"GATTACA"], 2, 9, 0.05)) + b",<DEL>"),                             # a name in column 4
            row(3, fl(htt[0] * 17 + htt[1] + htt[0] + htt[2] + htt[3] + htt[2] * 7 + htt[4] * 2),
                b",".join(fl(Pc.tracts(rng, htt, 5, 9, 0.04)) for _ in range(5))),                                        # the five HTT units; six alleles
            row(4, Cs.rs(rng, 60), b"AC"),                                                                                # one unit, lower case in the catalogue
            row(5, b"AC", b"."),                                                                                          # no BED record
            row(1, b"tt" + b"ccg" * 9 + b"cagcag" + b"a", b".")]                                                          # the region of the first line again


CATALOGUE = "chr1\t100\t150\tID=x;MOTIFS=CAG,CCG\nchr1\t200\t250\tlocus_two\nchr1\t300\t350\tCAG,CAA,CCG,CCA,CCT\nchr1\t400\t450\tacg\nchr1\t100\t150\tTTT\n"
BED_UNITS = {b"chr1:100-150": [b"CAG", b"CCG"], b"chr1:300-350": Pc.HTT, b"chr1:400-450": [b"acg"]}


def _expected_text(lines, scores=R.DEFAULT):
    out = []
    for l in lines:
        if not l or l.startswith(b"#"):
            continue
        f = l.split(b"\t")
        alleles = [f[3]]
        if len(f) > 4 and f[4] != b".":
            alleles += [b"N"] if f[4] == b"<DEL>" else f[4].split(b",")      # (a <DEL> beside other alleles is read as its five bytes)
        for i, a in enumerate(alleles):
            units = BED_UNITS.get(f[2], [])
            rec, segs = ref(a, units, scores) if units else ((0,) * 8, [])
            out.append(R.row(f[2], i, len(a), units, rec, segs))
    return b"".join(out)


def test_files_and_tool(gpu, tmp_path):
    lines = _vcf_lines(np.random.default_rng(71))
    plain, gz, bed = str(tmp_path / "calls.vcf"), str(tmp_path / "calls.vcf.gz"), str(tmp_path / "catalogue.bed")
    open(plain, "wb").write(b"\n".join(lines) + b"\n")
    with gzip.GzipFile(gz, "wb", mtime=0) as f:
        f.write(b"\n".join(lines))                                         # the last line has no '\n'
    open(bed, "w").write(CATALOGUE)
    want = _expected_text(lines)
    assert want.count(b"\n") == 3 + 3 + 6 + 2 + 1 + 1
    assert b"chr1:100-150\t0\t95\tCAG,CCG\t7\t88\t162\t0\t1\t81\t1.0000\t20.00,7.00\t(CAG)20(CCG)7\n" in want      # the first row of the table
    assert b"chr1:100-150\t1\t96\tCAG,CCG\t7\t89\t155\t1\t1\t81\t0.9878\t20.00,7.00\t(CAG)20~1(CCG)7\n" in want
    assert b"chr1:100-150\t2\t77\tCAG,CCG\t7\t70\t126\t0\t2\t63\t1.0000\t20.00,1.00\t(CAG)10(CCG)1(CAG)10\n" in want
    assert b"chr1:100-150\t0\t36\tCAG,CCG\t2\t35\t66\t0\t1\t33\t1.0000\t2.00,9.00\t(CCG)9(CAG)2\n" in want
    assert b"chr1:500-550\t0\t2\t.\t0\t0\t0\t0\t0\t0\t0.0000\t.\t.\n" in want and b"\tTTT\t" not in want
    assert want.count(b"\t.\t0\t0\t0\t0\t0\t0\t0.0000\t.\t.\n") == 4
    text, st = otter_amd.loci_files(gz, bed)
    assert text == want and st["n_regions"] == 6 and st["n_alleles"] == 16 and st["output_bytes"] == len(want)
    for batch, threads in ((2, 1), (5, 2)):                                 # batches smaller than the six-allele record
        assert otter_amd.loci_files(plain, bed, batch_alleles=batch, threads=threads)[0] == want, (batch, threads)
    other = (3, 2, 5, 40)
    assert otter_amd.loci_files(plain, bed, **_kw(other))[0] == _expected_text(lines, other) != want
    r = subprocess.run([CLI, "-b", bed, "-t", "2", "--batch", "3", gz], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = subprocess.run([CLI, "-b", bed, "--scores", "3,2,5", "--min-score=40", "--batch", "7", plain], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == _expected_text(lines, other), r.stderr
    wide = str(tmp_path / "wide.bed")
    open(wide, "w").write("chr1\t100\t150\t" + "A" * 256 + ",CCGG\n")
    with pytest.raises(otter_amd.OtterGpuError, match="chr1:100-150 do not fit one wave") as e:
        otter_amd.loci_files(plain, wide)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)

"""GPU: alleles parsed against sets of repeat units (otg_unitparse_batch / _cohort / otg_unitparse_files, tools/otter_unitparse).  Summaries
and segments must equal tests/unitparse_ref.py (the rule of include/otter_gpu.h restated in plain Python) record for record and segment for
segment, on shapes chosen where the kernel can go wrong: every lane layout, units across lanes 16 and 32, unequal neighbours in a wave,
alleles with edits (the tie order of the traceback bits), the chunks of the traceback store."""
import gzip
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, synth
import cohort_matrix_helpers as M
import motif_cases as Cs
import unitalign_ref as Ua
import unitparse_cases as Uc
import unitparse_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "otter_unitparse")
_REF = {}


def ref(s, units):
    key = (s, tuple(units))
    if key not in _REF:
        _REF[key] = R.unitparse_np(s, units)
    return _REF[key]


def _run(gpu, tasks, **kw):
    seqs, sets, ts, tq = Uc.pack(tasks)
    arena, off, ln = abi.pack_seqs(seqs)
    return gpu.unitparse_batch(arena, off, ln, sets, ts, tq, **kw)


def _check(gpu, tasks):
    sums, seg_off, segs = _run(gpu, tasks)
    assert sums.shape == (len(tasks),) and seg_off.shape == (len(tasks) + 1,) and seg_off[0] == 0 and int(seg_off[-1]) == len(segs)
    for t, (s, units) in enumerate(tasks):
        try:
            Uc.check(sums[t], segs[int(seg_off[t]):int(seg_off[t + 1])], ref(s, units))
        except AssertionError:
            raise AssertionError((t, s[:100], [u[:40] for u in units], sums[t], segs[int(seg_off[t]):int(seg_off[t + 1])], ref(s, units)))
    return sums, seg_off, segs


def _per_task(res):
    sums, seg_off, segs = res
    return [(sums[t].tobytes(), segs[int(seg_off[t]):int(seg_off[t + 1])].tobytes()) for t in range(len(sums))]


# ---------------------------------------------------------------------------------------------- 1: the table and every lane layout
def test_table(gpu):
    tasks = [(s, u) for s, u, _, _, _ in Uc.TABLE]
    sums, seg_off, segs = _check(gpu, tasks)
    for t, (_, _, key, want_segs, end) in enumerate(Uc.TABLE):
        assert (int(sums[t]["edits"]), int(sums[t]["switches"]), int(sums[t]["unit_bases"])) == key
        assert (int(sums[t]["end_unit"]), int(sums[t]["end_phase"])) == end
        got = [tuple(int(x) for x in g) for g in segs[int(seg_off[t]):int(seg_off[t + 1])]]
        assert len(got) == want_segs if isinstance(want_segs, int) else got == want_segs
    fwd, back = gpu.unitparse_last_ms()
    assert fwd > 0 and back > 0
    empty = _run(gpu, [])
    assert empty[0].shape == (0,) and list(empty[1]) == [0] and empty[2].shape == (0,)


def test_every_lane_layout(gpu):
    tasks = Uc.layout_set()
    per = len(tasks) // len(Uc.LAYOUTS)
    for i, (lens, lanes, regs) in enumerate(Uc.LAYOUTS):                    # the layouts are the ones they are listed as
        assert [len(u) for u in tasks[i * per][1]] == lens
        r = next(r for r in (1, 2, 4) if sum(-(-p // r) for p in lens) <= 64)
        need = sum(-(-p // r) for p in lens)
        assert r == regs and (lanes == 64 if r > 1 else lanes // 2 < max(need, 3) <= lanes)
    assert {(l, r) for _, l, r in Uc.LAYOUTS} == {(4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    assert any(len(u) == 256 for _, us in tasks for u in us) and any(len(us) == 8 for _, us in tasks) and any(us[0] == us[1] for _, us in tasks if len(us) > 1)
    assert {len(s) for s, _ in tasks} >= {0, 1, 15, 16, 17, 300}
    sums, _, _ = _check(gpu, tasks)
    assert (sums["switches"] > 0).sum() > 20 and (sums["edits"] > 0).sum() > 60


# ---------------------------------------------------------------------------------------------- 2: edits, ties, duplicates, task order
def test_random_sets_and_task_order(gpu):
    tasks = Uc.random_set() + Uc.tiny_set(100)
    res = _check(gpu, tasks)
    dup = [t for t, (_, us) in enumerate(tasks) if len(us) > 1 and us[-1] == us[0]]
    assert len(dup) > 20 and all(int(g["unit"]) != len(tasks[t][1]) - 1 for t in dup for g in res[2][int(res[1][t]):int(res[1][t + 1])])      # the lower index wins
    perm = np.random.default_rng(3).permutation(len(tasks))
    per = _per_task(res)
    assert _per_task(_run(gpu, [tasks[i] for i in perm])) == [per[i] for i in perm]


def test_unequal_neighbours_share_a_wave(gpu):
    tasks = Uc.shared_wave_set()
    assert len({len(us) for _, us in tasks}) >= 4 and len({len(s) for s, _ in tasks}) > 40
    per = _per_task(_check(gpu, tasks))
    long = max(range(len(tasks)), key=lambda t: len(tasks[t][0]))
    assert _per_task(_run(gpu, [tasks[long]])) == [per[long]]                # alone in its wave or beside finished neighbours


def test_one_long_allele(gpu):
    rng = np.random.default_rng(8)
    units = [b"CAG", b"CCG", b"CAA"]
    s = b"".join(Uc.tracts(rng, units, 40, 40, 0.01) for _ in range(20))[:40001]
    assert len(s) == 40001
    sums, _, segs = _check(gpu, [(s, units), (s[:77], units)])
    assert int(sums[0]["n_segments"]) > 100 and int(segs[int(sums[0]["n_segments"]) - 1]["end"]) == 40001


def test_one_unit_is_the_unit_alignment(gpu):
    rng = np.random.default_rng(12)
    tasks = []
    for p in (1, 2, 3, 5, 7, 16, 17, 33, 64, 65, 130, 256):
        u = Uc.rs(rng, p)
        tasks += [(Uc.tracts(rng, [u], 3, max(1, 90 // p), 0.1)[:200], [u]) for _ in range(3)]
    sums, seg_off, segs = _check(gpu, tasks)
    seqs, sets, ts, tq = Uc.pack(tasks)
    arena, off, ln = abi.pack_seqs(seqs)
    one = gpu.unitalign_batch(arena, off, ln, [q[0] for q in sets], ts, tq)
    for t in range(len(tasks)):
        assert (int(sums[t]["edits"]), int(sums[t]["unit_bases"]), int(sums[t]["end_phase"])) == tuple(int(x) for x in one[t])[:3], t
        assert (int(sums[t]["edits"]), int(sums[t]["unit_bases"]), int(sums[t]["end_phase"]), 0) == Ua.unitalign_np(*[tasks[t][0], tasks[t][1][0]])
        assert int(sums[t]["switches"]) == 0 and int(sums[t]["n_segments"]) == (1 if tasks[t][0] else 0)


# ---------------------------------------------------------------------------------------------- 3: the bounds and the refusals
def test_too_long_leaves_the_batch_intact(gpu):
    L = abi.UNITPARSE_MAX_LEN
    units = [b"A", b"C"]
    tasks = [(b"A" * (L + 1), units), (b"CAG" * 9, [b"CAG"]), (b"A" * L, units), (b"", units)]
    sums, seg_off, segs = _run(gpu, tasks)
    zero = (0, 0, 0, 0, 0, 0)
    assert tuple(int(x) for x in sums[0]) == zero + (abi.UNITPARSE_TOO_LONG, 0) and tuple(int(x) for x in sums[3]) == zero + (0, 0)
    Uc.check(sums[1], segs[int(seg_off[1]):int(seg_off[2])], ref(*tasks[1]))
    # the longest allele the key carries: L unit bases, no edit
    assert tuple(int(x) for x in sums[2]) == (0, 0, L, 1, 0, 0, 0, 0)
    assert list(seg_off) == [0, 0, 1, 2, 2] and tuple(int(x) for x in segs[1]) == (0, 0, L, L, 0, 0)


def test_refusals_on_the_device(gpu):
    arena, off, ln = abi.pack_seqs([b"CAG" * 20, b"ACGT" * 50])
    wide = [b"A" * 256, b"C" * 4]                                            # 64 + 1 lanes at four positions each
    fits = [b"A" * 252, b"C" * 4]
    ok = gpu.unitparse_batch(arena, off, ln, [[b"CAG"], fits], [0, 1], [0, 1])
    assert tuple(int(x) for x in ok[0][0])[:4] == (0, 0, 60, 1)
    Uc.check(ok[0][1], ok[2][int(ok[1][1]):int(ok[1][2])], ref(b"ACGT" * 50, fits))
    for sets, ts, tq in (([[b"CAG"]], [2], [0]), ([[b"CAG"]], [0], [1]), ([[b"A" * 257]], [0], [0]), ([[]], [0], [0]), ([[b"CAG"], []], [0], [0]),
                         ([[b"CAG", b""]], [0], [0]), ([[b"A"] * 9], [0], [0]), ([wide], [0], [0]), ([], [0], [0])):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.unitparse_batch(arena, off, ln, sets, ts, tq)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), (sets, ts, tq)
    with pytest.raises(otter_amd.OtterGpuError, match="does not fit one wave"):
        gpu.unitparse_batch(arena, off, ln, [wide], [0], [0])
    with pytest.raises(otter_amd.OtterGpuError) as e:
        gpu.unitparse_batch(arena, np.array([arena.size, 0], dtype=np.uint64), ln, [[b"CAG"]], [0], [0])
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)


# ---------------------------------------------------------------------------------------------- 4: the chunks of the traceback store
def test_trace_budget_in_a_fresh_process():
    out = {}
    for mb in ("1", "64"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("OTG_UNITPARSE_")}
        env["OTG_UNITPARSE_TRACE_MB"] = mb
        env["OTG_NO_TORCH_PRELOAD"] = "1"                                  # the child takes numpy arrays only
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unitparse_trace_child.py")], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.startswith("ok 1452 "), (r.stdout[-2000:], r.stderr[-2000:])
        out[mb] = r.stdout
    assert out["1"] == out["64"]


# ---------------------------------------------------------------------------------------------- 5: results in HBM, the cohort rows
def test_device_tensors(gpu):
    tasks = Uc.shared_wave_set()[:60]
    sums, seg_off, segs = _run(gpu, tasks)
    d_sums, d_off, d_segs = _run(gpu, tasks, device_tensor=True)
    assert d_sums.is_cuda and tuple(d_sums.shape) == (60, 8) and tuple(d_segs.shape) == (len(segs), 6)
    assert np.array_equal(d_sums.cpu().numpy().astype(np.uint32), sums.view(np.uint32).reshape(-1, 8))
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), seg_off)
    assert np.array_equal(d_segs.cpu().numpy().astype(np.uint32), segs.view(np.uint32).reshape(-1, 6))
    e = _run(gpu, [], device_tensor=True)
    assert tuple(e[0].shape) == (0, 8) and tuple(e[1].shape) == (1,) and tuple(e[2].shape) == (0, 6)


def test_cohort_rows(gpu):
    B, S = 4, 3
    P = abi.default_params(max_alleles=4)
    other = otter_amd.Context(0)
    try:
        gpu.cohort_begin(B, S)
        for k in range(S):                                                 # staged as tests/test_gpu_unitalign.py stages them
            b = synth.make_batch(B, len_range=(150, 400), reads_range=(8, 14), err="hifi", seed=911 + k, frac_partial=0.1, frac_het=0.8)
            ctx = other if (k % 2) else gpu
            ctx.assemble_submit(P, b)
            ctx.assemble_run()
            ctx.assemble_collect()
            gpu.cohort_stage(k, src=ctx)
    finally:
        other.close()
    rng = np.random.default_rng(4)
    refs = [Cs.substitute(rng, Cs.rs(rng, int(rng.integers(2, 7))) * int(rng.integers(30, 60)), 2) for _ in range(B)]
    gpu.cohort_regroup(*abi.pack_seqs(refs))
    sets = [[refs[0][:4], b"AC"], [b"CAG"], [b"ACGTTGCA", b"T", b"GGC"]]
    with pytest.raises(otter_amd.OtterGpuError, match="has not been clustered"):
        gpu.cohort_unitparse(sets, [0], [0])
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    rows = gpu.cohort_kmer_rows()
    n = rows["n_rows"]
    seqs = M.row_seqs(rows, got)
    assert n == len(seqs) >= 8
    ts = np.repeat(np.arange(n - 1, dtype=np.uint32), 3)
    tq = np.tile(np.arange(3, dtype=np.uint32), n - 1)
    res = gpu.cohort_unitparse(sets, ts, tq, row_begin=1)
    arena, off, ln = abi.pack_seqs(seqs[1:])
    want = gpu.unitparse_batch(arena, off, ln, sets, ts, tq)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res, want))
    for t in range(0, len(ts), 5):
        Uc.check(res[0][t], res[2][int(res[1][t]):int(res[1][t + 1])], ref(seqs[1 + int(ts[t])], sets[int(tq[t])]))
    dev = gpu.cohort_unitparse(sets, ts, tq, row_begin=1, device_tensor=True)
    assert np.array_equal(dev[2].cpu().numpy().astype(np.uint32), want[2].view(np.uint32).reshape(-1, 6))
    for kw in (dict(unit_sets=sets, task_seq=[0], task_set=[0], row_begin=n, n=1), dict(unit_sets=sets, task_seq=[n], task_set=[0]),
               dict(unit_sets=sets, task_seq=[0], task_set=[3]), dict(unit_sets=[[b"A" * 257]], task_seq=[0], task_set=[0]),
               dict(unit_sets=[[]], task_seq=[0], task_set=[0])):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.cohort_unitparse(**kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), kw
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
        gpu.cohort_unitparse(sets, [0], [0])


# ---------------------------------------------------------------------------------------------- 6: files and the tool
def _vcf_lines(rng):
    row = lambda i, ref_, alt: b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + ref_ + b"\t" + alt + b"\t.\tPASS\t.\tGT\t0/1"
    htt = Uc.HTT
    return [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
            row(1, b"CAG" * 20 + b"CCG" * 10, b"CAG" * 10 + b"T" + b"CAG" * 10 + b"CCG" * 7 + b"," + b"CAG" * 17),      # a region with two units
            row(2, b"GATTACA" * 9, Uc.tracts(rng, [b"GATTACA"], 2, 9, 0.05) + b",<DEL>"),                                # a name in column 4
            row(3, htt[0] * 17 + htt[1] + htt[0] + htt[2] + htt[3] + htt[2] * 7 + htt[4] * 2,
                b",".join(Uc.tracts(rng, htt, 5, 9, 0.04) for _ in range(5))),                                           # the five HTT units; six alleles
            row(4, Cs.rs(rng, 60), b"AC"),                                                                               # one unit, lower case in the catalogue
            row(5, b"AC", b"."),                                                                                         # no BED record
            row(1, b"ccg" * 9 + b"cagcag", b".")]                                                                        # the region of the first line again


CATALOGUE = "chr1\t100\t150\tID=x;MOTIFS=CAG,CCG\nchr1\t200\t250\tlocus_two\nchr1\t300\t350\tCAG,CAA,CCG,CCA,CCT\nchr1\t400\t450\tacg\nchr1\t100\t150\tTTT\n"
BED_UNITS = {b"chr1:100-150": [b"CAG", b"CCG"], b"chr1:300-350": Uc.HTT, b"chr1:400-450": [b"acg"]}


def _expected_text(lines):
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
            rec, segs = ref(a, units) if units else ((0,) * 7, [])
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
    assert b"chr1:100-150\t0\t90\tCAG,CCG\t0\t1\t90\t1.0000\t20.00,10.00\t(CAG)20(CCG)10\n" in want
    assert b"chr1:100-150\t1\t82\tCAG,CCG\t1\t1\t81\t0.9878\t20.00,7.00\t(CAG)20~1(CCG)7\n" in want
    assert b"chr1:300-350\t0\t90\tCAG,CAA,CCG,CCA,CCT\t0\t6\t90\t1.0000\t18.00,1.00,8.00,1.00,2.00\t(CAG)17(CAA)1(CAG)1(CCG)1(CCA)1(CCG)7(CCT)2\n" in want
    assert b"chr1:500-550\t0\t2\t.\t0\t0\t0\t0.0000\t.\t.\n" in want and b"chr1:100-150\t0\t33\tCAG,CCG\t0\t1\t33\t1.0000\t2.00,9.00\t(CCG)9(CAG)2\n" in want
    assert b"TTT" not in want and want.count(b"\t.\t0\t0\t0\t0.0000\t.\t.\n") == 4
    text, st = otter_amd.unitparse_files(gz, bed)
    assert text == want and st["n_regions"] == 6 and st["n_alleles"] == 16 and st["output_bytes"] == len(want)
    for batch, threads in ((2, 1), (1, 3), (5, 2)):                         # batches smaller than the six-allele record
        assert otter_amd.unitparse_files(plain, bed, batch_alleles=batch, threads=threads)[0] == want, (batch, threads)
    r = subprocess.run([CLI, "-b", bed, "-t", "2", "--batch", "3", gz], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    wide = str(tmp_path / "wide.bed")
    open(wide, "w").write("chr1\t100\t150\t" + "A" * 256 + ",CCGG\n")
    with pytest.raises(otter_amd.OtterGpuError, match="chr1:100-150 do not fit one wave") as e:
        otter_amd.unitparse_files(plain, wide)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    nine = str(tmp_path / "nine.bed")
    open(nine, "w").write("chr1\t100\t150\t" + ",".join(["CAG"] * 9) + "\n")
    with pytest.raises(otter_amd.OtterGpuError, match="chr1:100-150 has 9 units"):
        otter_amd.unitparse_files(plain, nine)

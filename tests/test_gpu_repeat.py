"""GPU: the repeat structure of alleles (otg_repeat_batch / otg_repeat_collect / otg_repeat_cohort / otg_repeats_files, tools/otter_repeats).
Summaries, offsets and segments must equal tests/repeat_ref.py (the rule of include/otter_gpu.h restated in plain Python) exactly, on shapes
chosen where the kernels can go wrong: word and carry edges of the run walk, the period range, nested horizons, the boundary between the LDS
and the HBM tier, the length cap."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, synth
import cohort_helpers as H
import cohort_matrix_helpers as M
import motif_cases as Cs
import repeat_cases as Rc
import repeat_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "otter_repeats")


def _same(res, seqs, par, exps=None):
    sums, seg_off, segs = res
    assert sums.shape == (len(seqs),) and seg_off.shape == (len(seqs) + 1,) and int(seg_off[0]) == 0 and segs.shape == (int(seg_off[-1]),)
    for i, s in enumerate(seqs):
        exp = exps[i] if exps else R.structure_cached(s, *par)
        assert int(seg_off[i + 1]) - int(seg_off[i]) == exp["n_segments"], (par, i, s[:100])
        assert Rc.as_tuples(sums, seg_off, segs, i) == exp["segs"], (par, i, s[:100], Rc.as_tuples(sums, seg_off, segs, i)[:8], exp["segs"][:8])
        assert tuple(int(x) for x in sums[i]) == (exp["n_segments"], exp["n_repeats"], exp["covered"], exp["flags"]), (par, i, s[:100])


def _check(gpu, seqs, par=(256, 2, 12)):
    res = gpu.repeat_batch(*abi.pack_seqs(seqs), *par)
    _same(res, seqs, par)
    return res


def test_literal_table(gpu):
    seqs = [t[0] for t in Rc.TABLE]
    sums, seg_off, segs = _check(gpu, seqs + [s.lower() for s in seqs])
    for i, (seq, want, _) in enumerate(Rc.TABLE):
        assert Rc.as_tuples(sums, seg_off, segs, i) == want == Rc.as_tuples(sums, seg_off, segs, i + len(seqs)), seq
    assert _check(gpu, [b"CAG" * 20], (2, 2, 12))[0]["n_repeats"][0] == 0


def test_edge_and_random_sets(gpu):
    seqs = Cs.edge_set() + Cs.random_set()
    _check(gpu, seqs)
    exps = [R.structure_cached(s) for s in seqs]
    assert sum(e["n_segments"] > 1 for e in exps) >= 150 and sum(e["moved"] for e in exps) >= 1


@pytest.mark.parametrize("max_period", Rc.EDGE_PERIODS)
def test_word_and_carry_edges(gpu, max_period):
    seqs = Rc.word_edge_set()
    for mc, ms in Rc.EDGE_ENOUGH:
        sums, _, segs = _check(gpu, seqs, (max_period, mc, ms))
        assert int(segs["period"].max()) <= max_period and (max_period < 63 or int(sums["n_repeats"].sum()) > 20)


def test_stack_depth(gpu):
    seq = Rc.deep_stack()
    exp = R.structure_cached(seq)
    assert exp["depth"] >= 3 and exp["n_repeats"] == 4
    _check(gpu, [b"CAG" * 20, seq, b"AC"])


def test_tier_boundary(gpu):
    """the LDS tier's limit, one below and one above (the HBM tier), between small neighbours"""
    rng = np.random.default_rng(17)
    lim = abi.MOTIF_LDS_LEN
    unit = Cs.rs(rng, 37)
    seqs = [b"CAG" * 20]
    for L in (lim - 1, lim, lim + 1):
        seqs += [Cs.substitute(rng, (unit * (L // 37 + 1))[:L], 40), Cs.rs(rng, 33)]
    sums, _, _ = _check(gpu, seqs, (64, 2, 12))
    assert all(int(sums[i]["n_repeats"]) >= 20 for i in (1, 3, 5))        # the substitutions cut the 37-base repeat into many segments


def test_force_hbm_tier_in_a_fresh_process():
    env = dict(os.environ, OTG_MOTIF_WIDE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "repeat_wide_child.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])


def test_length_cap(gpu):
    rng = np.random.default_rng(23)
    big = np.tile(np.frombuffer(b"ACGGT", dtype=np.uint8), abi.REPEAT_MAX_LEN // 5 + 1)
    too_long = big[:abi.REPEAT_MAX_LEN + 1].tobytes()
    longest = big[:abi.REPEAT_MAX_LEN].tobytes()
    seqs = [b"CAG" * 20, too_long, Cs.rs(rng, 77), longest, b"AAAG" * 25]
    sums, seg_off, segs = _check(gpu, seqs, (64, 2, 12))
    assert Rc.as_tuples(sums, seg_off, segs, 1) == [(0, 0, 0, abi.REPEAT_MAX_LEN + 1)] and tuple(int(x) for x in sums[1]) == (1, 0, 0, abi.REPEAT_TOO_LONG)
    assert Rc.as_tuples(sums, seg_off, segs, 3) == [(0, 5, 209715, 1048575)] and int(sums[3]["flags"]) == 0
    assert Rc.as_tuples(sums, seg_off, segs, 0) == [(0, 3, 20, 60)] and Rc.as_tuples(sums, seg_off, segs, 4) == [(0, 4, 25, 100)]


def test_results_in_hbm(gpu):
    import torch
    seqs = Cs.random_set(n=40) + [b"", b"A", b"AC"]
    arena, off, ln = abi.pack_seqs(seqs)
    sums, seg_off, segs = _check(gpu, seqs)
    r_ms, s_ms = gpu.repeat_last_ms()
    assert r_ms > 0 and s_ms > 0
    dsums, doff, dsegs = gpu.repeat_batch(arena, off, ln, device_tensor=True)
    dev = torch.device("cuda", gpu.device)
    assert dsums.device == dev and doff.device == dev and dsegs.device == dev
    assert (dsums.dtype, doff.dtype, dsegs.dtype) == (torch.int32, torch.int64, torch.int32)
    assert dsums.shape == (len(seqs), 4) and doff.shape == (len(seqs) + 1,) and dsegs.shape == (len(segs), 4)
    assert np.array_equal(dsums.cpu().numpy().astype(np.uint32), sums.view(np.uint32).reshape(-1, 4))
    assert np.array_equal(doff.cpu().numpy().astype(np.uint64), seg_off)
    assert np.array_equal(dsegs.cpu().numpy().astype(np.uint32), segs.view(np.uint32).reshape(-1, 4))
    assert [Rc.as_tuples(sums, seg_off, segs, len(seqs) - 3 + i) for i in range(3)] == [[], [(0, 0, 0, 1)], [(0, 0, 0, 2)]]
    e = np.zeros(0, dtype=np.uint8)
    s0, o0, g0 = gpu.repeat_batch(e, np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert s0.shape == (0,) and o0.tolist() == [0] and g0.shape == (0,)
    d0 = gpu.repeat_batch(e, np.zeros(0, np.uint64), np.zeros(0, np.uint32), device_tensor=True)
    assert d0[0].shape == (0, 4) and d0[1].cpu().tolist() == [0] and d0[2].shape == (0, 4)
    one = gpu.repeat_batch(*abi.pack_seqs([b""]))                          # a batch without a single segment
    assert one[0].tolist() == [(0, 0, 0, 0)] and one[1].tolist() == [0, 0] and one[2].shape == (0,)


def test_batch_order_and_repeatability(gpu):
    seqs = Cs.edge_set()[::2] + Cs.random_set(n=50)
    arena, off, ln = abi.pack_seqs(seqs)
    a = gpu.repeat_batch(arena, off, ln)
    b = gpu.repeat_batch(arena, off, ln)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    perm = np.random.default_rng(2).permutation(len(seqs))
    pseqs = [seqs[i] for i in perm]
    _same(gpu.repeat_batch(*abi.pack_seqs(pseqs)), pseqs, (256, 2, 12))
    o = gpu.repeat_batch(arena, off[perm], ln[perm])                       # the same arena read through permuted offsets, too
    _same(o, pseqs, (256, 2, 12))
    assert o[0].tobytes() == a[0][perm].tobytes()


def test_refusals_on_the_device(gpu):
    fresh = otter_amd.Context(0)
    try:
        assert fresh._L.otg_repeat_device_results(fresh._h, None, None, None, None, None) == abi.OTG_ERR_ARG      # before any call
        assert b"no repeat results" in fresh._L.otg_last_error(fresh._h)
        assert fresh._L.otg_repeat_collect(fresh._h, None, C.c_uint64(0)) == abi.OTG_ERR_ARG
    finally:
        fresh.close()
    arena, off, ln = abi.pack_seqs([b"CAG" * 20 + b"CCG" * 20, b"ACGT" * 50])
    for kw in (dict(max_period=0), dict(max_period=abi.REPEAT_MAX_PERIOD + 1), dict(min_copies=1), dict(min_copies=1025), dict(min_span=1), dict(min_span=65536)):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.repeat_batch(arena, off, ln, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    u = C.c_uint32
    bad = np.array([arena.size], dtype=np.uint64)
    assert gpu._L.otg_repeat_batch(gpu._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(bad), abi.ptr(ln), u(1), u(256), u(2), u(12), None, None, None) == abi.OTG_ERR_ARG
    assert b"outside" in gpu._L.otg_last_error(gpu._h)
    total = C.c_uint64(0)
    assert gpu._L.otg_repeat_batch(gpu._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(off), abi.ptr(ln), u(2), u(256), u(2), u(12), None, None, C.byref(total)) == 0
    assert total.value == 3
    segs = np.zeros(3, dtype=abi.repeat_seg_dt)
    assert gpu._L.otg_repeat_collect(gpu._h, abi.ptr(segs), C.c_uint64(2)) == abi.OTG_ERR_CAPACITY and b"3 segments" in gpu._L.otg_last_error(gpu._h)
    assert gpu._L.otg_repeat_collect(gpu._h, abi.ptr(segs), C.c_uint64(3)) == 0
    assert [tuple(int(x) for x in g) for g in segs] == [(0, 3, 20, 60), (60, 3, 20, 60), (0, 4, 50, 200)]


# ---------------------------------------------------------------------------------------------- cohort rows
def _stage(gpu, other):
    """3 samples over 4 regions, regrouped and clustered; every read of sample 1 in region 2 is empty (a whole-locus deletion): a zero-length
    allele.  -> (per-sample assemble results, reference alleles)"""
    B, S = 4, 3
    P = abi.default_params(max_alleles=4)
    gpu.cohort_begin(B, S)
    results = []
    for k in range(S):
        b = synth.make_batch(B, len_range=(150, 400), reads_range=(8, 14), err="hifi", seed=911 + k, frac_partial=0.1, frac_het=0.8)
        if k == 1:
            rg = b["regions"][2]
            sl = slice(int(rg["first_read"]), int(rg["first_read"]) + int(rg["n_reads"]))
            b["reads"]["seq_len"][sl] = 0
            b["reads"]["spanning_l"][sl] = 1; b["reads"]["spanning_r"][sl] = 1
            b["reads"]["ccoord_first"][sl] = 0; b["reads"]["ccoord_second"][sl] = 0
        ctx = other if (k % 2) else gpu
        ctx.assemble_submit(P, b)
        ctx.assemble_run()
        results.append(ctx.assemble_collect())
        gpu.cohort_stage(k, src=ctx)
    rng = np.random.default_rng(4)
    refs = [Cs.substitute(rng, Cs.rs(rng, int(rng.integers(2, 7))) * int(rng.integers(30, 60)), 2) for _ in range(B)]
    return P, results, refs


def test_cohort_rows(gpu):
    import torch
    other = otter_amd.Context(0)
    try:
        P, results, refs = _stage(gpu, other)
    finally:
        other.close()
    ref_arena, ref_off, ref_len = abi.pack_seqs(refs)
    gpu.cohort_regroup(ref_arena, ref_off, ref_len)
    with pytest.raises(otter_amd.OtterGpuError, match="has not been clustered") as e:
        gpu.cohort_repeats()
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    H.same_regroup(got, H.numpy_regroup(results, refs))
    rows = gpu.cohort_kmer_rows()
    n = rows["n_rows"]
    seqs = M.row_seqs(rows, got)
    assert n == len(seqs) >= 8 and seqs.count(b"N") == 1                  # the zero-length allele is the row of "N"
    res = gpu.cohort_repeats()
    _same(res, seqs, (256, 2, 12))
    sums, seg_off, segs = res
    assert Rc.as_tuples(sums, seg_off, segs, seqs.index(b"N")) == [(0, 0, 0, 1)] and (sums["n_repeats"] > 0).sum() >= n - 2
    host = gpu.repeat_batch(*abi.pack_seqs(seqs))                          # the same kernels on the same bytes uploaded from the host
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res, host))
    _same(gpu.cohort_repeats(2, 3), seqs[2:5], (256, 2, 12))
    _same(gpu.cohort_repeats(1, None, 64, 3, 20), seqs[1:], (64, 3, 20))
    dsums, doff, dsegs = gpu.cohort_repeats(1, device_tensor=True)
    assert dsums.device == torch.device("cuda", gpu.device) and np.array_equal(dsums.cpu().numpy().astype(np.uint32), sums[1:].view(np.uint32).reshape(-1, 4))
    assert np.array_equal(doff.cpu().numpy().astype(np.uint64), seg_off[1:] - seg_off[1])
    assert np.array_equal(dsegs.cpu().numpy().astype(np.uint32), segs[int(seg_off[1]):].view(np.uint32).reshape(-1, 4))
    assert gpu.cohort_repeats(n, 0)[0].shape == (0,)
    for args, kw in (((n, 1), {}), ((0, n + 1), {}), ((0, n), dict(max_period=0)), ((0, n), dict(min_copies=1)), ((0, n), dict(min_span=65536))):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.cohort_repeats(*args, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), (args, kw)
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
        gpu.cohort_repeats()


# ---------------------------------------------------------------------------------------------- files and the tool
def _vcf_lines(rng):
    rep = lambda u, c, sub=0: Cs.substitute(rng, Cs.rs(rng, u) * c, sub) if sub else Cs.rs(rng, u) * c
    row = lambda i, ref, alt: b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + ref + b"\t" + alt + b"\t.\tPASS\t.\tGT\t0/1"
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
             row(1, b"CAG" * 20 + b"CCG" * 20, b"CCG" * 20 + b"CAG" * 20 + b"," + rep(3, 17)),
             row(2, rep(5, 30), b"."), row(3, rep(4, 40, 2), b"<DEL>"), row(4, rep(2, 50), b"A,<DEL>"),
             row(5, rep(7, 12), b",".join(rep(7, c, c % 2) for c in (9, 14, 20, 26, 31))),            # six alleles: more than a batch of two
             b"# a comment in the body", row(6, Cs.rs(rng, 300), Cs.rs(rng, 40).lower() + b"," + rep(37, 6)), b"chr1\t700\tfour_columns\t" + rep(6, 9),
             row(8, b"acgtNNacgt" * 6, b"AC"), row(9, rep(300, 3), rep(1, 30))]
    return lines


def _expected_text(lines, par=(256, 2, 12)):
    out = []
    for l in lines:
        if not l or l.startswith(b"#"):
            continue
        f = l.split(b"\t")
        alleles = [f[3]]
        if len(f) > 4 and f[4] != b".":
            alleles += [b"N"] if f[4] == b"<DEL>" else f[4].split(b",")
        out += [R.row(f[2], i, a, R.structure_cached(a, *par)) for i, a in enumerate(alleles)]
    return b"".join(out)


def test_files_and_tool(gpu, tmp_path):
    lines = _vcf_lines(np.random.default_rng(9))
    plain, gz, bed = str(tmp_path / "calls.vcf"), str(tmp_path / "calls.vcf.gz"), str(tmp_path / "regions.bed")
    open(plain, "wb").write(b"\n".join(lines) + b"\n")
    with gzip.GzipFile(gz, "wb", mtime=0) as f:
        f.write(b"\n".join(lines))                                         # the last line has no '\n'
    open(bed, "w").write("chr1\t100\t150\n")
    want = _expected_text(lines)
    assert want.count(b"\n") == 23 and b"chr1:300-350\t1\t1\t0\t0\tN\n" in want
    assert want.startswith(b"chr1:100-150\t0\t120\t2\t120\t(CAG)20(CCG)20\nchr1:100-150\t1\t120\t2\t120\t(CCG)20(CAG)20\n")
    text, st = otter_amd.repeats_files(gz, bed)
    assert text == want and st["n_regions"] == 9 and st["n_alleles"] == 23 and st["output_bytes"] == len(want)
    for batch, threads in ((2, 1), (1, 3), (5, 2)):                         # batches smaller than the six-allele record
        assert otter_amd.repeats_files(plain, bed, batch_alleles=batch, threads=threads)[0] == want, (batch, threads)
    other = _expected_text(lines, (4, 3, 20))
    assert otter_amd.repeats_files(plain, bed, max_period=4, min_copies=3, min_span=20)[0] == other != want
    r = subprocess.run([CLI, "-b", bed, "-t", "2", "--batch", "3", gz], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = subprocess.run([CLI, "-b", bed, "-p", "4", "--min-copies", "3", "--min-span=20", plain], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == other, r.stderr
    for args in (["-p", "0"], ["--min-copies", "1"], ["--min-span", "65536"]):
        r = subprocess.run([CLI, "-b", bed] + args + [plain], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and b"[ERROR] invalid" in r.stderr, args

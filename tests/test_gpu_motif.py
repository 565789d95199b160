"""GPU: the tandem-repeat motif annotation (otg_motif_batch / otg_motif_cohort / otg_motifs_files, tools/otter_motifs).  Records and unit
bytes must equal tests/motif_ref.py (the rule of include/otter_gpu.h restated in plain Python) exactly, on shapes chosen where the kernels can
go wrong: word and lane edges, the period range, the masks, the boundary between the LDS and the HBM tier, the length cap."""
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
import motif_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "otter_motifs")
SUBST = b"CAG" * 10 + b"CTG" + b"CAG" * 9


def _check(gpu, seqs, max_period=256, slack=50):
    arena, off, ln = abi.pack_seqs(seqs)
    rec, units = gpu.motif_batch(arena, off, ln, max_period=max_period, slack=slack)
    assert rec.shape == (len(seqs),) and units.shape == (len(seqs), max(1, min(max_period, max(map(len, seqs)) // 2)))
    for i, s in enumerate(seqs):
        exp = R.motif_cached(s, max_period, slack)
        assert R.same(rec[i], units[i], exp), (max_period, slack, i, s[:100], rec[i], bytes(units[i])[:100], exp)
    return rec, units


def test_word_and_lane_edges_and_bytes(gpu):
    seqs = Cs.edge_set()
    rec, units = _check(gpu, seqs)
    assert set(int(p) for p in rec["period"]) >= {0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65}
    i = seqs.index(b"CAG" * 20)
    assert tuple(rec[i])[:4] == (3, 57, 57, 3) and bytes(units[i][:3]) == b"AGC"
    i = seqs.index(SUBST)
    assert tuple(rec[i])[:4] == (3, 55, 57, 30)
    c_ms, r_ms = gpu.motif_last_ms()
    assert c_ms > 0 and r_ms > 0


@pytest.mark.parametrize("max_period", [1, 2, 63, 64, 65])
def test_max_period(gpu, max_period):
    rec, _ = _check(gpu, Cs.edge_set()[::3] + [b"CAG" * 20, b"AAAG" * 25], max_period=max_period)
    assert int(rec["period"].max()) <= max_period
    if max_period <= 2:
        assert int(rec[-2]["period"]) == 0                                 # max_period below the true period: CAG has no match at 1 or 2


def test_max_period_4096(gpu):
    rng = np.random.default_rng(21)
    long = Cs.substitute(rng, Cs.rs(rng, 2900) * 3 + Cs.rs(rng, 300), 9)   # 9 000 bases, period 2 900: sixteen periods per thread, a unit beyond 256
    rec, _ = _check(gpu, [b"AC" * 9, long, Cs.rs(rng, 700) * 4], max_period=4096)
    assert len(long) == 9000 and int(rec[1]["period"]) == 2900 and int(rec[2]["period"]) == 700


def test_slack(gpu):
    seqs = Cs.edge_set()[::2] + [SUBST]
    rec0, _ = _check(gpu, seqs, slack=0)
    rec9, _ = _check(gpu, seqs, slack=999)
    assert int(rec0[-1]["period"]) == 30 and int(rec9[-1]["period"]) == 3
    assert np.array_equal(rec0["best_period"], rec9["best_period"])


def test_tier_boundary(gpu):
    """the LDS tier's limit, one below and one above (the HBM tier), between small neighbours"""
    rng = np.random.default_rng(17)
    lim = abi.MOTIF_LDS_LEN
    unit = Cs.rs(rng, 37)
    seqs = [b"CAG" * 20]
    for L in (lim - 1, lim, lim + 1):
        seqs += [Cs.substitute(rng, (unit * (L // 37 + 1))[:L], 40), Cs.rs(rng, 33)]
    seqs.append(Cs.rs(rng, lim + 1, b"ACGTN"))
    rec, _ = _check(gpu, seqs)
    assert [int(p) for p in rec["period"][1:7:2]] == [37, 37, 37]


def test_force_hbm_tier_in_a_fresh_process():
    env = dict(os.environ, OTG_MOTIF_WIDE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "motif_wide_child.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])


def test_length_cap(gpu):
    rng = np.random.default_rng(23)
    big = np.tile(np.frombuffer(b"ACGGT", dtype=np.uint8), abi.MOTIF_MAX_LEN // 5 + 1)
    too_long = big[:abi.MOTIF_MAX_LEN + 1].tobytes()
    longest = big[:abi.MOTIF_MAX_LEN].tobytes()
    seqs = [b"CAG" * 20, too_long, Cs.rs(rng, 77), longest, b"AAAG" * 25]
    arena, off, ln = abi.pack_seqs(seqs)
    rec, units = gpu.motif_batch(arena, off, ln, max_period=64)
    assert tuple(int(x) for x in rec[1]) == (0, 0, 0, 0, abi.MOTIF_TOO_LONG, 0) and not units[1].any()
    for i in (0, 2, 3, 4):
        assert R.same(rec[i], units[i], R.motif_cached(seqs[i], 64, 50)), i
    assert tuple(int(x) for x in rec[3])[:4] == (5, abi.MOTIF_MAX_LEN - 5, abi.MOTIF_MAX_LEN - 5, 5) and bytes(units[3][:5]) == b"ACGGT"


def test_random_batch(gpu):
    seqs = Cs.random_set()
    rec, _ = _check(gpu, seqs)
    assert len(seqs) == 300 and (rec["period"] != rec["best_period"]).sum() > 5 and (rec["period"] > 0).sum() > 250


def test_results_in_hbm(gpu):
    import torch
    seqs = Cs.random_set(n=40) + [b"", b"AC"]
    arena, off, ln = abi.pack_seqs(seqs)
    rec, units = gpu.motif_batch(arena, off, ln)
    drec, dunits = gpu.motif_batch(arena, off, ln, device_tensor=True)
    dev = torch.device("cuda", gpu.device)
    assert drec.device == dev and dunits.device == dev and drec.dtype == torch.int32 and dunits.dtype == torch.uint8
    assert drec.shape == (len(seqs), 6) and dunits.shape == units.shape
    assert np.array_equal(drec.cpu().numpy().astype(np.uint32), rec.view(np.uint32).reshape(-1, 6))
    assert np.array_equal(dunits.cpu().numpy(), units)
    e = np.zeros(0, dtype=np.uint8)
    rec0, units0 = gpu.motif_batch(e, np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert rec0.shape == (0,) and units0.shape == (0, 1)


def test_batch_order_and_repeatability(gpu):
    seqs = Cs.edge_set()[::2] + Cs.random_set(n=50)
    arena, off, ln = abi.pack_seqs(seqs)
    rec, units = gpu.motif_batch(arena, off, ln)
    rec2, units2 = gpu.motif_batch(arena, off, ln)
    assert rec.tobytes() == rec2.tobytes() and units.tobytes() == units2.tobytes()
    perm = np.random.default_rng(2).permutation(len(seqs))
    prec, punits = gpu.motif_batch(*abi.pack_seqs([seqs[i] for i in perm]))
    assert prec.tobytes() == rec[perm].tobytes() and punits.tobytes() == units[perm].tobytes()
    # the same arena read through permuted offsets, too
    orec, ounits = gpu.motif_batch(arena, off[perm], ln[perm])
    assert orec.tobytes() == rec[perm].tobytes() and ounits.tobytes() == units[perm].tobytes()


def test_refusals_on_the_device(gpu):
    arena, off, ln = abi.pack_seqs([b"CAG" * 20, b"ACGT" * 50])
    for kw in (dict(max_period=0), dict(max_period=abi.MOTIF_MAX_PERIOD + 1), dict(slack=1000)):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.motif_batch(arena, off, ln, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    rec = np.zeros(2, dtype=abi.motif_dt)
    units = np.zeros((2, 100), dtype=np.uint8)
    call = lambda stride, mp: gpu._L.otg_motif_batch(gpu._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(off), abi.ptr(ln), C.c_uint32(2), C.c_uint32(mp),
                                                     C.c_uint32(50), abi.ptr(rec), abi.ptr(units), C.c_uint32(stride))
    assert call(99, 256) == abi.OTG_ERR_ARG and b"unit_stride" in gpu._L.otg_last_error(gpu._h)      # min(256, 200 / 2) = 100
    assert call(100, 256) == 0 and call(7, 7) == 0 and call(6, 7) == abi.OTG_ERR_ARG
    bad = np.array([arena.size], dtype=np.uint64)
    assert gpu._L.otg_motif_batch(gpu._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(bad), abi.ptr(ln), C.c_uint32(1), C.c_uint32(256), C.c_uint32(50),
                                  abi.ptr(rec), abi.ptr(units), C.c_uint32(100)) == abi.OTG_ERR_ARG


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
        gpu.cohort_motifs()
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    H.same_regroup(got, H.numpy_regroup(results, refs))
    rows = gpu.cohort_kmer_rows()
    n = rows["n_rows"]
    seqs = M.row_seqs(rows, got)
    assert n == len(seqs) >= 8
    assert int(results[1]["regions"][2]["n_alleles"]) >= 1 and seqs.count(b"N") == 1      # the zero-length allele is the row of "N"
    rec, units = gpu.cohort_motifs()
    assert rec.shape == (n,) and units.shape == (n, 256)
    for i, s in enumerate(seqs):
        assert R.same(rec[i], units[i], R.motif_cached(s)), (i, s, rec[i])
    assert tuple(int(x) for x in rec[seqs.index(b"N")]) == (0, 0, 0, 0, 0, 0) and (rec["period"] > 0).sum() >= n - 2
    stride = max(1, max(map(len, seqs)) // 2)
    hrec, hunits = gpu.motif_batch(*abi.pack_seqs(seqs))                   # the same kernels on the same bytes uploaded from the host
    assert hrec.tobytes() == rec.tobytes() and hunits.shape == (n, min(256, stride)) and np.array_equal(hunits, units[:, :hunits.shape[1]])
    part, punits = gpu.cohort_motifs(2, 3, unit_stride=min(256, stride))
    assert part.tobytes() == rec[2:5].tobytes() and np.array_equal(punits, units[2:5, :punits.shape[1]])
    drec, dunits = gpu.cohort_motifs(1, device_tensor=True)
    assert drec.device == torch.device("cuda", gpu.device) and np.array_equal(drec.cpu().numpy().astype(np.uint32), rec[1:].view(np.uint32).reshape(-1, 6))
    assert np.array_equal(dunits.cpu().numpy(), units[1:])
    assert gpu.cohort_motifs(n, 0)[0].shape == (0,)
    for args, kw in (((n, 1), {}), ((0, n + 1), {}), ((0, n), dict(unit_stride=1)), ((0, n), dict(max_period=0)), ((0, n), dict(slack=1000))):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.cohort_motifs(*args, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), (args, kw)
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
        gpu.cohort_motifs()


# ---------------------------------------------------------------------------------------------- files and the tool
def _vcf_lines(rng):
    rep = lambda u, c, sub=0: Cs.substitute(rng, Cs.rs(rng, u) * c, sub) if sub else Cs.rs(rng, u) * c
    row = lambda i, ref, alt: b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + ref + b"\t" + alt + b"\t.\tPASS\t.\tGT\t0/1"
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
             row(1, rep(3, 20), rep(3, 25, 1) + b"," + rep(3, 17)),
             row(2, rep(5, 30), b"."), row(3, rep(4, 40, 2), b"<DEL>"), row(4, rep(2, 50), b"A,<DEL>"),
             row(5, rep(7, 12), b",".join(rep(7, c, c % 2) for c in (9, 14, 20, 26, 31))),            # six alleles: more than a batch of two
             b"# a comment in the body", row(6, Cs.rs(rng, 300), Cs.rs(rng, 40).lower() + b"," + rep(37, 6)), b"chr1\t700\tfour_columns\t" + rep(6, 9),
             row(8, b"acgtNNacgt" * 6, b"AC"), row(9, rep(300, 3), rep(1, 30))]
    return lines


def _expected_text(lines, max_period=256, slack=50):
    out = []
    for l in lines:
        if not l or l.startswith(b"#"):
            continue
        f = l.split(b"\t")
        alleles = [f[3]]
        if len(f) > 4 and f[4] != b".":
            alleles += [b"N"] if f[4] == b"<DEL>" else f[4].split(b",")
        out += [R.row(f[2], i, a, R.motif_cached(a, max_period, slack)) for i, a in enumerate(alleles)]
    return b"".join(out)


def test_files_and_tool(gpu, tmp_path):
    lines = _vcf_lines(np.random.default_rng(9))
    plain, gz, bed = str(tmp_path / "calls.vcf"), str(tmp_path / "calls.vcf.gz"), str(tmp_path / "regions.bed")
    open(plain, "wb").write(b"\n".join(lines) + b"\n")
    with gzip.GzipFile(gz, "wb", mtime=0) as f:
        f.write(b"\n".join(lines))                                         # the last line has no '\n'
    open(bed, "w").write("chr1\t100\t150\n")
    want = _expected_text(lines)
    assert want.count(b"\n") == 23 and b"chr1:400-450\t2\t5\t0\t.\t" in want and b"\t1\t1\t0\t.\t0.00\t0.0000\n" in want
    text, st = otter_amd.motifs_files(gz, bed)
    assert text == want and st["n_regions"] == 9 and st["n_alleles"] == 23 and st["output_bytes"] == len(want)
    for batch, threads in ((2, 1), (1, 3), (5, 2)):                         # batches smaller than the six-allele record
        assert otter_amd.motifs_files(plain, bed, batch_alleles=batch, threads=threads)[0] == want, (batch, threads)
    assert otter_amd.motifs_files(plain, bed, max_period=4096, slack=0)[0] == _expected_text(lines, 4096, 0) != want
    r = subprocess.run([CLI, "-b", bed, "-t", "2", "--batch", "3", gz], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = subprocess.run([CLI, "-b", bed, "-p", "4096", "--slack=0", plain], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == _expected_text(lines, 4096, 0), r.stderr
    for args in (["-p", "0"], ["-p", "4097"], ["--slack", "1000"]):
        r = subprocess.run([CLI, "-b", bed] + args + [plain], capture_output=True, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and b"[ERROR] invalid" in r.stderr, args

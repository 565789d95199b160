"""GPU: the tract mode of the copy numbers (otg_tract_batch / _motifs / _cohort / otg_tracts_files, tools/otter_tracts).  Records must equal
tests/tract_ref.py (the rule of include/otter_gpu.h restated in plain Python) exactly, on shapes chosen where the kernel can go wrong: every
segment class and its neighbours, tracts that start and end on both sides of a 16-byte load, unequal tasks in one wave, min_score at a
tract's score, other scores, the boundary between the two key widths, the length cap."""
import gzip
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
import cohort_matrix_helpers as M
import motif_cases as Cs
import motif_ref as Mr
import tract_cases as Tc
import tract_ref as R
import unitalign_cases as Uc
import unitalign_ref as U
from test_gpu_unitalign import _stage

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "otter_tracts")
_REF = {}


def ref(s, u, scores=R.DEFAULT, chained=False):
    key = (s, u, scores, chained)
    if key not in _REF:
        _REF[key] = R.tract_np(s, u, *scores, chained=chained)
    return _REF[key]


def _kw(scores):
    return dict(match=scores[0], mismatch=scores[1], indel=scores[2], min_score=scores[3])


def _run(gpu, pairs, scores=R.DEFAULT, **kw):
    seqs, units, ts, tu = Tc.pack(pairs)
    arena, off, ln = abi.pack_seqs(seqs)
    return gpu.tract_batch(arena, off, ln, units, ts, tu, **_kw(scores), **kw)


def _check(gpu, pairs, scores=R.DEFAULT):
    rec = _run(gpu, pairs, scores)
    assert rec.shape == (len(pairs),)
    for t, (s, u) in enumerate(pairs):
        assert tuple(int(x) for x in rec[t]) == ref(s, u, scores), (t, s[:100], u[:100], rec[t], ref(s, u, scores))
    return rec


# ---------------------------------------------------------------------------------------------- 1: the edge set
def test_edge_set(gpu):
    pairs = Tc.edge_set()
    assert {len(u) for _, u in pairs} >= set(Tc.EDGE_P)
    rec = _check(gpu, pairs)
    for t, (s, u, want) in enumerate(Tc.TABLE):                             # the first nine tasks are the prototype's table
        got = tuple(int(x) for x in rec[t])
        assert got[:6] == want and got[7] == 0 if isinstance(want, tuple) else got == (want, 0, 0, 0, 0, 0, 0, abi.TRACT_NONE)
    flags = [int(f) for f in rec["flags"]]
    assert flags.count(0) > 250 and flags.count(abi.TRACT_NONE) >= len(Tc.EDGE_P)
    both, local = gpu.tract_last_ms()
    assert 0 < local < both
    assert _run(gpu, []).shape == (0,)


def test_random_set_and_task_order(gpu):
    pairs = Tc.random_set()
    rec = _check(gpu, pairs)
    perm = np.random.default_rng(3).permutation(len(pairs))
    assert _run(gpu, [pairs[i] for i in perm]).tobytes() == rec[perm].tobytes()


# ---------------------------------------------------------------------------------------------- 2: one wave, unequal neighbours
@pytest.mark.parametrize("p", [3, 7, 13, 29])                              # segments of 4, 8, 16 and 32 lanes
def test_one_wave_of_unequal_neighbours(gpu, p):
    pairs = Tc.one_wave_batch(p)
    lens = sorted(len(s) for s, _ in pairs)
    assert len(pairs) == 16 and lens[:4] == [0, 1, 2, 5] and lens[-1] >= 2700 and all(35 <= x <= 75 for x in lens[4:15])
    rec = _check(gpu, pairs)
    long = max(range(16), key=lambda t: len(pairs[t][0]))
    assert _run(gpu, [pairs[long]]).tobytes() == rec[long:long + 1].tobytes()       # alone in its wave or beside fifteen finished tasks


# ---------------------------------------------------------------------------------------------- 3: the switches
@pytest.mark.parametrize("switch", ["OTG_TRACT_WIDE", "OTG_TRACT_SEG64"])
def test_switch_in_a_fresh_process(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("OTG_TRACT_")}
    env[switch] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tract_switch_child.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- 4: min_score and other scores
def test_min_score_at_a_tracts_score(gpu):
    pairs = [Tc.TABLE[0][:2], Tc.TABLE[7][:2], Tc.TABLE[5][:2], (b"TTT" + Cs.rs(np.random.default_rng(5), 40) * 3 + b"GG", Cs.rs(np.random.default_rng(5), 40))]
    for s, u in pairs:
        score = ref(s, u, (2, 7, 7, 0))[0]
        assert score > 0
        for ms, none in ((score - 1, False), (score, False), (score + 1, True)):
            got = tuple(int(x) for x in _run(gpu, [(s, u)], (2, 7, 7, ms))[0])
            assert got == ref(s, u, (2, 7, 7, ms)) and (got[7] == abi.TRACT_NONE) == none and got[0] == score, (s, u, ms)


@pytest.mark.parametrize("scores", [(1, 1, 1, 5), (16, 64, 64, 100), (3, 2, 5, 0)])
def test_other_scores(gpu, scores):
    _check(gpu, Tc.edge_set()[::3] + Tc.random_set(n=120) + Tc.one_wave_batch(7) + Tc.one_wave_batch(29), scores)
    for bad in (dict(match=0), dict(match=17), dict(mismatch=0), dict(mismatch=65), dict(indel=0), dict(indel=65), dict(min_score=(1 << 24) + 1)):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.tract_batch(*abi.pack_seqs([b"CAG" * 20]), [b"CAG"], [0], [0], **bad)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), bad


# ---------------------------------------------------------------------------------------------- 5: the boundary between the key widths
@pytest.mark.parametrize("p", [37, 256])
def test_tier_boundary(gpu, p):
    N = R.narrow_len(2, 7, p)
    assert 31000 < N < 33000
    rng = np.random.default_rng(53)
    pairs = []
    for k, L in enumerate((N - 1, N, N + 1)):                              # between small neighbours; the score and the begin near their largest
        s, unit = Uc.noisy_repeat(p, L - 2 * k, 100 + k)
        pairs += [(Cs.rs(rng, 20), Cs.rs(rng, 5)), (b"N" * k + s[:L - 2 * k] + b"N" * k, unit), (b"CAG" * 9, b"CAG")]
    pairs[1] = (Uc.repeat_from(pairs[1][1], 3, N - 1), pairs[1][1])          # a pure repeat: the score field at m (N - 1)
    rec = _check(gpu, pairs)
    assert tuple(int(x) for x in rec[1])[:5] == (2 * (N - 1), 0, N - 1, 0, N - 1)
    for t in (4, 7):
        assert len(pairs[t][0]) == N - 1 + t // 3 and int(rec[t]["score"]) > N // 2 and int(rec[t]["end"]) - int(rec[t]["begin"]) > 0.9 * N


# ---------------------------------------------------------------------------------------------- 6: the length cap
def test_length_cap(gpu):
    big = np.tile(np.frombuffer(b"CAG", dtype=np.uint8), abi.TRACT_MAX_LEN // 3 + 2)
    too_long = big[:abi.TRACT_MAX_LEN + 1].tobytes()
    longest = b"TT" + big[1:abi.TRACT_MAX_LEN - 3].tobytes() + b"TT"
    pairs = [Tc.TABLE[0][:2], (too_long, b"CAG"), Tc.TABLE[5][:2], (longest, b"CAG"), Tc.TABLE[1][:2]]
    rec = _run(gpu, pairs)
    assert tuple(int(x) for x in rec[1]) == (0,) * 7 + (abi.TRACT_TOO_LONG,)
    for t in (0, 2, 4):
        assert tuple(int(x) for x in rec[t]) == ref(*pairs[t]), t
    # a perfect repeat that starts on unit position 1 between two flank bases on either side
    n = abi.TRACT_MAX_LEN - 4
    assert len(longest) == abi.TRACT_MAX_LEN and tuple(int(x) for x in rec[3]) == (2 * n, 2, 2 + n, 0, n, (1 + n) % 3, 1, 0)


# ---------------------------------------------------------------------------------------------- 7: the device tensor and the context's other results
def test_device_tensor_and_the_unit_alignment_beside_it(gpu):
    import torch
    pairs = Tc.random_set(n=40) + [(b"", b"CAG"), (b"ACGT", b"")]
    seqs, units, ts, tu = Tc.pack(pairs)
    arena, off, ln = abi.pack_seqs(seqs)
    before = gpu.unitalign_batch(arena, off, ln, units, ts, tu)
    host = gpu.tract_batch(arena, off, ln, units, ts, tu)
    assert tuple(int(x) for x in host[-2]) == (0,) * 7 + (abi.TRACT_NONE,) and tuple(int(x) for x in host[-1]) == (0,) * 7 + (abi.TRACT_NO_UNIT,)
    dev = gpu.tract_batch(arena, off, ln, units, ts, tu, device_tensor=True)
    assert dev.device == torch.device("cuda", gpu.device) and dev.dtype == torch.int32 and dev.shape == (len(pairs), 8)
    assert np.array_equal(dev.cpu().numpy().astype(np.uint32), host.view(np.uint32).reshape(-1, 8))
    # the call counts as a unit alignment on the context: its device results are those of the tracts
    sub = gpu._unitalign_device_results(len(pairs)).cpu().numpy().astype(np.uint32)
    has = host["flags"] == 0
    assert has.sum() > 20 and np.array_equal(sub[has][:, :3], np.stack([host["edits"], host["unit_bases"], host["end_phase"]], axis=1)[has])
    # and either operator still returns what it returned before
    assert gpu.unitalign_batch(arena, off, ln, units, ts, tu).tobytes() == before.tobytes()
    assert gpu.tract_batch(arena, off, ln, units, ts, tu).tobytes() == host.tobytes()
    for t, (s, u) in enumerate(pairs[:40]):
        assert tuple(int(x) for x in before[t]) == U.unitalign_np(s, u) and tuple(int(x) for x in host[t]) == ref(s, u)


# ---------------------------------------------------------------------------------------------- 8: the chains against the host-fed batch
def _chain_expect(gpu, seqs, mrec, munits, scores=R.DEFAULT):
    """tract_batch fed the same alleles and the motif call's units from the host; a period of 0 or over 256 cannot be passed in"""
    pairs, idx = [], []
    for i, s in enumerate(seqs):
        p = int(mrec[i]["period"])
        if 0 < p <= abi.UNITALIGN_MAX_UNIT:
            pairs.append((s, bytes(munits[i][:p]))); idx.append(i)
    want = np.zeros(len(seqs), dtype=abi.tract_dt)
    want[idx] = _run(gpu, pairs, scores)
    for i, s in enumerate(seqs):
        p = int(mrec[i]["period"])
        if p == 0:
            want[i] = (0,) * 7 + (abi.TRACT_NO_UNIT,)
        elif p > abi.UNITALIGN_MAX_UNIT:
            want[i] = (0,) * 7 + (abi.TRACT_UNIT_TOO_LONG,)
    return want


def test_motif_chain_against_the_host_fed_batch(gpu):
    with otter_amd.Context(0) as fresh:
        with pytest.raises(otter_amd.OtterGpuError, match="no motif results") as e:
            fresh.tract_motifs()
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    rng = np.random.default_rng(67)
    seqs = [Cs.rs(rng, int(rng.integers(0, 12))) + s + Cs.rs(rng, int(rng.integers(0, 12))) for s in Cs.random_set(n=50)]
    seqs += [b"", b"AC", b"N" * 30, Cs.rs(rng, 300) * 4, b"GATTACA" + Cs.rs(rng, 19) * 40 + b"TTGACCA", Cs.rs(rng, 700) * 3]
    arena, off, ln = abi.pack_seqs(seqs)
    mrec, munits = gpu.motif_batch(arena, off, ln, max_period=4096)
    rec = gpu.tract_motifs()
    want = _chain_expect(gpu, seqs, mrec, munits)
    assert rec.tobytes() == want.tobytes()
    flags = [int(f) for f in rec["flags"]]
    assert flags.count(abi.TRACT_NO_UNIT) >= 3 and flags.count(abi.TRACT_UNIT_TOO_LONG) == 2 and flags.count(0) > 20
    for i in (50, 51, 52, 53, 54, 55):                                       # and against the reference, unit by unit
        p = int(mrec[i]["period"])
        assert tuple(int(x) for x in rec[i]) == R.tract_np(seqs[i], bytes(munits[i][:p]), chained=True), i
    assert int(mrec[54]["period"]) == 19 and 5 <= int(rec[54]["begin"]) <= 9 and len(seqs[54]) - 9 <= int(rec[54]["end"]) <= len(seqs[54]) - 5      # the flanks are outside
    gpu.motif_batch(arena, off, ln, max_period=4096)
    dev = gpu.tract_motifs(match=3, mismatch=2, indel=5, min_score=0, device_tensor=True)
    assert np.array_equal(dev.cpu().numpy().astype(np.uint32), _chain_expect(gpu, seqs, mrec, munits, (3, 2, 5, 0)).view(np.uint32).reshape(-1, 8))


def test_cohort_rows(gpu):
    other = otter_amd.Context(0)
    try:
        P, refs = _stage(gpu, other)
    finally:
        other.close()
    gpu.cohort_regroup(*abi.pack_seqs(refs))
    with pytest.raises(otter_amd.OtterGpuError, match="has not been clustered"):
        gpu.cohort_tracts(units=[b"CAG"], task_seq=[0], task_unit=[0])
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    rows = gpu.cohort_kmer_rows()
    n = rows["n_rows"]
    seqs = M.row_seqs(rows, got)
    assert n == len(seqs) >= 8
    # the units of the cohort's own motif annotation, in place
    mrec, munits = gpu.cohort_motifs()
    rec = gpu.cohort_tracts()
    assert rec.shape == (n,) and rec.tobytes() == _chain_expect(gpu, seqs, mrec, munits).tobytes()
    with pytest.raises(otter_amd.OtterGpuError, match="was not otg_motif_cohort over rows"):
        gpu.cohort_tracts(1)                                               # the motif call covered other rows
    # a caller's units and task lists: every row against two units, rows counted from row_begin; == tract_batch on the downloaded rows
    k = 1 + int(np.flatnonzero(rec["flags"][1:] == 0)[0])                  # a row with a tract of its own motif unit
    units = [bytes(munits[k][:int(mrec[k]["period"])]), b"AC"]
    ts = np.repeat(np.arange(n - 1, dtype=np.uint32), 2)
    tu = np.tile(np.arange(2, dtype=np.uint32), n - 1)
    crec = gpu.cohort_tracts(1, units=units, task_seq=ts, task_unit=tu, min_score=10)
    arena, off, ln = abi.pack_seqs(seqs[1:])
    assert crec.tobytes() == gpu.tract_batch(arena, off, ln, units, ts, tu, min_score=10).tobytes() and (crec["flags"] == 0).sum() >= 1
    assert int(crec[2 * (k - 1)]["flags"]) == 0 and crec[2 * (k - 1)].tobytes()[4:28] == rec[k].tobytes()[4:28]      # that row again, from the caller's unit
    for t in range(0, len(ts), 3):
        assert tuple(int(x) for x in crec[t]) == ref(seqs[1 + int(ts[t])], units[int(tu[t])], (2, 7, 7, 10)), t
    dev = gpu.cohort_tracts(1, units=units, task_seq=ts, task_unit=tu, min_score=10, device_tensor=True)
    assert np.array_equal(dev.cpu().numpy().astype(np.uint32), crec.view(np.uint32).reshape(-1, 8))
    for args, kw in (((n, 1), dict(units=units, task_seq=[0], task_unit=[0])), ((0, n), dict(units=units, task_seq=[n], task_unit=[0])),
                     ((0, n), dict(units=[b"A" * 257], task_seq=[0], task_unit=[0])), ((0, n), dict(units=units, task_seq=[0], task_unit=[0], indel=0))):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.cohort_tracts(*args, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), (args, kw)
    gpu.cohort_motifs()
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
        gpu.cohort_tracts()
    with pytest.raises(otter_amd.OtterGpuError, match="no longer on the device"):
        gpu.tract_motifs()                                                 # the rows that motif call read went with the batch


# ---------------------------------------------------------------------------------------------- 9: files and the tool
def _vcf_lines(rng):
    noisy = lambda u, c: Cs.rs(rng, int(rng.integers(3, 30))) + Uc.indels(rng, u * c, 0.03, 0.03) + Cs.rs(rng, int(rng.integers(3, 30)))      # flanked
    row = lambda i, ref, alt: b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + ref + b"\t" + alt + b"\t.\tPASS\t.\tGT\t0/1"
    u5, u11 = Cs.rs(rng, 5), Cs.rs(rng, 11)
    return [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
            row(1, Tc.TABLE[3][0], noisy(b"CAG", 25) + b"CCG" * 9 + b"GATTACA," + Tc.TABLE[0][0]),       # a region with two units
            row(2, b"TTGACCA" + u5 * 30 + b"GATTACA", noisy(u5, 22) + b",<DEL>"),                      # a name in column 4: the motif unit
            row(3, u11 * 12, b",".join(noisy(u11, c) for c in (9, 14, 20, 26, 31))),                     # absent from the BED; six alleles
            row(4, Cs.rs(rng, 60), b"AC"),                                                              # units; alleles without a tract
            row(5, b"AC", b"."),                                                                        # no BED record, no period
            row(1, b"GATTACA" * 9, b".")]                                                               # the region of the first line again


CATALOGUE = "chr1\t100\t150\tID=x;MOTIFS=CAG,CCG\nchr1\t200\t250\tlocus_two\nchr1\t400\t450\tacg\nchr1\t100\t150\tTTT\n"
BED_UNITS = {b"chr1:100-150": [b"CAG", b"CCG"], b"chr1:400-450": [b"acg"]}


def _expected_text(lines, scores=R.DEFAULT, max_period=256, slack=50):
    """by construction the edits, unit bases and copies of a row are those of the global unit alignment (otter_copies) of s[begin, end)"""
    out = []
    for l in lines:
        if not l or l.startswith(b"#"):
            continue
        f = l.split(b"\t")
        alleles = [f[3]]
        if len(f) > 4 and f[4] != b".":
            alleles += [b"N"] if f[4] == b"<DEL>" else f[4].split(b",")      # (a <DEL> beside other alleles is read as its five bytes)
        for i, a in enumerate(alleles):
            if f[2] in BED_UNITS:
                todo = [(b"bed", u) for u in BED_UNITS[f[2]]]
            else:
                m = Mr.motif_cached(a, max_period, slack)
                todo = [(b"motif", m["unit"] if m["period"] else b"")]
            for source, u in todo:
                rec = ref(a, u, scores, True)
                if rec[7] == 0:
                    assert rec[3:6] == U.unitalign_np(a[rec[1]:rec[2]], u)[:3]
                out.append(R.row(f[2], i, len(a), source, u, rec))
    return b"".join(out)


def test_files_and_tool(gpu, tmp_path):
    lines = _vcf_lines(np.random.default_rng(71))
    plain, gz, bed = str(tmp_path / "calls.vcf"), str(tmp_path / "calls.vcf.gz"), str(tmp_path / "catalogue.bed")
    open(plain, "wb").write(b"\n".join(lines) + b"\n")
    with gzip.GzipFile(gz, "wb", mtime=0) as f:
        f.write(b"\n".join(lines))                                         # the last line has no '\n'
    open(bed, "w").write(CATALOGUE)
    want = _expected_text(lines)
    assert want.count(b"\n") == 3 * 2 + 3 + 6 + 2 + 1 + 2
    assert b"chr1:100-150\t0\t120\tbed\tCAG\t0\t61\t122\t0\t61\t20.33\t1.0000\n" in want and b"chr1:100-150\t0\t120\tbed\tCCG\t59\t120\t122\t0\t61\t20.33\t1.0000\n" in want
    assert b"chr1:100-150\t2\t74\tbed\tCAG\t7\t67\t120\t0\t60\t20.00\t1.0000\n" in want and b"chr1:500-550\t0\t2\tmotif\t.\t0\t0\t0\t0\t0\t0.00\t0.0000\n" in want
    assert b"\tbed\tTTT\t" not in want and want.count(b"\tmotif\t") == 10
    text, st = otter_amd.tracts_files(gz, bed)
    assert text == want and st["n_regions"] == 6 and st["n_alleles"] == 16 and st["output_bytes"] == len(want)
    for batch, threads in ((2, 1), (5, 2)):                                 # batches smaller than the six-allele record
        assert otter_amd.tracts_files(plain, bed, batch_alleles=batch, threads=threads)[0] == want, (batch, threads)
    other = (3, 2, 5, 40)
    assert otter_amd.tracts_files(plain, bed, **_kw(other))[0] == _expected_text(lines, other) != want
    r = subprocess.run([CLI, "-b", bed, "-t", "2", "--batch", "3", gz], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = subprocess.run([CLI, "-b", bed, "--scores", "3,2,5", "--min-score=40", "--batch", "7", plain], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == _expected_text(lines, other), r.stderr

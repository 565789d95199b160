"""GPU: alleles aligned to a cyclic repeat unit (otg_unitalign_batch / _motifs / _cohort / otg_copies_files, tools/otter_copies).  Records
must equal tests/unitalign_ref.py (the rule of include/otter_gpu.h restated in plain Python) exactly, on shapes chosen where the kernel can
go wrong: every segment class and its neighbours, unequal tasks in one wave, the boundary between the two key widths, the length cap."""
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
import motif_ref as Mr
import unitalign_cases as Uc
import unitalign_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "otter_copies")
_REF = {}


def ref(s, u, chained=False):
    key = (s, u, chained)
    if key not in _REF:
        _REF[key] = R.unitalign_np(s, u, chained)
    return _REF[key]


def _run(gpu, pairs, **kw):
    seqs, units, ts, tu = Uc.pack(pairs)
    arena, off, ln = abi.pack_seqs(seqs)
    return gpu.unitalign_batch(arena, off, ln, units, ts, tu, **kw)


def _check(gpu, pairs):
    rec = _run(gpu, pairs)
    assert rec.shape == (len(pairs),)
    for t, (s, u) in enumerate(pairs):
        assert tuple(int(x) for x in rec[t]) == ref(s, u), (t, s[:100], u[:100], rec[t], ref(s, u))
    return rec


# ---------------------------------------------------------------------------------------------- 1: the edge set
def test_edge_set(gpu):
    pairs = Uc.edge_set()
    assert {len(u) for _, u in pairs} >= set(Uc.EDGE_P)
    rec = _check(gpu, pairs)
    for t, (s, u, want) in enumerate(Uc.TABLE):                             # the first eleven tasks are the prototype's table
        assert tuple(int(x) for x in rec[t])[:3] == want
    assert gpu.unitalign_last_ms() > 0
    assert _run(gpu, []).shape == (0,)


def test_random_set_and_task_order(gpu):
    pairs = Uc.random_set()
    rec = _check(gpu, pairs)
    perm = np.random.default_rng(3).permutation(len(pairs))
    assert _run(gpu, [pairs[i] for i in perm]).tobytes() == rec[perm].tobytes()


# ---------------------------------------------------------------------------------------------- 2: one wave, unequal neighbours
@pytest.mark.parametrize("p", [3, 7, 13, 29])                              # segments of 4, 8, 16 and 32 lanes
def test_one_wave_of_unequal_neighbours(gpu, p):
    pairs = Uc.one_wave_batch(p)
    lens = sorted(len(s) for s, _ in pairs)
    assert len(pairs) == 16 and lens[:4] == [0, 1, 2, 5] and lens[-1] >= 2700 and all(45 <= x <= 75 for x in lens[4:15])
    rec = _check(gpu, pairs)
    long = max(range(16), key=lambda t: len(pairs[t][0]))
    assert _run(gpu, [pairs[long]]).tobytes() == rec[long:long + 1].tobytes()       # alone in its wave or beside fifteen finished tasks


# ---------------------------------------------------------------------------------------------- 3: the switches
@pytest.mark.parametrize("switch", ["OTG_UNITALIGN_WIDE", "OTG_UNITALIGN_SEG64"])
def test_switch_in_a_fresh_process(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("OTG_UNITALIGN_")}
    env[switch] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unitalign_switch_child.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- 4: the boundary between the key widths
@pytest.mark.parametrize("p", [37, 256])
def test_tier_boundary(gpu, p):
    N = abi.UNITALIGN_NARROW_LEN
    rng = np.random.default_rng(53)
    pairs = []
    for k, L in enumerate((N - 1, N, N + 1)):
        pairs += [(Cs.rs(rng, 20), Cs.rs(rng, 5)), Uc.noisy_repeat(p, L, 100 + k), (b"CAG" * 9, b"CAG")]      # between small neighbours
    rec = _check(gpu, pairs)
    for t in (1, 4, 7):
        e, ub = int(rec[t]["edits"]), int(rec[t]["unit_bases"])
        assert len(pairs[t][0]) == N - 1 + t // 3 and 0.03 * N < e < 0.2 * N and abs(ub - N) < 0.1 * N


# ---------------------------------------------------------------------------------------------- 5: the length cap
def test_length_cap(gpu):
    big = np.tile(np.frombuffer(b"CAG", dtype=np.uint8), abi.UNITALIGN_MAX_LEN // 3 + 2)
    too_long, longest = big[:abi.UNITALIGN_MAX_LEN + 1].tobytes(), big[1:abi.UNITALIGN_MAX_LEN + 1].tobytes()
    pairs = [(b"CAG" * 20, b"CAG"), (too_long, b"CAG"), (b"GATTACA" * 9, b"TTACAGA"), (longest, b"CAG"), (b"CAG" * 10 + b"T" + b"CAG" * 10, b"AGC")]
    rec = _run(gpu, pairs)
    assert tuple(int(x) for x in rec[1]) == (0, 0, 0, abi.UNITALIGN_TOO_LONG)
    for t in (0, 2, 4):
        assert tuple(int(x) for x in rec[t]) == ref(*pairs[t]), t
    # a perfect repeat that starts on unit position 1: no edit, every base a unit base, and the phase behind the last one
    assert tuple(int(x) for x in rec[3]) == (0, abi.UNITALIGN_MAX_LEN, (1 + abi.UNITALIGN_MAX_LEN) % 3, 0)


# ---------------------------------------------------------------------------------------------- 6: the limit this removes
def test_copies_of_a_noisy_repeat_through_the_motif_chain(gpu):
    """The 37-base unit at 10 % indel error that the shifted self-comparison recovers about every second time: the chain counts its 30
    copies.  (CAG)10T(CAG)10 gives (1, 60) against the catalogue unit CAG.  Through the chain the reference gives it (21, 59): the motif
    rule builds its unit by a majority per phase, and the inserted T puts the second half out of phase, so that unit is not a rotation of
    CAG.  Both values are the reference's."""
    rng = np.random.default_rng(61)
    unit = Cs.rs(rng, 37)
    noisy = Uc.indels(rng, unit * 30, 0.05, 0.05)
    seqs = [noisy, b"CAG" * 10 + b"T" + b"CAG" * 10]
    want = []
    for s in seqs:                                                         # the reference chain: the motif rule's unit, then the alignment rule
        m = Mr.motif(s)
        want.append(R.unitalign_np(s, m["unit"] if m["period"] else b"", chained=True))
    assert Mr.motif(noisy)["period"] == 37 and abs(want[0][1] / 37 - 30) <= 1 and want[0][0] > 40
    assert want[1][:2] == (21, 59) and R.unitalign(seqs[1], b"CAG")[:2] == (1, 60)
    arena, off, ln = abi.pack_seqs(seqs)
    mrec, munits = gpu.motif_batch(arena, off, ln)
    rec = gpu.unitalign_motifs()
    assert [int(p) for p in mrec["period"]] == [37, 3]
    assert [tuple(int(x) for x in r) for r in rec] == want
    assert abs(int(rec[0]["unit_bases"]) / 37 - 30) <= 1
    assert tuple(int(x) for x in _run(gpu, [(seqs[1], b"CAG")])[0])[:2] == (1, 60)


# ---------------------------------------------------------------------------------------------- 7: the chains against the host-fed batch
def _chain_expect(gpu, seqs, mrec, munits):
    """unitalign_batch fed the same alleles and the motif call's units from the host; a period of 0 or over 256 cannot be passed in"""
    pairs, idx = [], []
    for i, s in enumerate(seqs):
        p = int(mrec[i]["period"])
        if 0 < p <= abi.UNITALIGN_MAX_UNIT:
            pairs.append((s, bytes(munits[i][:p]))); idx.append(i)
    want = np.zeros(len(seqs), dtype=abi.unitalign_dt)
    want[idx] = _run(gpu, pairs)
    for i, s in enumerate(seqs):
        p = int(mrec[i]["period"])
        if p == 0:
            want[i] = (0, 0, 0, abi.UNITALIGN_NO_UNIT)
        elif p > abi.UNITALIGN_MAX_UNIT:
            want[i] = (0, 0, 0, abi.UNITALIGN_UNIT_TOO_LONG)
    return want


def test_motif_chain_against_the_host_fed_batch(gpu):
    import torch
    with otter_amd.Context(0) as fresh:
        with pytest.raises(otter_amd.OtterGpuError, match="no motif results") as e:
            fresh.unitalign_motifs()
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    rng = np.random.default_rng(67)
    seqs = Cs.random_set(n=60) + [b"", b"AC", b"N" * 30, Cs.rs(rng, 300) * 4, Uc.indels(rng, Cs.rs(rng, 19) * 40, 0.04, 0.04), Cs.rs(rng, 700) * 3]
    arena, off, ln = abi.pack_seqs(seqs)
    mrec, munits = gpu.motif_batch(arena, off, ln, max_period=4096)
    rec = gpu.unitalign_motifs()
    want = _chain_expect(gpu, seqs, mrec, munits)
    assert rec.tobytes() == want.tobytes()
    flags = [int(f) for f in rec["flags"]]
    assert flags.count(abi.UNITALIGN_NO_UNIT) >= 3 and flags.count(abi.UNITALIGN_UNIT_TOO_LONG) == 2 and flags.count(0) > 50
    for i in (60, 61, 62, 63, 64):                                           # and against the reference, unit by unit
        p = int(mrec[i]["period"])
        assert tuple(int(x) for x in rec[i]) == R.unitalign_np(seqs[i], bytes(munits[i][:p]), chained=True), i
    gpu.motif_batch(arena, off, ln, max_period=4096)
    dev = gpu.unitalign_motifs(device_tensor=True)
    assert dev.device == torch.device("cuda", gpu.device) and dev.dtype == torch.int32 and dev.shape == (len(seqs), 4)
    assert np.array_equal(dev.cpu().numpy().astype(np.uint32), want.view(np.uint32).reshape(-1, 4))
    drec = _run(gpu, [(seqs[1], b"ACG"), (seqs[3], b"T")], device_tensor=True)
    assert np.array_equal(drec.cpu().numpy().astype(np.uint32), _run(gpu, [(seqs[1], b"ACG"), (seqs[3], b"T")]).view(np.uint32).reshape(-1, 4))


def test_refusals_on_the_device(gpu):
    arena, off, ln = abi.pack_seqs([b"CAG" * 20, b"ACGT" * 50])
    ok = gpu.unitalign_batch(arena, off, ln, [b"CAG", b"A" * 256], [0, 1], [0, 1])
    assert tuple(int(x) for x in ok[0]) == (0, 60, 0, 0)
    for units, ts, tu in (([b"CAG"], [2], [0]), ([b"CAG"], [0], [1]), ([b"A" * 257], [0], [0]), ([], [0], [0])):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.unitalign_batch(arena, off, ln, units, ts, tu)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), (units, ts, tu)
    with pytest.raises(otter_amd.OtterGpuError) as e:
        gpu.unitalign_batch(arena, np.array([arena.size, 0], dtype=np.uint64), ln, [b"CAG"], [0], [0])
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    none = gpu.unitalign_batch(arena, off, ln, [b"", b"CAG"], [0, 1], [0, 1])                       # an empty unit is a flag, not a refusal
    assert tuple(int(x) for x in none[0]) == (0, 0, 0, abi.UNITALIGN_NO_UNIT) and tuple(int(x) for x in none[1]) == ref(b"ACGT" * 50, b"CAG")


def _stage(gpu, other):
    """3 samples over 4 regions, staged for a regroup (as tests/test_gpu_motif.py stages them) -> (parameters, reference alleles)"""
    B, S = 4, 3
    P = abi.default_params(max_alleles=4)
    gpu.cohort_begin(B, S)
    for k in range(S):
        b = synth.make_batch(B, len_range=(150, 400), reads_range=(8, 14), err="hifi", seed=911 + k, frac_partial=0.1, frac_het=0.8)
        ctx = other if (k % 2) else gpu
        ctx.assemble_submit(P, b)
        ctx.assemble_run()
        ctx.assemble_collect()
        gpu.cohort_stage(k, src=ctx)
    rng = np.random.default_rng(4)
    return P, [Cs.substitute(rng, Cs.rs(rng, int(rng.integers(2, 7))) * int(rng.integers(30, 60)), 2) for _ in range(B)]


def test_cohort_rows(gpu):
    other = otter_amd.Context(0)
    try:
        P, refs = _stage(gpu, other)
    finally:
        other.close()
    gpu.cohort_regroup(*abi.pack_seqs(refs))
    with pytest.raises(otter_amd.OtterGpuError, match="has not been clustered"):
        gpu.cohort_unitalign(units=[b"CAG"], task_seq=[0], task_unit=[0])
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    rows = gpu.cohort_kmer_rows()
    n = rows["n_rows"]
    seqs = M.row_seqs(rows, got)
    assert n == len(seqs) >= 8
    # the units of the cohort's own motif annotation, in place
    mrec, munits = gpu.cohort_motifs()
    rec = gpu.cohort_unitalign()
    assert rec.shape == (n,) and rec.tobytes() == _chain_expect(gpu, seqs, mrec, munits).tobytes() and (rec["flags"] == 0).sum() >= n - 2
    for i in range(0, n, 3):
        p = int(mrec[i]["period"])
        assert tuple(int(x) for x in rec[i]) == R.unitalign_np(seqs[i], bytes(munits[i][:p]), chained=True), i
    with pytest.raises(otter_amd.OtterGpuError, match="was not otg_motif_cohort over rows"):
        gpu.cohort_unitalign(1)                                            # the motif call covered other rows
    gpu.cohort_motifs(2, 3)
    assert gpu.cohort_unitalign(2, 3).tobytes() == rec[2:5].tobytes()
    # a caller's units and task lists: every row against two units, rows counted from row_begin
    units = [refs[0][:4], b"AC"]
    ts = np.repeat(np.arange(n - 1, dtype=np.uint32), 2)
    tu = np.tile(np.arange(2, dtype=np.uint32), n - 1)
    crec = gpu.cohort_unitalign(1, units=units, task_seq=ts, task_unit=tu)
    for t in range(len(ts)):
        assert tuple(int(x) for x in crec[t]) == ref(seqs[1 + int(ts[t])], units[int(tu[t])]), t
    dev = gpu.cohort_unitalign(1, units=units, task_seq=ts, task_unit=tu, device_tensor=True)
    assert np.array_equal(dev.cpu().numpy().astype(np.uint32), crec.view(np.uint32).reshape(-1, 4))
    for args, kw in (((n, 1), dict(units=units, task_seq=[0], task_unit=[0])), ((0, n), dict(units=units, task_seq=[n], task_unit=[0])),
                     ((0, n), dict(units=units, task_seq=[0], task_unit=[2])), ((0, n), dict(units=[b"A" * 257], task_seq=[0], task_unit=[0]))):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.cohort_unitalign(*args, **kw)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value), (args, kw)
    gpu.cohort_motifs()
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
        gpu.cohort_unitalign()
    with pytest.raises(otter_amd.OtterGpuError, match="no longer on the device"):
        gpu.unitalign_motifs()                                             # the rows that motif call read went with the batch


# ---------------------------------------------------------------------------------------------- 8: files and the tool
def _vcf_lines(rng):
    noisy = lambda u, c: Uc.indels(rng, u * c, 0.04, 0.04)
    row = lambda i, ref, alt: b"chr1\t%d\tchr1:%d-%d\t" % (100 * i, 100 * i, 100 * i + 50) + ref + b"\t" + alt + b"\t.\tPASS\t.\tGT\t0/1"
    u5, u11 = Cs.rs(rng, 5), Cs.rs(rng, 11)
    return [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
            row(1, b"CAG" * 20 + b"CCG" * 10, noisy(b"CAG", 25) + b"CCG" * 9 + b"," + b"CAG" * 17),      # a region with units
            row(2, u5 * 30, noisy(u5, 22) + b",<DEL>"),                                                 # a name in column 4
            row(3, u11 * 12, b",".join(noisy(u11, c) for c in (9, 14, 20, 26, 31))),                     # absent from the BED; six alleles
            row(4, Cs.rs(rng, 60), b"AC"),                                                              # units; an allele without a repeat
            row(5, b"AC", b"."),                                                                        # no BED record, no period
            row(1, b"GATTACA" * 9, b".")]                                                               # the region of the first line again


CATALOGUE = "chr1\t100\t150\tID=x;MOTIFS=CAG,CCG\nchr1\t200\t250\tlocus_two\nchr1\t400\t450\tacg\nchr1\t100\t150\tTTT\n"
BED_UNITS = {b"chr1:100-150": [b"CAG", b"CCG"], b"chr1:400-450": [b"acg"]}


def _expected_text(lines, max_period=256, slack=50):
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
                out += [R.row(f[2], i, len(a), b"bed", u, ref(a, u)) for u in BED_UNITS[f[2]]]
            else:
                m = Mr.motif_cached(a, max_period, slack)
                u = m["unit"] if m["period"] else b""
                out.append(R.row(f[2], i, len(a), b"motif", u, ref(a, u, True)))
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
    assert b"chr1:100-150\t0\t90\tbed\tCAG\t10\t90\t30.00\t0.8889\n" in want and b"chr1:500-550\t0\t2\tmotif\t.\t0\t0\t0.00\t0.0000\n" in want
    assert b"\tbed\tTTT\t" not in want and want.count(b"\tmotif\t") == 10
    text, st = otter_amd.copies_files(gz, bed)
    assert text == want and st["n_regions"] == 6 and st["n_alleles"] == 16 and st["output_bytes"] == len(want)
    for batch, threads in ((2, 1), (1, 3), (5, 2)):                         # batches smaller than the six-allele record
        assert otter_amd.copies_files(plain, bed, batch_alleles=batch, threads=threads)[0] == want, (batch, threads)
    assert otter_amd.copies_files(plain, bed, max_period=4, slack=0)[0] == _expected_text(lines, 4, 0) != want
    r = subprocess.run([CLI, "-b", bed, "-t", "2", "--batch", "3", gz], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = subprocess.run([CLI, "-b", bed, "-p", "4", "--slack=0", plain], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == _expected_text(lines, 4, 0), r.stderr

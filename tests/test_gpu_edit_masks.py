"""GPU parity of the match masks of the bit-parallel edit tiers (otter_amd/csrc/myers_masks.hpp): the per-read plane table the pipeline
builds once per run, and the wave-parallel builder every other pair falls back to.

Pipeline against the oracle on a dozen small regions whose read lengths sit on the 64-row block edges (1, 63, 64, 65, 127, 128, 129,
191, 192, 193) plus two regions near 1 000: identical reads, partial reads with only spanning_l or only spanning_r (the second kind are
the mirrored tasks, whose reversed copies have no table blocks), a read with an N as the longer and one as the shorter read of its pairs,
a read with two further byte values; and a `-r` batch in which realignment trims reads' starts, so that a read's blocks no longer begin
where the submitted ones did.  Labels, distance matrices and allele records must equal the oracle's.  The first case runs again with
OTG_EDIT_MASKS=0 (no table: every pair builds its own masks) in a fresh child process, and the two outputs must be equal.

otg_edit_distance_batch (no table, the builder alone) against the oracle's edit distance: eight pairs per wave with eight different
pattern lengths, tasks with m < n, one and two further byte values in the pattern."""
import os
import subprocess
import sys
import numpy as np
import pytest
from otter_amd import abi, synth
from helpers import rand_seq, mutate, tr_seq, pair_tasks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_ENV = "OTG_TEST_EDIT_MASKS_DUMP"       # set for the child: where it writes what the pipeline returned

EDGE_LENS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193)


def _put(s, i, ch):
    b = bytearray(s); b[i] = ord(ch); return bytes(b)


def _far_pair(rng, m):
    """Two sequences of m and about m bytes that the wavefront pass cannot finish (its score cap is 48 for short pairs), so that the pair
    reaches the bit-parallel tiers: unrelated ones from 127 bytes on; below that 49 columns that cannot match (A / C against G / T) between
    a shared head and tail, whose rows still have to match."""
    if m >= 127:
        return tr_seq(rng, m), rand_seq(rng, m - 5)
    if m < 56:
        s = rand_seq(rng, m)
        return s, s
    ac, gt = np.frombuffer(b"AC", np.uint8), np.frombuffer(b"GT", np.uint8)
    head, tail = rand_seq(rng, 7), rand_seq(rng, m - 56)
    return head + ac[rng.integers(0, 2, 49)].tobytes() + tail, head + gt[rng.integers(0, 2, 49)].tobytes() + tail


def _edge_batch():
    """regions of 6-10 reads; a read = (bytes, spanning_l, spanning_r)"""
    rng = np.random.default_rng(6464)
    regions = []
    for L in EDGE_LENS:
        a, b = _far_pair(rng, L)                                                                  # two alleles more than 48 edits apart
        reads = [(a, 1, 1), (a, 1, 1), (b, 1, 1), (b, 1, 1)]                                       # identical reads
        reads += [(mutate(rng, a, 0.02) or b"A", 1, 1), (mutate(rng, b, 0.02) or b"C", 1, 1)]
        if L > 1:
            reads += [(mutate(rng, a, 0.05) or b"G", 1, 1)]
            cut = max(1, (2 * L) // 3)
            reads += [(a[:cut], 1, 0), (b[len(b) - min(cut, len(b)):], 0, 1)]                      # only spanning_l; only spanning_r (mirrored)
            if L % 2:
                reads += [(a[len(a) - cut:], 0, 1)]
        regions.append(reads)
    for L in (1000, 960):
        a = tr_seq(rng, L)
        b = a[:300] + a[300 + 90:]
        longest = _put(mutate(rng, a, 0.03) + rand_seq(rng, 40), 517, "N")                        # N in the longer read of every pair it is in
        shortest = _put(mutate(rng, b, 0.03)[:820], 64, "N")                                      # N in the shorter read of every pair it is in
        two = _put(_put(mutate(rng, a, 0.03), 63, "N"), 700, "R")                                 # two further byte values: the wavefront kernel's
        reads = [(a, 1, 1), (a, 1, 1), (mutate(rng, a, 0.07), 1, 1), (mutate(rng, b, 0.07), 1, 1), (mutate(rng, b, 0.07), 1, 1),
                 (longest, 1, 1), (shortest, 1, 1), (two, 1, 1), (mutate(rng, a, 0.05)[:640], 1, 0), (mutate(rng, b, 0.05)[-513:], 0, 1)]
        regions.append(reads)
    seqs = [s for reads in regions for s, _, _ in reads]
    arena, offs, lens = abi.pack_seqs(seqs)
    rd = np.zeros(len(seqs), dtype=abi.read_dt)
    rg = np.zeros(len(regions), dtype=abi.region_dt)
    k = 0
    for r, reads in enumerate(regions):
        assert 6 <= len(reads) <= 10
        rg[r]["first_read"], rg[r]["n_reads"] = k, len(reads)
        for s, spl, spr in reads:
            rd[k] = (int(offs[k]), int(lens[k]), spl, spr, 0, -1, -1, 0, int(lens[k]))
            k += 1
    return {"arena": arena, "reads": rd, "regions": rg}


def _dist_slices(batch, res, max_cov=200):
    """(start, count) of every region's condensed matrix in otg_assemble_collect_dist's layout, and the number of slots"""
    n = batch["regions"]["n_reads"].astype(np.int64)
    slots = np.where(n > max_cov, 0, n * (n - 1) // 2)
    start = np.concatenate([[0], np.cumsum(slots)])
    v = res["regions"]["n_valid"].astype(np.int64)
    return [(int(start[r]), int(v[r] * (v[r] - 1) // 2)) for r in range(len(n))], int(start[-1])


def _run(gpu, batch, **kw):
    P = abi.default_params(**kw)
    res = gpu.assemble(P, batch)
    st = gpu.assemble_stats()
    sl, n_slots = _dist_slices(batch, res)
    d = gpu.assemble_collect_dist(n_slots)
    res["dist"] = [d[a:a + c].copy() for a, c in sl]
    return res, st


def _check_against_oracle(res, st, ora):
    for f in ("status", "ic", "fc", "n_valid", "n_alleles", "first_allele"):
        assert np.array_equal(res["regions"][f], ora["regions"][f]), f
    assert np.array_equal(res["labels"], ora["labels"])
    for r, d in enumerate(res["dist"]):
        if res["regions"]["status"][r] != 0 or len(d) == 0:
            continue
        o = ora["dist"][int(ora["dist_off"][r]):int(ora["dist_off"][r]) + len(d)]
        assert np.array_equal(d, o), ("distance matrix of region", r, d, o)
    ga, oa = res["alleles"], ora["alleles"]
    assert len(ga) == len(oa)
    for f in ("seq_len", "scov", "acov", "tcov", "ic", "ps", "hp", "region", "label"):
        assert np.array_equal(ga[f], oa[f]), f
    assert np.allclose(ga["se"], oa["se"], rtol=0, atol=1e-6)
    for i in range(len(ga)):
        assert res["seqs"][int(ga[i]["seq_off"]):int(ga[i]["seq_off"]) + int(ga[i]["seq_len"])].tobytes() == \
            ora["seqs"][int(oa[i]["seq_off"]):int(oa[i]["seq_off"]) + int(oa[i]["seq_len"])].tobytes(), "allele %d sequence differs" % i
    os_ = ora["stats"][0]
    for f in ("edit_tasks", "edit_cells", "edit_seq_bytes"):
        assert int(st[f]) == int(os_[f]), f


def _flat(res):
    out = {"labels": res["labels"], "seqs": res["seqs"], "dist": np.concatenate(res["dist"]) if res["dist"] else np.zeros(0)}
    for f in res["regions"].dtype.names:
        out["regions_" + f] = res["regions"][f]
    for f in res["alleles"].dtype.names:
        out["alleles_" + f] = res["alleles"][f]
    return out


@pytest.fixture(scope="module")
def edge_batch():
    return _edge_batch()


def test_pipeline_edges_against_oracle(gpu, oracle, edge_batch):
    res, st = _run(gpu, edge_batch)
    ora = oracle.assemble_batch(abi.default_params(), edge_batch)
    assert int(st["edit_tasks"]) > 200 and int((res["regions"]["status"] == 0).sum()) == len(edge_batch["regions"])
    _check_against_oracle(res, st, ora)
    if os.environ.get(DUMP_ENV):
        np.savez(os.environ[DUMP_ENV], **_flat(res))


def test_pipeline_realigned_reads_against_oracle(gpu, oracle):
    """-r: realignment moves seq_off and shortens reads after the table's blocks were laid out from the submitted lengths"""
    b = synth.make_batch(3, len_range=(500, 800), n_reads=8, err="ont", realign=True, frac_clipped=0.5, frac_partial=0.15, seed=65)
    trimmed = gpu.realign_reads(abi.default_params(realign=1), b)
    moved = trimmed["seq_off"] > b["reads"]["seq_off"]
    assert moved.any() and (trimmed["seq_len"][moved] < b["reads"]["seq_len"][moved]).all()        # a read's start was trimmed
    res, st = _run(gpu, b, realign=1)
    ora = oracle.assemble_batch(abi.default_params(realign=1), b)
    _check_against_oracle(res, st, ora)


def test_force_switch_child(gpu, edge_batch, tmp_path):
    """OTG_EDIT_MASKS=0 in a fresh process: no table, the in-kernel builder everywhere; the same outputs"""
    res, _ = _run(gpu, edge_batch)
    gpu.trim()
    path = str(tmp_path / "no_table.npz")
    env = dict(os.environ, OTG_EDIT_MASKS="0")
    env[DUMP_ENV] = path
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_edit_masks.py::test_pipeline_edges_against_oracle"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    mine = _flat(res)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(mine)
        for k in z.files:
            assert np.array_equal(z[k], mine[k]), k


# ---------------------------------------------------------------------------------------------- the builder alone
WAVE_LENS = (1, 63, 64, 65, 640, 1000, 4097, 16384)      # eight pairs of one <1,8> wave, eight pattern lengths


def _builder_batch():
    rng = np.random.default_rng(1664)
    pairs = []
    for rep in range(2):                                  # the same eight lengths in two orders: the sort keeps like with like, the first pass does not
        for m in (WAVE_LENS if rep == 0 else WAVE_LENS[::-1]):
            if m > 65:                                    # close enough for the narrowest tier, too far for the wavefront pass
                p = rand_seq(rng, m)
                t = mutate(rng, p, 0.1 if m < 2000 else 0.04)[:m]
            else:
                p, t = _far_pair(rng, m)
            pairs.append((p, t))
    n_wave = len(pairs)
    for m in (65, 129, 1000):                             # m < n: the kernel swaps the two
        p = rand_seq(rng, m)
        pairs.append((mutate(rng, p, 0.1)[:m - 7], p))
    n_swapped = len(pairs)
    for m in (64, 65, 700, 4097):                         # one further byte value: in the first block, on a block edge, past it
        p = rand_seq(rng, m)
        x = _put(_put(p, 0, "N"), m - 1, "N") if m > 64 else _put(p, 63, "N")
        pairs.append((_put(x, m // 2, "N"), mutate(rng, p, 0.1)[:m]))
        pairs.append((x, _put(mutate(rng, p, 0.1)[:m - 1], 5, "N")))          # ... and in the text as well
    n_one = len(pairs)
    for m in (130, 900):                                  # two further byte values: goes on to the wavefront kernel
        p = rand_seq(rng, m)
        pairs.append((_put(_put(p, 64, "N"), 65, "R"), mutate(rng, p, 0.15)[:m]))
    return pair_tasks(pairs), (n_wave, n_swapped, n_one)


def test_builder_against_oracle(gpu, oracle):
    (arena, tasks), (n_wave, n_swapped, n_one) = _builder_batch()
    assert all(int(t["pattern_len"]) < int(t["text_len"]) for t in tasks[n_wave:n_swapped])
    exp = oracle.edit_distance_batch(arena, tasks)
    got = gpu.edit_distance_batch(arena, tasks)
    reach = [int(e) for t, e in zip(tasks[:n_wave], exp[:n_wave]) if int(t["pattern_len"]) > 1]
    assert min(reach) > 48, reach                      # beyond the wavefront pass's score cap: the bit-parallel tiers finish them
    bad = [(int(i), int(tasks[i]["pattern_len"]), int(tasks[i]["text_len"]), int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]
    print("builder: %d pairs, %d differ; distances %s" % (len(got), len(bad), exp.tolist()))
    assert not bad, bad


@pytest.mark.parametrize("switch", ["OTG_EDIT_TIERS=255 OTG_NO_EDIT_ROUTE=1 OTG_NO_EDIT_SORT=1"], ids=["all_tiers_unrouted"])
def test_builder_child(gpu, switch):
    """every pair enters at tier 0, unsorted — the eight lengths share one wave — and climbs: every tier's builder runs"""
    gpu.trim()
    env = dict(os.environ)
    for kv in switch.split():
        k, _, v = kv.partition("=")
        env[k] = v
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_edit_masks.py::test_builder_against_oracle"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (switch, r.stdout[-3000:], r.stderr[-1000:])

"""The small kernels between the aligner passes of the pipeline (pipeline.hip): the pair-task and reassignment-task generators, which take one
lane per pair and append to the todo list with one atomic per wave, and the two compaction scans, which are one launch.  Checked through the
pipeline against the CPU oracle: distance matrices (otg_assemble_collect_dist), the number of edit alignments, labels after reassignment,
allele offsets and totals."""
import numpy as np
import pytest
from otter_amd import abi, synth
from test_gpu_edit_masks import _run, _check_against_oracle

pytestmark = pytest.mark.gpu


def _check(gpu, oracle, batch, **kw):
    res, st = _run(gpu, batch, **kw)
    ora = oracle.assemble_batch(abi.default_params(**kw), batch)
    _check_against_oracle(res, st, ora)          # matrices slot by slot, labels, records, edit_tasks = the oracle's pair count
    return res, st, ora


@pytest.mark.parametrize("n_reads", [2, 3, 65, 130])
def test_pair_tasks_rows(gpu, oracle, n_reads):
    """2 and 3 valid reads (one pair, one full row); 65 and 130: 2 080 and 8 385 pairs, rows longer than a wave, a last trip that is partly
    filled, row starts at every lane position.  100-base reads keep the alignments short."""
    b = synth.make_batch(3, len_range=(100, 100), n_reads=n_reads, err="ont", seed=300 + n_reads, frac_partial=0.0)
    res, st, ora = _check(gpu, oracle, b)
    assert (res["regions"]["n_valid"] == n_reads).all()
    assert int(st["edit_tasks"]) == int(ora["stats"][0]["edit_tasks"]) > 0


def test_pair_tasks_haplotagged(gpu, oracle):
    """Haplotagged reads: no alignment, the distances are 0 (same phase set and haplotype) or 1."""
    b = synth.make_batch(6, len_range=(150, 300), n_reads=9, err="hifi", haps=True, frac_partial=0.0, seed=311)
    res, st, _ = _check(gpu, oracle, b, ignore_haps=0)
    assert int(st["edit_tasks"]) == 0
    d = np.concatenate(res["dist"])
    assert d.size and np.isin(d, (0.0, 1.0)).all() and (d == 0).any() and (d == 1).any()


def test_pair_tasks_one_allele(gpu, oracle):
    """max_alleles = 1: the matrix is all ones, nothing is aligned for it."""
    b = synth.make_batch(5, len_range=(150, 300), n_reads=7, err="hifi", frac_partial=0.0, seed=312)
    res, _, _ = _check(gpu, oracle, b, max_alleles=1)
    d = np.concatenate(res["dist"])
    assert d.size == 5 * 21 and (d == 1.0).all()


def test_reassign_invalid_first_middle_last(gpu, oracle):
    """Reassignment with the untagged (invalid) reads in the first, a middle and the last position of their regions, alone and together, in
    regions of 12 and of 70 reads (a row of targets longer than a wave)."""
    parts = []
    for n_reads, seed in ((12, 320), (70, 321)):
        b = synth.make_batch(5, len_range=(100, 160), n_reads=n_reads, err="hifi", haps=True, frac_partial=0.0, seed=seed)
        reads = b["reads"].copy()
        for r, where in enumerate(([0], [n_reads // 2], [n_reads - 1], [0, n_reads // 2, n_reads - 1], [0, 1, n_reads - 2, n_reads - 1])):
            f = int(b["regions"][r]["first_read"])
            for i in where:
                reads["ps"][f + i] = -1
                reads["hp"][f + i] = -1
        parts.append(dict(b, reads=reads))
    b = synth.concat_batches(parts)
    res, st, ora = _check(gpu, oracle, b, ignore_haps=0)
    untagged = b["reads"]["ps"] < 0
    assert untagged.sum() == 2 * 10 and (res["labels"][untagged] >= 0).sum() >= 10      # the case is live: they were given to an allele
    assert int(st["edit_tasks"]) == int(ora["stats"][0]["edit_tasks"]) > 0


@pytest.mark.parametrize("n_slots", [1, 1023, 1024, 1025, 2100, 8193])
def test_compaction_offsets(gpu, oracle, n_slots):
    """Batches of 1 .. 8 193 read slots (the scan kernel's tile is 8 192 values; 1 024 was the old kernel's thread count): the sequence offsets
    of the allele records are the running sum of their lengths in slot order, the totals are the lengths of the result arrays, the records
    equal the oracle's."""
    per = 1 if n_slots == 1 else 3
    b = synth.make_batch((n_slots + per - 1) // per, len_range=(40, 60), n_reads=per, err="hifi", frac_partial=0.0, seed=330)
    if len(b["reads"]) != n_slots:          # the last region gives up the reads beyond n_slots
        cut = len(b["reads"]) - n_slots
        regions = b["regions"].copy()
        regions[-1]["n_reads"] -= cut
        b = dict(b, reads=b["reads"][:n_slots].copy(), regions=regions)
    assert len(b["reads"]) == n_slots
    P = abi.default_params()
    res = gpu.assemble(P, b)
    ora = oracle.assemble_batch(P, b)
    al = res["alleles"]
    assert len(al) == len(ora["alleles"]) > 0
    lens = al["seq_len"].astype(np.int64)
    assert np.array_equal(al["seq_off"].astype(np.int64), np.cumsum(lens) - lens)
    assert np.array_equal(al["seq_len"], ora["alleles"]["seq_len"]) and np.array_equal(al["region"], ora["alleles"]["region"])
    assert np.array_equal(res["regions"]["first_allele"], ora["regions"]["first_allele"])
    n = int(lens.sum())
    assert res["seqs"][:n].tobytes() == ora["seqs"][:n].tobytes()

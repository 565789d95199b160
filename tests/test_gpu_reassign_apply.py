"""GPU parity of the reassignment decision (otter_amd/csrc/pipeline.hip, K_reassign_apply: one wave per region, the lanes sharing the
(label, target) terms of one read) against the oracle's invalid_reassignment, on the cases in which the decision turns:
  * a one-sided read that is a shared prefix of both alleles: two labels tie in max_val, `same` is 2, no label is given;
  * one edit of difference between the two alleles inside a one-sided read of 100 and of 101 bases: min_diff = 1/100 and 1/101 around
    max_error = 0.01;
  * a one-sided read of 100 bases with 10 and with 11 substitutions: max_val = 0.90 and 0.89 around min_sim = 0.9;
  * a haplotagged batch (ignore_haps = 0) in which an untagged spanning read is labelled first and is then the only target close enough
    for a later one-sided read;
  * regions of 65 and of 130 reads: more targets than lanes;
  * max_alleles = 1: one label, min_diff stays 1.
Labels, region records, distance matrices and allele records must equal the oracle's."""
import numpy as np
import pytest
from otter_amd import abi
from helpers import rand_seq, mutate
from test_gpu_edit_masks import _put, _run, _check_against_oracle

pytestmark = pytest.mark.gpu


def _batch(regions):
    """regions: lists of (bytes, spanning_l, spanning_r, ps, hp)"""
    seqs = [rd[0] for reads in regions for rd in reads]
    arena, offs, lens = abi.pack_seqs(seqs)
    rd = np.zeros(len(seqs), dtype=abi.read_dt)
    rg = np.zeros(len(regions), dtype=abi.region_dt)
    k = 0
    for r, reads in enumerate(regions):
        rg[r]["first_read"], rg[r]["n_reads"] = k, len(reads)
        for s, spl, spr, ps, hp in reads:
            rd[k] = (int(offs[k]), int(lens[k]), spl, spr, 0, ps, hp, 0, int(lens[k]))
            k += 1
    return {"arena": arena, "reads": rd, "regions": rg}


def _sub(s, positions):
    """s with the base at every position replaced by another one"""
    for p in positions:
        s = _put(s, p, "ACGT"[("ACGT".index(chr(s[p])) + 1) % 4])
    return s


def _two_alleles(rng, n_prefix=120, n_suffix=220):
    pre = rand_seq(rng, n_prefix)
    return pre, pre + rand_seq(rng, n_suffix), pre + rand_seq(rng, n_suffix + 9)


def _spanning(a, b):
    """three spanning reads of each allele, differing behind the shared prefix only"""
    return [(a, 1, 1, -1, -1), (_sub(a, (200,)), 1, 1, -1, -1), (_sub(a, (260, 300)), 1, 1, -1, -1),
            (b, 1, 1, -1, -1), (_sub(b, (210,)), 1, 1, -1, -1), (_sub(b, (250, 310)), 1, 1, -1, -1)]


def _threshold_batch():
    rng = np.random.default_rng(4242)
    regions = []
    # 0: the tie.  reads 6, 7: prefixes of both alleles
    pre, a, b = _two_alleles(rng)
    regions.append(_spanning(a, b) + [(pre[:100], 1, 0, -1, -1), (pre[:57], 1, 0, -1, -1)])
    # 1: min_diff around max_error.  the alleles differ by one base at 50; reads 6, 7: 100 and 101 bases of allele a
    pre, a, b = _two_alleles(rng)
    b = _sub(b, (50,))
    regions.append(_spanning(a, b) + [(a[:100], 1, 0, -1, -1), (a[:101], 1, 0, -1, -1)])
    # 2: max_val around min_sim.  the alleles share nothing; reads 6, 7: 100 bases of allele a with 10 and 11 substitutions
    a, b = rand_seq(rng, 340), rand_seq(rng, 349)
    ten, eleven = range(4, 86, 9), range(4, 95, 9)
    assert len(ten) == 10 and len(eleven) == 11
    regions.append(_spanning(a, b) + [(_sub(a[:100], ten), 1, 0, -1, -1), (_sub(a[:100], eleven), 1, 0, -1, -1)])
    return _batch(regions)


@pytest.fixture(scope="module")
def threshold_batch():
    return _threshold_batch()


def test_thresholds_against_oracle(gpu, oracle, threshold_batch):
    res, st = _run(gpu, threshold_batch)
    ora = oracle.assemble_batch(abi.default_params(), threshold_batch)
    lab = ora["labels"].reshape(3, 8)
    print("reassignment thresholds: fc %s, labels of the one-sided reads %s" % (ora["regions"]["fc"].tolist(), lab[:, 6:].tolist()))
    assert ora["regions"]["fc"].tolist() == [2, 2, 2]
    assert lab[0, 6] == -1 and lab[0, 7] == -1                       # tie
    assert lab[1, 6] == lab[1, 0] and lab[1, 7] == -1                # 1/100 passes max_error (as doubles (1 - 0) - (1 - 0.01) >= 0.01), 1/101 does not
    assert lab[2, 6] == lab[2, 0] and lab[2, 7] == -1                # 0.90 passes min_sim, 0.89 does not
    _check_against_oracle(res, st, ora)


def test_single_allele_against_oracle(gpu, oracle, threshold_batch):
    """max_alleles = 1: every spanning read has label 0, no other label to differ from"""
    res, st = _run(gpu, threshold_batch, max_alleles=1)
    ora = oracle.assemble_batch(abi.default_params(max_alleles=1), threshold_batch)
    assert ora["regions"]["fc"].tolist() == [1, 1, 1] and (ora["labels"].reshape(3, 8)[:2, 6:] == 0).all()
    _check_against_oracle(res, st, ora)


def test_haplotagged_later_target_against_oracle(gpu, oracle):
    """ignore_haps = 0: the tagged spanning reads are the valid ones; read 6 spans and is untagged, so it is reassigned, and is then the
    only target within min_sim of read 7, whose 150 bases the tagged reads of its allele carry with a fifth of them changed"""
    rng = np.random.default_rng(77)
    a, b = rand_seq(rng, 1000), rand_seq(rng, 1010)
    worn = lambda s, seed: mutate(np.random.default_rng(seed), s[:150], 0.2) + s[150:]
    reads = [(worn(a, 1), 1, 1, 1, 1), (worn(a, 2), 1, 1, 1, 1), (worn(a, 3), 1, 1, 1, 1),
             (worn(b, 4), 1, 1, 1, 2), (worn(b, 5), 1, 1, 1, 2), (worn(b, 6), 1, 1, 1, 2),
             (a, 1, 1, -1, -1), (a[:150], 1, 0, -1, -1), (b[:150], 1, 0, -1, -1)]
    batch = _batch([reads])
    res, st = _run(gpu, batch, ignore_haps=0)
    ora = oracle.assemble_batch(abi.default_params(ignore_haps=0), batch)
    lab = ora["labels"]
    print("haplotagged: n_valid %d, labels %s" % (int(ora["regions"]["n_valid"][0]), lab.tolist()))
    assert int(ora["regions"]["n_valid"][0]) == 6 and lab[6] == lab[0] and lab[7] == lab[0] and lab[8] == -1
    _check_against_oracle(res, st, ora)


def _deep_region(rng, n_span, n_part):
    """two unrelated alleles of 300 and 330 bases; spanning reads with 1 % errors, one-sided reads (prefixes and suffixes) among them"""
    alleles = (rand_seq(rng, 300), rand_seq(rng, 330))
    reads = []
    for i in range(n_span + n_part):
        s = mutate(rng, alleles[int(rng.integers(0, 2))], 0.01)
        if i % 4 == 3 and sum(1 for r in reads if not (r[1] and r[2])) < n_part:
            cut = int(rng.integers(100, 280))
            reads.append((s[:cut], 1, 0, -1, -1) if rng.random() < 0.5 else (s[len(s) - cut:], 0, 1, -1, -1))
        else:
            reads.append((s, 1, 1, -1, -1))
    return reads


def test_more_targets_than_lanes_against_oracle(gpu, oracle):
    """65 and 130 reads in a region: a lane holds more than one target"""
    rng = np.random.default_rng(65130)
    batch = _batch([_deep_region(rng, 50, 15), _deep_region(rng, 100, 30)])
    res, st = _run(gpu, batch)
    ora = oracle.assemble_batch(abi.default_params(), batch)
    one_sided = (batch["reads"]["spanning_l"] & batch["reads"]["spanning_r"]) == 0
    print("deep regions: fc %s, %d one-sided reads, %d of them labelled" % (ora["regions"]["fc"].tolist(), int(one_sided.sum()), int((ora["labels"][one_sided] >= 0).sum())))
    assert batch["regions"]["n_reads"].tolist() == [65, 130] and int(one_sided.sum()) == 45 and int((ora["labels"][one_sided] >= 0).sum()) >= 30
    _check_against_oracle(res, st, ora)

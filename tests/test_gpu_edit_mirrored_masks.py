"""GPU parity of the table blocks and row codes of the reversed reads (otter_amd/csrc/pipeline.hip, K_reverse_reads).  A read that spans
only the right side is compared with the spanning reads from the other end, on reversed copies; K_reverse_reads writes each copy eight
bytes per lane and, in the same pass, its plane blocks into the second region of the per-read table and its row codes, so that these
mirrored tasks take their match masks from the table like every other task.

Regions against the oracle — reassignment decisions (labels), distance matrices, allele records:
  * right-spanning reads against spanning reads of 64 k - 1, 64 k and 64 k + 1 bases (k = 2, 3, 8): the last block of the reversed
    pattern is full, one short and one over; the copies end on every residue mod 8;
  * a right-spanning read next to a left-spanning one and one that spans neither side;
  * a spanning read with an N — its reversed copy gets no table entry, its mirrored tasks build their masks — and a right-spanning
    read with an N, whose reversed codes carry the zero row;
  * a region in which every read spans: no copy, no blocks, nothing to reassign.
The batch runs again under OTG_EDIT_MASKS=0 (no table at all, no codes) in a fresh child process; the outputs must be equal byte for byte."""
import os
import subprocess
import sys
import numpy as np
import pytest
from otter_amd import abi
from helpers import rand_seq, mutate
from test_gpu_edit_masks import _put, _run, _check_against_oracle, _flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_ENV = "OTG_TEST_EDIT_MIRRORED_DUMP"       # set for the child: where it writes what the pipeline returned

EDGE_LENS = (127, 128, 129, 191, 192, 193, 511, 512, 513)


def _batch(regions):
    """regions: lists of (bytes, spanning_l, spanning_r)"""
    seqs = [s for reads in regions for s, _, _ in reads]
    arena, offs, lens = abi.pack_seqs(seqs)
    rd = np.zeros(len(seqs), dtype=abi.read_dt)
    rg = np.zeros(len(regions), dtype=abi.region_dt)
    k = 0
    for r, reads in enumerate(regions):
        rg[r]["first_read"], rg[r]["n_reads"] = k, len(reads)
        for s, spl, spr in reads:
            rd[k] = (int(offs[k]), int(lens[k]), spl, spr, 0, -1, -1, 0, int(lens[k]))
            k += 1
    return {"arena": arena, "reads": rd, "regions": rg}


def _alleles(rng, L):
    """two unrelated alleles of L bases and three spanning reads of each (exactly L bases: substitutions only)"""
    a, b = rand_seq(rng, L), rand_seq(rng, L)
    flip = lambda s, at: _put(s, at, "ACGT"[("ACGT".index(chr(s[at])) + 1) % 4])
    return a, b, [(a, 1, 1), (flip(a, L // 3), 1, 1), (flip(a, L // 2), 1, 1), (b, 1, 1), (flip(b, L // 3), 1, 1), (flip(b, L // 2), 1, 1)]


def _mirrored_batch():
    rng = np.random.default_rng(6465)
    regions = []
    for n, L in enumerate(EDGE_LENS):
        a, b, reads = _alleles(rng, L)
        cut = (9 * L) // 10 - n % 8                                        # the copies' lengths cover the residues mod 8
        regions.append(reads + [(mutate(rng, a, 0.03)[-cut:], 0, 1), (mutate(rng, b, 0.03)[-(cut - 9):], 0, 1)])
    a, b, reads = _alleles(rng, 400)                                        # right-spanning, left-spanning, neither, side by side
    regions.append(reads + [(a[-250:], 0, 1), (b[:260], 1, 0), (a[70:330], 0, 0), (b[-134:], 0, 1)])
    a, b, reads = _alleles(rng, 300)                                        # N in a spanning read and in a right-spanning one
    reads[1] = (_put(reads[1][0], 10, "N"), 1, 1)
    regions.append(reads + [(a[-200:], 0, 1), (_put(_put(b[-203:], 0, "N"), 202, "N"), 0, 1)])
    a, b, reads = _alleles(rng, 320)                                        # every read spans
    regions.append(reads)
    return _batch(regions)


@pytest.fixture(scope="module")
def mirrored_batch():
    return _mirrored_batch()


def test_mirrored_against_oracle(gpu, oracle, mirrored_batch):
    res, st = _run(gpu, mirrored_batch)
    ora = oracle.assemble_batch(abi.default_params(), mirrored_batch)
    right_only = (mirrored_batch["reads"]["spanning_l"] == 0) & (mirrored_batch["reads"]["spanning_r"] == 1)
    print("mirrored: %d right-spanning reads, %d of them labelled; fc %s" %
          (int(right_only.sum()), int((ora["labels"][right_only] >= 0).sum()), ora["regions"]["fc"].tolist()))
    assert (ora["regions"]["status"] == 0).all() and (ora["regions"]["fc"] == 2).all()
    assert int(right_only.sum()) == 2 * len(EDGE_LENS) + 4 and int((ora["labels"][right_only] >= 0).sum()) >= 2 * len(EDGE_LENS)
    _check_against_oracle(res, st, ora)
    if os.environ.get(DUMP_ENV):
        np.savez(os.environ[DUMP_ENV], **_flat(res))


def test_mirrored_switch_child(gpu, mirrored_batch, tmp_path):
    """OTG_EDIT_MASKS=0 in a fresh process: no table, so the mirrored tasks build their masks pair by pair; the same outputs"""
    res, _ = _run(gpu, mirrored_batch)
    gpu.trim()
    path = str(tmp_path / "no_table.npz")
    env = dict(os.environ, OTG_EDIT_MASKS="0")
    env[DUMP_ENV] = path
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_edit_mirrored_masks.py::test_mirrored_against_oracle"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    mine = _flat(res)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(mine)
        for k in z.files:
            assert np.array_equal(z[k], mine[k]), k

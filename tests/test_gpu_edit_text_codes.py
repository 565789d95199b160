"""GPU parity of the text row codes of the bit-parallel edit tiers (otter_amd/csrc/myers_edit.hip, `load_group`): a task whose pattern has
blocks in the per-read plane table reads its text as one row code per byte, written once per run by read_masks_kernel, instead of
translating the bytes through the LDS byte map pair after pair.

Small regions of 3 to 8 reads against the oracle — distance matrices, labels after reassignment, allele records:
  * read lengths 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 in all-against-all regions, so that texts shorter than 8 bytes and texts whose
    length mod 8 is 0, 1 and 7 meet patterns on both sides of the 64-row block edges; the reads of a region are unrelated, so every pair
    longer than the wavefront pass's score cap of 48 reaches the tiers;
  * unrelated reads of about 1 400 bases, whose pairs leave <1,8> (456 rows of band) for <2,8>, with one-sided reads to reassign;
  * a text with N at positions 0, 7, 8 and last under patterns of pure A C G T: the code path and its zero row;
  * a read with N that is the pattern of its pairs: it has no table blocks, so its pairs translate through the byte map in the same waves
    in which the other pairs of the region read codes;
  * a `-r` batch whose reads realignment shortened: the codes are written from the reads' current offsets and lengths.
The first batch runs again under OTG_EDIT_TEXT_CODES=0 (every task on the byte map) in a fresh child process; the outputs must be equal
byte for byte."""
import os
import subprocess
import sys
import numpy as np
import pytest
from otter_amd import abi, synth
from helpers import rand_seq, mutate
from test_gpu_edit_masks import _put, _run, _check_against_oracle, _flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_ENV = "OTG_TEST_EDIT_TEXT_CODES_DUMP"       # set for the child: where it writes what the pipeline returned


def _batch(regions):
    """regions: lists of (bytes, spanning_l, spanning_r)"""
    seqs = [s for reads in regions for s, _, _ in reads]
    arena, offs, lens = abi.pack_seqs(seqs)
    rd = np.zeros(len(seqs), dtype=abi.read_dt)
    rg = np.zeros(len(regions), dtype=abi.region_dt)
    k = 0
    for r, reads in enumerate(regions):
        assert 3 <= len(reads) <= 8
        rg[r]["first_read"], rg[r]["n_reads"] = k, len(reads)
        for s, spl, spr in reads:
            rd[k] = (int(offs[k]), int(lens[k]), spl, spr, 0, -1, -1, 0, int(lens[k]))
            k += 1
    return {"arena": arena, "reads": rd, "regions": rg}


def _code_batch():
    rng = np.random.default_rng(808)
    regions = []
    for lens in ((1, 7, 8, 9, 63, 64, 65, 127), (129, 128, 127, 65, 64, 63, 9, 8), (64, 128, 7), (129, 65, 1, 9)):
        regions.append([(rand_seq(rng, L), 1, 1) for L in lens])
    a, b = rand_seq(rng, 1400), rand_seq(rng, 1393)          # mod 8: 0 and 1
    regions.append([(a, 1, 1), (mutate(rng, a, 0.1), 1, 1), (b, 1, 1), (mutate(rng, b, 0.1), 1, 1), (rand_seq(rng, 1407), 1, 1),
                    (mutate(rng, a, 0.05)[:900], 1, 0), (mutate(rng, b, 0.05)[-777:], 0, 1)])
    # N in the text under pure patterns: the text is the shorter read of its pairs
    p1, p2, p3 = rand_seq(rng, 130), rand_seq(rng, 131), rand_seq(rng, 200)
    t = rand_seq(rng, 100)
    for at in (0, 7, 8, 99):
        t = _put(t, at, "N")
    regions.append([(p1, 1, 1), (p2, 1, 1), (p3, 1, 1), (t, 1, 1), (mutate(rng, p1, 0.03), 1, 1), (_put(rand_seq(rng, 9), 8, "N"), 1, 1)])
    # N in the pattern: the longest read of the region, no table blocks; the other pairs of the region keep theirs
    q = _put(_put(rand_seq(rng, 260), 0, "N"), 131, "N")
    regions.append([(q, 1, 1), (rand_seq(rng, 250), 1, 1), (rand_seq(rng, 249), 1, 1), (rand_seq(rng, 185), 1, 1), (rand_seq(rng, 64), 1, 1),
                    (mutate(rng, q, 0.04)[:170], 1, 0)])
    return _batch(regions)


@pytest.fixture(scope="module")
def code_batch():
    return _code_batch()


def test_text_codes_against_oracle(gpu, oracle, code_batch):
    res, st = _run(gpu, code_batch)
    ora = oracle.assemble_batch(abi.default_params(), code_batch)
    # most pairs lie beyond the wavefront pass's score cap (48 for these lengths, 1.0 x sqrt(1400) < 48): the tiers finish them
    n = code_batch["regions"]["n_reads"].astype(np.int64)
    far = 0
    for r, d in enumerate(res["dist"]):
        if res["regions"]["status"][r] != 0 or len(d) == 0:
            continue
        f = int(code_batch["regions"]["first_read"][r])
        L = code_batch["reads"]["seq_len"][f:f + int(n[r])].astype(np.int64)
        L = L[(code_batch["reads"]["spanning_l"][f:f + int(n[r])] & code_batch["reads"]["spanning_r"][f:f + int(n[r])]) != 0]
        iu = np.triu_indices(len(L), 1)
        far += int((np.rint(d * np.maximum(L[iu[0]], L[iu[1]])) > 48).sum())
    print("text codes: %d regions ok of %d, %d edit tasks, %d pairs beyond the wavefront cap" %
          (int((res["regions"]["status"] == 0).sum()), len(n), int(st["edit_tasks"]), far))
    assert int((res["regions"]["status"] == 0).sum()) == len(n) and far >= 60
    _check_against_oracle(res, st, ora)
    if os.environ.get(DUMP_ENV):
        np.savez(os.environ[DUMP_ENV], **_flat(res))


def test_text_codes_realigned_reads_against_oracle(gpu, oracle):
    """-r: realignment moves seq_off and shortens reads before the codes are written"""
    b = synth.make_batch(3, len_range=(600, 1400), n_reads=8, err="ont", realign=True, frac_clipped=0.5, frac_partial=0.15, seed=88)
    trimmed = gpu.realign_reads(abi.default_params(realign=1), b)
    moved = trimmed["seq_off"] > b["reads"]["seq_off"]
    assert moved.any() and (trimmed["seq_len"] < b["reads"]["seq_len"]).any()
    res, st = _run(gpu, b, realign=1)
    ora = oracle.assemble_batch(abi.default_params(realign=1), b)
    _check_against_oracle(res, st, ora)


def test_text_codes_switch_child(gpu, code_batch, tmp_path):
    """OTG_EDIT_TEXT_CODES=0 in a fresh process: every task translates its text through the byte map; the same outputs"""
    res, _ = _run(gpu, code_batch)
    gpu.trim()
    path = str(tmp_path / "byte_map.npz")
    env = dict(os.environ, OTG_EDIT_TEXT_CODES="0")
    env[DUMP_ENV] = path
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_edit_text_codes.py::test_text_codes_against_oracle"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    mine = _flat(res)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(mine)
        for k in z.files:
            assert np.array_equal(z[k], mine[k]), k

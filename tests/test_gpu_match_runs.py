"""GPU parity of the extend step the wavefront kernels share (otter_amd/csrc/otg_match_queue.hpp: sweep probe, match-run queue, drain passes,
wave-wide step): pairs of at most ~2.5 kb built to walk every branch of the drain, against the oracle — edit scores, gap-affine scores and op
strings, in exact mode and under wfadaptive(10, 50, 1), end-to-end and ends-free.  tests/test_gpu_alt_paths.py re-runs this file with each
kernel family as the first tier that sees the pairs.

  1. run-length boundaries: pattern and text differ by single substitutions and one-base indels placed so that the exact run behind an edit is
     7 / 8 / 9 bases long (the sweep's 8-byte probe), 23 / 24 / 25 (+ 16), 87 / 88 / 89 (+ 64), 151 / 152 / 153 (a second 64-byte pass), 31 ... 97
     around the multiples of 32 (packed probes, the second probe inside the sweep of the LDS tiers) and 600 (the wave-wide step, more than one
     512-byte iteration); every length also as the LAST run of a pair, where the end of a sequence and not a mismatch limits it — both
     sequences ending together, and one of them running on;
  2. runs alive after the first pass: one edit in a random sequence (one or two runs: the wave-wide step) and one substitution in 400 copies of a
     5-base unit (behind the edit every diagonal at a multiple of 5 carries a long run: many more than four for several passes);
  3. the queue filling DURING a sweep: homopolymer (and two-base repeat) pairs, free at the beginning on both sides, whose D start diagonals all
     carry long runs at score 0.  D by the launchers' instantiations (window CAP, queue QCAP, waves per pair NW; a sweep drains on the way when
     qn + 64 > QCAP, the pipelined kernel when qn + 128 > QCAP):
       250   gap-affine LDS tier <256, 256> (admits 252);
       800   edit LDS tier <1024, 512> inside its window;
       1000  gap-affine <1024, 256, 4 waves> (admits 1020) and the byte-probe tier <1024, 1024>;
       1500  edit LDS tier <1024, 512> on its global row, and <4096, 1024>;
       2040  edit byte-probe tier <2048, 2048> (admits 2048);
       2400  edit <16384, 256, 8 waves>, <16384, 2048> and the HBM row; gap-affine <4096, 256, 8 waves>, the HBM rings <0, 2048>, the exact
             HBM-row tier <4096, 512, 4 waves> and the generic kernel (2048);
       4401  the exact HBM-row tier <12288, 512, 4 waves> behind the 4096 one (which admits 3956).
     The one-wave gap-affine LDS tier <1024, 1024> admits 956 diagonals and would need 961: no pair can fill its queue during a sweep.
"""
import numpy as np
import pytest
from helpers import rand_seq, pair_tasks
from otter_amd import abi

pytestmark = pytest.mark.gpu

RUNS = [7, 8, 9, 23, 24, 25, 87, 88, 89, 151, 152, 153, 31, 32, 33, 63, 64, 65, 95, 96, 97, 600]
WIDE = [250, 800, 1000, 1500, 2040, 2400, 4401]


def _other(c, avoid=b""):
    return bytes([next(x for x in b"ACGT" if x != c and x not in avoid)])


def _edited(rng, runs, kinds):
    """pattern, text: a 40-base head, then per run an edit and `run` equal bases.  The base an edit puts on the run's diagonal differs from what
    the other sequence holds there, on both sides of the run, so the exact run on that diagonal is `run` bases long"""
    a, b = bytearray(rand_seq(rng, 40)), bytearray()
    b += a
    for run, kind in zip(runs, kinds):
        r = rand_seq(rng, run)
        last = a[-1]
        if kind == 0:                      # substitution
            x = _other(r[0])
            a += x; b += _other(x[0], avoid=r[:1])
        elif kind == 1:                    # a base only the pattern has: differs from its neighbours, so neither diagonal runs on through it
            a += _other(r[0], avoid=bytes([last]))
        else:                              # a base only the text has
            b += _other(r[0], avoid=bytes([last]))
        a += r; b += r
    return bytes(a), bytes(b)


def _pairs():
    rng = np.random.default_rng(2051)
    pairs = []
    # 1. every run length between two edits, in three orders and with the three kinds of edit rotating
    for rep in range(3):
        order = [RUNS[i] for i in rng.permutation(len(RUNS))]
        a, b = _edited(rng, order + [50], [(j + rep) % 3 for j in range(len(order) + 1)])
        pairs.append((a, b) if rep != 1 else (b, a))
    # ... and as the last run of the pair: both sequences end with it, or one of them runs on
    for i, run in enumerate(RUNS):
        a, b = _edited(rng, [run], [i % 3])
        pairs.append((a, b))
        tail = rand_seq(rng, 5)
        pairs.append((a + tail, b) if i % 2 else (a, b + tail))
    # 2. one or two runs alive / many more than four
    a = rand_seq(rng, 2000)
    pairs.append((a, a[:1000] + _other(a[1000]) + a[1001:]))
    pairs.append((a, a[:700] + a[701:]))
    tr = b"ACGTT" * 400
    pairs.append((tr, tr[:203] + _other(tr[203]) + tr[204:]))
    pairs.append((tr[:203] + _other(tr[203]) + tr[204:], tr + b"ACG"))
    return pairs


def _wide():
    """3. D = 2 F + 1 start diagonals over sequences of F + 200 bases; begins free (the alignment must still end in the corner), and all four ends free"""
    pairs, forms = [], []
    for i, D in enumerate(WIDE):
        F = D // 2
        L = F + 200
        p, t = b"A" * L, b"A" * L
        if i % 2:
            t = t[:L // 2] + b"C" + t[L // 2 + 1:]           # every diagonal meets the substitution at another offset
        pairs += [(p, t), (p, t)]
        forms += [(F, 0, D - 1 - F, 0), (F, F, D - 1 - F, D - 1 - F)]
    L = 2400                                                 # two-base repeat: every second start diagonal carries a run
    pairs += [(b"AC" * (L // 2), b"AC" * (L // 2)), (b"AC" * (L // 2), b"AC" * (L // 2 - 1) + b"AA")]
    forms += [(2200, 2200, 2200, 2200), (2200, 0, 2200, 0)]
    return pairs, forms


@pytest.fixture(scope="module")
def batch():
    """one batch for every test of the file: the pairs of 1. and 2. end-to-end and ends-free (what is left of the longer sequence is free, and two
    bases more), the pairs of 3. with their forms"""
    pairs = _pairs()
    ef = [(0, max(len(a) - len(b), 0) + 2, 0, max(len(b) - len(a), 0) + 2) for a, b in pairs]
    wide, wforms = _wide()
    assert max(max(len(a), len(b)) for a, b in pairs + wide) <= 2500
    return pair_tasks(pairs + pairs + wide, [None] * len(pairs) + ef + wforms)


@pytest.fixture
def adaptive(gpu, oracle):
    """both sides in wfadaptive(10, 50, 1); restored to exact afterwards"""
    gpu.set_heuristic(abi.OTG_HEURISTIC_WFADAPTIVE, 10, 50, 1)
    oracle.set_heuristic(1, 10, 50, 1)
    yield
    gpu.set_heuristic(abi.OTG_HEURISTIC_NONE, 10, 50, 1)
    oracle.set_heuristic(0, 10, 50, 1)


def _check_edit(gpu, oracle, batch):
    arena, tasks = batch
    got = gpu.edit_distance_batch(arena, tasks)
    exp = oracle.edit_distance_batch(arena, tasks)
    assert np.array_equal(got, exp), [(int(i), int(got[i]), int(exp[i])) for i in np.flatnonzero(got != exp)[:8]]


def _check_affine(gpu, oracle, batch):
    arena, tasks = batch
    gs, gc = gpu.affine_align_batch(arena, tasks)
    es, ec = oracle.affine_align_batch(arena, tasks)
    assert np.array_equal(gs, es), [(int(i), int(gs[i]), int(es[i])) for i in np.flatnonzero(gs != es)[:8]]
    bad = [i for i in range(len(tasks)) if gc[i] != ec[i]]
    assert not bad, bad[:10]


def test_match_runs_edit_exact(gpu, oracle, batch):
    _check_edit(gpu, oracle, batch)


def test_match_runs_affine_exact(gpu, oracle, batch):
    _check_affine(gpu, oracle, batch)


def test_match_runs_edit_adaptive(gpu, oracle, batch, adaptive):
    _check_edit(gpu, oracle, batch)


def test_match_runs_affine_adaptive(gpu, oracle, batch, adaptive):
    _check_affine(gpu, oracle, batch)

"""GPU: which half of the register tiers' score loop ends an alignment, and which halves a score skips.

`wfa_affine_reg_kernel` runs two scores per trip of its score loop: score s in a body compiled for the even scores (M rows of set 0), score
s + 1 in one compiled for the odd scores (set 1).  An alignment may end after either half, an unreachable score writes `rowtab[s] = -1` and
touches no slot, and queue, drain and fold-back exist once per body.  Every batch runs under penalties (4, 6, 2) — g = 2, (2, 4, 1) in units
of g: a mismatch costs 2, a gap of G bases 3 + G — and is compared with the oracle on score, op string and cells;
`Context.affine_last_routing` must say that the routed register tier finished every alignment (a fall-through to tier A would hide a body
that gives up or goes wrong).  The final scores are conditions on the inputs and asserted against the oracle, in units of g:

  0  identical sequences: the exit after the very first half;
  2  one mismatch;                       4  a gap of one base;
  5  a gap of two bases: the first exit in the odd half;
  6  a gap of three bases;               7  a gap of four bases.

Scores 1 and 3 are the unreachable ones: nothing costs 1, and 3 would be a gap of no bases.  Both are odd, so both fall to the odd body (a
final score of 2 passes score 1, one of 4 and more passes both); the even body never sees an unreachable score below the end of an
alignment, since M[s-2] + mismatch always exists.  The same six final scores run as ends-free tasks in the forms 0, 1, 2 and 4 of
`test_gpu_affine_routing._ends_free` (score 0 then starts on a hundred and more diagonals), and a batch of ONT-like pairs and of pairs made
of exact runs beyond 64 bases, about 1 200 bases each, keeps queue, drain and fold-back busy in both bodies over 60 to 200 scores, ending
in either.  These are the 1024 window's (one wave, 40 to 1 400 bases).  The 1536, 2048 and 4096 windows (one, two and four waves) get the
insertion pairs of the routing test: a random insertion of G and of G + 1 bases behind a core of 900 bases ends in the two bodies; the sequences
stay within 3 500 bases.  (The 8192 window only runs on sequences beyond 4 096 bases and is left to the routing test.)
The inputs were established on the parent of the change that split the loop: the file passes there with the same routing."""
import numpy as np
import pytest
from helpers import rand_seq, mutate, pair_tasks
from test_gpu_affine_routing import PEN, _insertion_pair, _ends_free, _expected_tiers, _check_chain, _check_finishes
from test_gpu_affine_queue_exits import _runs_pair

pytestmark = pytest.mark.gpu

G_UNIT = 2                                    # gcd of (4, 6 + 2, 2)
FINALS = (0, 2, 4, 5, 6, 7)                   # final scores in units of g
CORE = 900
# per window: the insertion lengths; each runs as G and as G + 1 (from test_gpu_affine_routing.WINDOW's end-to-end ranges)
WINDOW_G = {1: (620, 650, 680, 704), 2: (880, 910, 940, 964), 3: (1300, 1420, 1540, 1652)}


def _edited(rng, n, units):
    """a random sequence of n bases and a copy whose optimal alignment costs exactly `units`: identical, one mismatch, or one gap of units - 3 bases"""
    a = rand_seq(rng, n)
    mid = n // 2
    if units == 0:
        return a, a
    if units == 2:
        return a, a[:mid] + b"ACGT"[(b"ACGT".index(a[mid]) + 1) % 4:][:1] + a[mid + 1:]
    return a, a[:mid] + a[mid + units - 3:]


def _build_e2e():
    rng = np.random.default_rng(6100)
    pairs, want = [], []
    for n in (40, 1400):
        for j, u in enumerate(FINALS):
            a, b = _edited(rng, n, u)
            pairs.append((a, b) if j % 2 else (b, a)); want.append(u)
    return pairs, None, want


def _build_ends_free():
    rng = np.random.default_rng(6200)
    pairs, forms, want = [], [], []
    for j, u in enumerate((0, 2, 4, 5, 6, 7, 5, 4, 0, 2, 7, 6)):
        a, b = _edited(rng, 300 + 90 * j, u)
        pr, f = _ends_free(rng, a, b, (0, 1, 2, 4)[j % 4], 100)
        pairs.append(pr); forms.append(f); want.append(u)
    return pairs, forms, want


def _build_long():
    rng = np.random.default_rng(6300)
    pairs = []
    for rep in range(4):
        a = rand_seq(rng, 1200)
        pairs.append((a, mutate(rng, a, 0.08)))
    for rep in range(4):
        pairs.append(_runs_pair(rng, rep))
    # the last pair again with one more base of gap at its end: the other parity of the same path
    a, b = pairs[-1]
    pairs.append((a + b"A", b))
    return pairs, None, None


def _build_window(tier):
    def build():
        rng = np.random.default_rng(6400 + tier)
        core = rand_seq(rng, CORE)
        pairs, want = [], []
        for i, G in enumerate(WINDOW_G[tier]):
            ins = rand_seq(rng, G + 1)
            for g in (G, G + 1):
                pairs.append(_insertion_pair(core, ins[:g], CORE, i % 2)); want.append(3 + g)
        return pairs, None, want
    return build


BUILDERS = {"e2e": _build_e2e, "ends_free": _build_ends_free, "long": _build_long}
BUILDERS.update({"window%d" % t: _build_window(t) for t in WINDOW_G})
_cache = {}


def _batch(name, oracle):
    if name not in _cache:
        pairs, forms, want = BUILDERS[name]()
        arena, tasks = pair_tasks(pairs, forms)
        _cache[name] = (arena, tasks, want, oracle.affine_align_batch(arena, tasks, *PEN, want_cells=True))
    return _cache[name]


def _run(gpu, oracle, name, tier, max_len):
    arena, tasks, want, (es, ec, ecells) = _batch(name, oracle)
    assert 8 <= len(tasks) <= 16
    assert max(int(tasks["pattern_len"].max()), int(tasks["text_len"].max())) <= max_len
    # conditions on the inputs: the final scores are what the construction says, and both bodies end alignments
    units = es.astype(np.int64) // G_UNIT
    assert np.all(es % G_UNIT == 0)
    if want is not None:
        assert units.tolist() == list(want), (name, units.tolist())
    assert np.any(units % 2 == 0) and np.any(units % 2 == 1), (name, units.tolist())
    gs, gc, gcells = gpu.affine_align_batch(arena, tasks, *PEN, want_cells=True)
    r = gpu.affine_last_routing(len(tasks))
    print("%s: final scores in units of g %s" % (name, units.tolist()))
    assert np.array_equal(gs, es), (name, [(int(i), int(gs[i]), int(es[i])) for i in np.flatnonzero(gs != es)[:8]])
    bad = [i for i in range(len(tasks)) if gc[i] != ec[i]]
    assert not bad, (name, bad[:10])
    assert np.array_equal(gcells, ecells), name
    _check_chain(name, tasks, es, r)
    assert np.all(_expected_tiers(tasks, r, mask=31) == tier), (name, _expected_tiers(tasks, r, mask=31).tolist())      # a condition on the inputs
    _check_finishes(name, r)                                                                                            # finished == routed, exactly
    return units, r


def test_final_scores_end_to_end(gpu, oracle):
    """Final scores 0, 2, 4, 5, 6, 7 at 40 and at 1 400 bases: the exit after the first half of the first trip, after the odd half, and the
    unreachable scores 1 and 3 on the way."""
    _run(gpu, oracle, "e2e", 0, 1400)


def test_final_scores_ends_free(gpu, oracle):
    """The same final scores behind a free begin of 100 bases and more (forms 0, 1, 2 and 4): score 0 is a sweep over every start diagonal."""
    _run(gpu, oracle, "ends_free", 0, 1400)


def test_many_scores_queue_in_both_halves(gpu, oracle):
    """ONT-like pairs and pairs of exact runs beyond 64 bases, about 1 200 bases: queue, drain and fold-back in both bodies over many scores."""
    units, r = _run(gpu, oracle, "long", 0, 1400)
    assert int(units.min()) >= 20, units.tolist()


@pytest.mark.parametrize("tier", sorted(WINDOW_G), ids=["one-wave-1536", "two-wave-2048", "four-wave-4096"])
def test_window_ends_in_either_half(gpu, oracle, tier):
    """An insertion of G and of G + 1 bases behind the core: final scores 3 + G and 4 + G, the two bodies' exits, on the one-wave 1536 window and
    on the multi-wave windows, whose export row and barrier belong to a body each."""
    _run(gpu, oracle, "window%d" % tier, tier, 3500)

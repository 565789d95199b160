"""GPU: the regimes of the register tiers' score ranges — where a range starts, what clamps it, what clips it — on every window but the widest.

`wfa_affine_reg_kernel` takes the diagonals [lo, hi] of a score from a closed form (affine_score_range.hpp): the start range of score 0,
one diagonal more per side and score from score 2 on, clamped to [-pl, tl] and clipped to the diamond of the score bound U.  Score 0 runs
in a body of its own in front of the score loop, score 1 is a row-table entry, the loop starts at score 2.  Every batch runs under penalties
(4, 6, 2) — g = 2, (2, 4, 1) in units of g — and is compared with the oracle on score, op string and cells;
`Context.affine_last_routing` must say that the routed register tier finished every alignment, and that tier must be the window the batch
was built for (1024 and 1536: one wave; 2048: two waves; 4096: four waves; sequences stay within 3 500 bases).

What selects the window is the wanted width, about (start range + end range) / 2 + U, and the bound pass gives a bound only when the begins
or the ends are free over fewer than 40 bases in all.  So an alignment that ends within the first scores reaches a wide window only through
a wide END range, and a start range of more than one slot (128 diagonals) survives the clip to the diamond only under a loose bound.  Three
batches per window, built within that:

  finals   identical pairs (the alignment ends inside score 0), one mismatch (score 2, the first half of the loop's first trip), a gap of one
           base and of two (scores 4 and 5, the two halves of the second trip).  Both ends are free over the whole sequence, which makes the
           wanted window about the sequences' length L (900, 1 200, 1 700, 2 600 per window) whatever U is, and keeps the diamond out of
           the ranges: they are the start diagonal widened by one per side and score.  The 1024 window also runs the pairs end to end at 40
           and at 1 200 bases, where U is the optimum and the diamond clips every range.
  bound    U equal to the optimum: end-to-end pairs with a mismatch at every third base, as long as it takes for the optimum to fill the
           window (U + 8 diagonals), so the diamond clips the ranges from the first scores on; U loose: an insertion of G bases behind a
           core of 900, end to end, where the bound is about 2 G for an optimum of G + 3 (the pairs of test_gpu_affine_routing); and U loose
           behind a free begin of 640 bases and more (that test's begin-free pairs): a start range of more than one slot.
  clamps   a short pattern against a long text, and the reverse, so that the ranges run into -pl (into tl) and stay there.  The diagonal -pl
           is where deleting the whole pattern leads, at exactly the score such a gap costs, so the clamp only binds before the end of an
           alignment that cannot end that way, and only where the diamond is wider than the matrix: the short sequence is drawn from A and
           C, the long one from G and T (nothing matches); 20 bases of the short one's begin are free, and the long one's end but for KEPT
           bases — those have to be paid for (KEPT mismatches, then a gap over the rest of the short sequence), which keeps the alignment
           going beyond the score at which the clamp binds.  The long sequence selects the window.  That the clamp binds — before the
           final score, with the diamond wider than the clamp there — is asserted from the closed form restated below.

Conditions on the inputs (final scores, which window, bound tight or loose, start range, clamp binding) are asserted beside the results.  The
inputs were established on the parent of the change that introduced the closed form: the file passes there with the same routing."""
import numpy as np
import pytest
from helpers import rand_seq, pair_tasks
from test_gpu_affine_routing import (PEN, WINDOW, CUT, FREE_KINDS, SLACK, _insertion_pair, _ends_free, _expected_tiers, _check_chain, _check_finishes,
                                     affine_window)

pytestmark = pytest.mark.gpu

G_UNIT = 2                                    # gcd of (4, 6 + 2, 2)
FINALS = (0, 2, 4, 5)                         # final scores in units of g
LENGTH = {0: 900, 1: 1200, 2: 1700, 3: 2600}  # finals: the wanted window is about (pl + tl) / 2 + U + 8 diagonals
DENSE = {0: 600, 1: 1800, 2: 2700, 3: 3400}   # bound, tight: a mismatch at every third base, the wanted window about 2 n / 3 + 8
# clamps: (the short sequence, how much of the long one's end is not free, the long sequence); the wanted window is about long / 2 + U
CLAMP = {0: (40, 10, 800), 1: (40, 10, 2200), 2: (40, 10, 3300), 3: (400, 30, 3400)}
SHORT_FREE = 20


def _edited(rng, n, units):
    """a random sequence of n bases and a copy whose optimal alignment costs exactly `units`: identical, one mismatch, or one gap of units - 3 bases"""
    a = rand_seq(rng, n)
    mid = n // 2
    if units == 0:
        return a, a
    if units == 2:
        return a, a[:mid] + b"ACGT"[(b"ACGT".index(a[mid]) + 1) % 4:][:1] + a[mid + 1:]
    return a, a[:mid] + a[mid + units - 3:]


def _build_finals(tier):
    def build():
        rng = np.random.default_rng(7100 + tier)
        pairs, forms, want = [], [], []
        for n in (LENGTH[tier], LENGTH[tier] - 90):
            for j, u in enumerate(FINALS):
                a, b = _edited(rng, n, u)
                p, t = (a, b) if j % 2 else (b, a)
                pairs.append((p, t)); forms.append((0, len(p), 0, len(t))); want.append(u)      # (pattern_begin_free, pattern_end_free, text_begin_free, text_end_free)
        if tier == 0:
            for n in (40, 1200):
                for j, u in enumerate(FINALS):
                    a, b = _edited(rng, n, u)
                    pairs.append((b, a) if j % 2 else (a, b)); forms.append(None); want.append(u)
        return pairs, forms, want
    return build


def _build_bound(tier):
    def build():
        rng = np.random.default_rng(7200 + tier)
        pairs, forms = [], []
        for j in range(4):                                             # U tight
            a = rand_seq(rng, DENSE[tier] - 45 * j)
            b = bytearray(a)
            for i in range(1, len(a), 3):
                b[i] = b"ACGT"[(b"ACGT".index(b[i]) + 1 + int(rng.integers(0, 3))) % 4]
            pairs.append((a, bytes(b)) if j % 2 else (bytes(b), a)); forms.append(None)
        L, g_e2e, g_free, same_side = WINDOW[tier]                     # U loose
        core = rand_seq(rng, L)
        for i, G in enumerate(list(g_e2e)[1:9:2]):
            pairs.append(_insertion_pair(core, rand_seq(rng, G), L, i % 2)); forms.append(None)
        for G, kind in list(zip(g_free, FREE_KINDS))[2:8]:             # U loose behind a wide free begin (the layout of that test's _build_window)
            on_pattern = (kind != 2) == same_side
            p, t = _insertion_pair(core, rand_seq(rng, G + (SLACK[kind] if same_side else 0)), 0, on_pattern)
            pr, f = _ends_free(rng, p, t, kind, CUT)
            pairs.append(pr); forms.append(f)
        return pairs, forms, None
    return build


def _two_letter(rng, n, letters):
    return bytes(letters[int(i)] for i in rng.integers(0, 2, n))


def _build_clamps(tier):
    def build():
        rng = np.random.default_rng(7300 + tier)
        n_short, kept, n_long = CLAMP[tier]
        pairs, forms = [], []
        for j in range(4):
            n = n_long - 40 * j
            short, long_ = _two_letter(rng, n_short, b"AC"), _two_letter(rng, n, b"GT")
            # (pattern_begin_free, pattern_end_free, text_begin_free, text_end_free)
            pairs.append((short, long_)); forms.append((SHORT_FREE, 0, 0, n - kept))      # short pattern, long text: -pl
            short, long_ = _two_letter(rng, n_short, b"GT"), _two_letter(rng, n, b"AC")
            pairs.append((long_, short)); forms.append((0, n - kept, SHORT_FREE, 0))      # long pattern, short text: tl
        # kept mismatches, then a gap over what is left of the short sequence behind its free begin
        return pairs, forms, [2 * kept + 3 + n_short - SHORT_FREE - kept] * 8
    return build


BUILDERS = {}
for _t in LENGTH:
    BUILDERS.update({"finals%d" % _t: _build_finals(_t), "bound%d" % _t: _build_bound(_t), "clamps%d" % _t: _build_clamps(_t)})
_cache = {}


def _batch(name, oracle):
    if name not in _cache:
        pairs, forms, want = BUILDERS[name]()
        arena, tasks = pair_tasks(pairs, forms)
        _cache[name] = (arena, tasks, want, oracle.affine_align_batch(arena, tasks, *PEN, want_cells=True))
    return _cache[name]


def _run(gpu, oracle, name, tier):
    arena, tasks, want, (es, ec, ecells) = _batch(name, oracle)
    assert 8 <= len(tasks) <= 16
    assert max(int(tasks["pattern_len"].max()), int(tasks["text_len"].max())) <= 3500
    assert np.all(es % G_UNIT == 0)
    units = es.astype(np.int64) // G_UNIT
    if want is not None:
        assert units.tolist() == list(want), (name, units.tolist())      # a condition on the inputs
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
    return tasks, units, r


def _range(t, U, s):
    """affine_score_range.hpp restated in plain integers for task t under the bound U: (lo, hi, which of the two clamps set them) of score s >= 2"""
    pl, tl, ef = int(t["pattern_len"]), int(t["text_len"]), int(t["endsfree"]) != 0
    kend = tl - pl
    elo = kend - (int(t["text_end_free"]) if ef else 0)
    ehi = kend + (int(t["pattern_end_free"]) if ef else 0)
    lo0 = max(-int(t["pattern_begin_free"]), -pl) if ef else 0
    hi0 = min(int(t["text_begin_free"]), tl) if ef else 0
    lo0, hi0 = max(lo0, elo - U), min(hi0, ehi + U)
    lo, hi = lo0 - (s - 2), hi0 + (s - 2)
    lo_clamped = lo < -pl and -pl >= elo - (U - s)
    hi_clamped = hi > tl and tl <= ehi + (U - s)
    return max(lo, -pl, elo - (U - s)), min(hi, tl, ehi + (U - s)), lo_clamped, hi_clamped


TIERS = sorted(LENGTH)
IDS = ["one-wave-1024", "one-wave-1536", "two-wave-2048", "four-wave-4096"]


@pytest.mark.parametrize("tier", TIERS, ids=IDS)
def test_first_scores(gpu, oracle, tier):
    """Final scores 0, 2, 4 and 5: score 0 alone, and the two halves of the loop's first two trips."""
    _run(gpu, oracle, "finals%d" % tier, tier)


@pytest.mark.parametrize("tier", TIERS, ids=IDS)
def test_bound_tight_and_loose(gpu, oracle, tier):
    """Four pairs whose bound is the optimum itself, four whose bound is far above it, and six with a loose bound behind a wide free begin."""
    tasks, units, r = _run(gpu, oracle, "bound%d" % tier, tier)
    U = r["bound"].astype(np.int64)
    starts = np.array([affine_window(tasks[i], int(U[i]))[0] for i in range(len(tasks))])
    print("  bound %s optimum %s starts %s" % (U.tolist(), units.tolist(), starts.tolist()))
    assert np.all(U[:4] == units[:4]), (U.tolist(), units.tolist())
    assert np.all(2 * U[4:8] >= 3 * units[4:8]), (U.tolist(), units.tolist())
    assert np.all(starts[8:] > 128), starts.tolist()


@pytest.mark.parametrize("tier", TIERS, ids=IDS)
def test_ranges_run_into_the_sequence_ends(gpu, oracle, tier):
    """A short pattern in a long text and the reverse: from some score before the final one on, -pl (tl) is what sets the range's end, not
    the diamond."""
    tasks, units, r = _run(gpu, oracle, "clamps%d" % tier, tier)
    for i in range(len(tasks)):
        U, s_end = int(r["bound"][i]), int(units[i])
        binds = [_range(tasks[i], U, s)[2 + i % 2] for s in range(2, s_end + 1)]
        assert any(binds[:-1]), (i, U, s_end, binds)

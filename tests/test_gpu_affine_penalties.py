"""GPU: every chain of the exact gap-affine aligner under the penalties that select it.

otg_launch_affine picks its chain from the penalties in units of their gcd g, (xs, oes, es) = (x, o + e, e) / g:
  standard        (2, 4, 1)            score-bound pass, counting sort, register tiers, then the HBM-row tiers A and B, then the generic kernel C
  unit extension  es == 1, otherwise   tiers A (4096 diagonals) and B (12288) without a bound, then C
  generic         es != 1              kernel C alone
The rings hold rm = max(xs, oes) + 1 rows of M and ri = es + 1 rows of I and D, 64 at most; beyond that the penalties are refused.

Every case compares score, op string and (where asked) cell count with the oracle under the same penalties, and reads otg_affine_last_routing
back to assert WHICH tier finished each alignment: a chain that hands everything to the generic kernel is exact too.

The module also runs under the switches of test_gpu_alt_paths.py (OTG_NO_AFFINE_V3, OTG_AFFINE_REG=0, OTG_NO_AFFINE_BOUND, read once per
process); `_chain` restates what they leave of each class's chain, and the tier assertions follow it."""
import math
import os
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
from helpers import rand_seq, mutate, tr_seq, pair_tasks
from test_gpu_affine import _pairs
from test_gpu_affine_routing import _ends_free

pytestmark = pytest.mark.gpu

FIN_A, FIN_B, FIN_C, NONE = abi.AFFINE_FIN_A, abi.AFFINE_FIN_B, abi.AFFINE_FIN_C, abi.AFFINE_TIER_NONE
NO_BOUND = 0x40000000                      # the bound pass leaves INT_MAX where it finds no alignment (an empty sequence, a wide start range)


def _reduced(x, o, e):
    g = math.gcd(math.gcd(x, o + e), e)
    return g, x // g, (o + e) // g, e // g


def _chain(x, o, e):
    """(HBM-row tiers run, bound pass runs, register tiers may run) for these penalties in this process: wfa_affine.hip's choice, restated."""
    g, xs, oes, es = _reduced(x, o, e)
    hbm = es == 1 and "OTG_NO_AFFINE_V3" not in os.environ
    bounded = hbm and (xs, oes) == (2, 4) and "OTG_NO_AFFINE_BOUND" not in os.environ
    return hbm, bounded, bounded and (int(os.environ.get("OTG_AFFINE_REG", "31")) & 31) != 0


def _run(gpu, oracle, arena, tasks, pen):
    """One batch under penalties `pen` against the oracle (score, op string, cells) -> (oracle's result, routing)."""
    es, ec, ecells = oracle.affine_align_batch(arena, tasks, *pen, want_cells=True)
    gs, gc, gcells = gpu.affine_align_batch(arena, tasks, *pen, want_cells=True)
    r = gpu.affine_last_routing(len(tasks))
    print("%s: finished %s (index: 0-4 register tiers, 5 = A, 6 = B, 7 = C), mask %d" % (pen, np.bincount(np.maximum(r["finished"], 0), minlength=8).tolist(), r["mask"]))
    assert np.array_equal(gs, es), (pen, [(int(i), int(gs[i]), int(es[i]), int(tasks[i]["pattern_len"]), int(tasks[i]["text_len"])) for i in np.flatnonzero(gs != es)[:8]])
    bad = [(i, int(tasks[i]["pattern_len"]), int(tasks[i]["text_len"])) for i in range(len(tasks)) if gc[i] != ec[i]]
    assert not bad, (pen, bad[:8])
    assert np.array_equal(gcells, ecells), (pen, np.flatnonzero(gcells != ecells)[:8].tolist())
    assert np.all(r["finished"] >= 0), (pen, r["finished"].tolist())          # nobody is lost, and the generic kernel gives nothing up
    return (es, ec, ecells), r


def _check_class(pen, r):
    """What the routing readback must say for the class of `pen`, whatever the batch."""
    hbm, bounded, reg = _chain(*pen)
    fin, routed = r["finished"], r["routed"]
    if not hbm:                           # the generic kernel alone: no HBM-row tier ran, nothing was sorted or bounded
        assert r["mask"] == 0 and np.all(fin == FIN_C) and np.all(routed == NONE), (pen, fin.tolist())
        assert len(r["tier_a_gave_up"]) == 0 and len(r["tier_b_gave_up"]) == 0 and len(r["tier_a_input"]) == 0 and len(r["sorted"]) == 0, pen
        assert np.all(r["bound"] == -1), pen
        return
    if not bounded:                       # tiers A and B without a bound, then C
        assert r["mask"] == 0 and np.all(routed == NONE) and np.all(r["bound"] == -1), pen
        assert np.all((fin == FIN_A) | (fin == FIN_B) | (fin == FIN_C)), (pen, fin.tolist())
        return
    assert np.all(r["bound"] >= 0), pen
    assert (r["mask"] != 0) == reg, (pen, r["mask"])


def _ont_pairs(rng, n, lmin, lmax):
    pairs = []
    for i in range(n):
        L = int(rng.integers(lmin, lmax))
        a = mutate(rng, tr_seq(rng, L) if i % 2 else rand_seq(rng, L), 0.07)
        pairs.append((a, mutate(rng, a, 0.07 if i % 3 else 0.15)))
    return pairs


_cache = {}


def _mixed_batch():
    """_pairs(rng, 300, 260) of test_gpu_affine.py (0 - 260 bases, every divergence, unrelated pairs, the ends-free forms) and 30 ONT-like
    pairs of 1 - 3 kb."""
    if "mixed" not in _cache:
        rng = np.random.default_rng(6100)
        pairs, forms = _pairs(rng, 300, 260)
        long_pairs = _ont_pairs(rng, 30, 1000, 3000)
        _cache["mixed"] = pair_tasks(pairs + long_pairs, forms + [None] * len(long_pairs))
    return _cache["mixed"]


# ---- the standard class under every gcd
STANDARD = [(2, 3, 1), (4, 6, 2), (6, 9, 3), (8, 12, 4)]


def test_standard_class_every_gcd(gpu, oracle):
    """(2,3,1), (4,6,2), (6,9,3), (8,12,4) all reduce to (2,4,1) with g = 1, 2, 3, 4: one cost model up to scale.  Each equals the oracle;
    the op strings are the same for all four and score == units * g; the bound pass and the register tiers run; a register tier finishes
    what it admits; bound * g >= the oracle's score."""
    arena, tasks = _mixed_batch()
    units = cigs = None
    for pen in STANDARD:
        g = _reduced(*pen)[0]
        assert _reduced(*pen)[1:] == (2, 4, 1)
        (es, ec, _), r = _run(gpu, oracle, arena, tasks, pen)
        if units is None:
            units, cigs = es.astype(np.int64), ec
            assert g == 1
        assert np.array_equal(es, units * g), pen                      # on the oracle: the four sets are one cost model
        assert ec == cigs, pen
        _check_class(pen, r)
        hbm, bounded, reg = _chain(*pen)
        if bounded:
            has = r["bound"] < NO_BOUND
            assert np.count_nonzero(has) >= 0.9 * len(tasks), pen
            low = np.flatnonzero(has & (r["bound"].astype(np.int64) * g < es))
            assert len(low) == 0, (pen, [(int(i), int(r["bound"][i]), int(es[i])) for i in low[:8]])
        if reg:
            took = r["routed"] < NONE
            assert np.count_nonzero(took) >= 0.9 * len(tasks), (pen, np.bincount(r["routed"], minlength=6).tolist())
            gave_up = np.flatnonzero(took & (r["finished"] != r["routed"]))
            assert len(gave_up) == 0, (pen, [(int(i), int(r["routed"][i]), int(r["finished"][i])) for i in gave_up[:8]])
            assert not np.any(r["finished"] == FIN_C), pen


# ---- the unit-extension class: which of A, B, C finishes
# Without a bound the wavefront of score s spans about 2 (s - oes) + 1 diagonals, clipped to pattern + text + 1.  Tier A's window holds
# 4096 - 140 of them and tier B's 12288 - 140, so an end-to-end pair leaves tier A when pattern + text exceeds 3956 AND its score exceeds
# about 1980 + oes; it leaves tier B the same way beyond 12148 diagonals, or sooner when the provenance bytes of its wavefronts (the sum of
# their widths, about s^2 up to the clip) outgrow tier B's slab (0.2 x maxlen^2 = 13.4 MB for a batch whose longest sequence is 4 - 8 kb).
# Unrelated random pairs score about 1.55 per base under (3,5,1) and 0.52 per base under (1,0,1) (measured on the oracle).
UNIT_EXT_LENGTHS = {
    (3, 5, 1): {FIN_A: (1850, 1900), FIN_B: (2200, 2300), FIN_C: (6300,)},
    (1, 0, 1): {FIN_A: (1900, 3000), FIN_B: (4200, 4400), FIN_C: (7500,)},
}


def _unit_ext_batch(pen):
    if pen not in _cache:
        rng = np.random.default_rng(6200 + pen[0])
        pairs, forms, want = [], [], []
        for fin, lengths in UNIT_EXT_LENGTHS[pen].items():
            for L in lengths:
                pairs.append((rand_seq(rng, L), rand_seq(rng, L + int(rng.integers(-40, 41))))); forms.append(None); want.append(fin)
        # a free begin of a few hundred bases (the forms of _ends_free): score 0 has that many start diagonals, and `hi - lo + 140 > CAP` is
        # the only guard on the start range; then start ranges on both sides of tier A's two tests on them (a free begin of `cut` bases is
        # cut + 1 start diagonals: beyond 3956 the guard refuses them, from 3833 on the centred window has no room for score 0's probes
        # and the window test hands the pair on) and an unrelated pair behind a free begin
        for i, kind in enumerate((0, 1, 2, 4)):
            p = rand_seq(rng, 900 + 60 * i)
            pr, f = _ends_free(rng, p, mutate(rng, p, 0.1), kind, 300 + 130 * i)
            pairs.append(pr); forms.append(f); want.append(None)
        for cut in (3000, 3832, 3833, 3956, 3957):
            p = rand_seq(rng, 500)
            pr, f = _ends_free(rng, p, mutate(rng, p, 0.08), 0, cut)
            pairs.append(pr); forms.append(f); want.append(None)
        pr, f = _ends_free(rng, rand_seq(rng, 700), rand_seq(rng, 650), 4, 400)
        pairs.append(pr); forms.append(f); want.append(None)
        # bytes outside ACGT: the HBM-row tiers compare bytes, N == N and case matters
        a = bytearray(rand_seq(rng, 1200)); b = bytearray(mutate(rng, bytes(a), 0.1))
        for s_ in (a, b):
            for _ in range(6):
                s_[int(rng.integers(0, len(s_)))] = b"NnacgtRY"[int(rng.integers(0, 8))]
        pairs.append((bytes(a), bytes(b))); forms.append(None); want.append(None)
        _cache[pen] = pair_tasks(pairs, forms) + (want,)
    return _cache[pen]


@pytest.mark.parametrize("pen", sorted(UNIT_EXT_LENGTHS), ids=lambda p: "%d-%d-%d" % p)
def test_unit_extension_tiers_a_b_c(gpu, oracle, pen):
    """Unrelated random pairs on both sides of tier A's and tier B's limits, in one batch (the longest sequence sizes the tiers' slabs).
    Lengths settled on (pattern; the text is within 40 bases of it), by the tier that finishes them:
        (3,5,1): A 1850, 1900;  B 2200, 2300;  C 6300
        (1,0,1): A 1900, 3000;  B 4200, 4400;  C 7500
    Every pair is finished by the tier named, so each of A, B and C occurs; everything equals the oracle."""
    arena, tasks, want = _unit_ext_batch(pen)
    _, r = _run(gpu, oracle, arena, tasks, pen)
    _check_class(pen, r)
    hbm, bounded, reg = _chain(*pen)
    assert not bounded
    fin = r["finished"]
    if hbm:
        got = [(int(tasks[i]["pattern_len"]), int(fin[i])) for i in range(len(tasks)) if want[i] is not None]
        assert all(fin[i] == want[i] for i in range(len(tasks)) if want[i] is not None), (pen, got)
        for tier in (FIN_A, FIN_B, FIN_C):
            assert np.any(fin == tier), (pen, tier, got)


# ---- the generic class
GENERIC = [(6, 2, 3), (5, 3, 2), (1, 0, 63)]


@pytest.mark.parametrize("pen", GENERIC, ids=lambda p: "%d-%d-%d" % p)
def test_generic_class(gpu, oracle, pen):
    """es != 1: x > o + e, an even extension, and ri = es + 1 = 64 rows of I and D.  Kernel C alone, on the 0 - 260 base batch and 1 - 3 kb pairs."""
    assert _reduced(*pen)[3] != 1
    arena, tasks = _mixed_batch()
    _, r = _run(gpu, oracle, arena, tasks, pen)
    _check_class(pen, r)
    assert np.all(r["finished"] == FIN_C) and len(r["tier_a_input"]) == 0


# ---- the ring limits
# (63,0,1), (1,62,1) and (126,0,2) (the same as the first after the gcd) are the corners of what affine_penalties admits.  Under (63,0,1) an
# insertion plus a deletion costs 2 and a mismatch 63, so no alignment ever reads the row 63 scores back; (63,40,1) and (40,62,1) keep rm = 64
# and make both the mismatch row and the gap-open row of the ring matter (the oracle's op strings hold X as well as I and D).
RING = [(63, 0, 1), (1, 62, 1), (126, 0, 2), (63, 40, 1), (40, 62, 1)]


def _ring_batch():
    if "ring" not in _cache:
        rng = np.random.default_rng(6300)
        pairs = []
        for i in range(36):
            L = int(rng.integers(200, 1500))
            a = tr_seq(rng, L) if i % 4 == 3 else rand_seq(rng, L)
            pairs.append((a, mutate(rng, a, [0.02, 0.05, 0.1, 0.15][i % 4])))
        pairs += [(rand_seq(rng, L), rand_seq(rng, L - 17)) for L in (90, 300, 700)]
        _cache["ring"] = pair_tasks(pairs)
    return _cache["ring"]


@pytest.mark.parametrize("pen", RING, ids=lambda p: "%d-%d-%d" % p)
def test_ring_of_64_rows(gpu, oracle, pen):
    """rm = max(xs, oes) + 1 = 64, the most affine_penalties admits: tiers A / B index s_mlo[64] by s % rm and keep the ring plus the null row.
    Mutated pairs of 200 - 1500 bases at 2 - 15 % and a few unrelated ones.  On the oracle: more than half of the scores pass rm and a
    quarter pass it twice (under (63,0,1), whose scores are the smallest: 21 and 10 of 39), so the ring wraps.  Under the two sets with large
    scores the widest pairs outgrow the slabs of tiers A and B (3.4 MB for sequences below 4 kb) and end in the generic kernel: 6 and 7 of 39
    by the sum of their wavefront widths."""
    g, xs, oes, es = _reduced(*pen)
    assert max(xs, oes) + 1 == 64 and es == 1
    arena, tasks = _ring_batch()
    (scores, _, _), r = _run(gpu, oracle, arena, tasks, pen)
    assert np.count_nonzero(scores >= 64 * g) > len(tasks) // 2 and np.count_nonzero(scores >= 2 * 64 * g) >= len(tasks) // 4, sorted(scores.tolist())
    _check_class(pen, r)
    if _chain(*pen)[0]:
        assert np.count_nonzero(r["finished"] == FIN_A) > len(tasks) // 2, r["finished"].tolist()
        if max(xs, oes) - min(xs, oes) >= 62:
            assert np.all(r["finished"] == FIN_A), r["finished"].tolist()     # small scores: no wavefront here outgrows tier A


def test_penalties_refused(gpu, oracle):
    """Beyond the rings, or not a cost model: OTG_ERR_ARG, and no launch is accounted for on the context."""
    arena, tasks = _ring_batch()
    n = len(tasks)
    for pen in [(64, 0, 1), (1, 63, 1), (1, 0, 64), (0, 1, 1), (1, 1, 0), (1, -1, 1)]:
        gpu.affine_align_batch(arena, tasks[:3])
        assert gpu.affine_last_routing(3)["finished"].shape == (3,)
        with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\).*affine penalties"):
            gpu.affine_align_batch(arena, tasks, *pen)
        with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\)"):
            gpu.affine_last_routing(n)
        with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\)"):
            gpu.affine_last_routing(3)
    # and the largest that are admitted, once more behind the refusals
    _run(gpu, oracle, arena, tasks[:6], (63, 0, 1))

"""GPU: the three states of a register tier's match-run queue — empty, in use, overflowed — each with a witness.

A score of `wfa_affine_reg_kernel` decides from the queue's length alone what follows its sweep: nothing (0), the drain and the fold-back of
the patch table (in use), or giving the alignment up to the next tier (the marker QFULL, set by the first push that finds no room:
`qn + 128 > QCAP`, QCAP = 512).  Every batch is compared with the oracle on score, op string and cells, and `Context.affine_last_routing`
says which tier finished each alignment.

  (a) runs: near-identical pairs made of exact runs of 65 to 130 bases between single edits.  Behind every edit the leading cell's run outlives
      both probes of its slot visit (64 bases), so queue, drain and fold-back run in most reachable scores.  Finished by the routed tier.
  (b) overflow: the begin-free constructions of test_gpu_affine_routing.py (`_insertion_pair`, `_ends_free`, its forms 0, 1, 2 and 4) with
      the free stretch a homopolymer of CUT = 640 bases, and 80 bases of the same letter in front of core and insertion.  At score 0 every
      start diagonal inside the stretch has a match run of 80 bases or more: 641 cells of ONE score that outlive the 64 bases of the two
      probes.  A slot visit pushes at most 128 and a push is refused once the queue holds more than 384, so the tier gives the alignment
      up however the cells fall onto the slots (before the last pushing slot the queue holds at least 641 - 128).  Routed to a register
      tier, finished by tier A.
  (c) both kinds interleaved in one batch.  One-wave tiers run four alignments per block, one per wave, and a wave takes the next ticket
      as soon as it is done: one that gave up at score 0 is back for another alignment long before the others have finished theirs.
      Which wave takes which alignment is the device's decision (the chain launches a full grid whatever the batch); the batch is
      ordered so that an overflowing pair precedes every other one.
Batches (a), (b), (c) are built for the 1024 window (one wave, sequences up to 1 500 bases); (c) also for the 2048 window (two waves
share an alignment) and the 4096 window (four).  Those two cannot be reached with 1 500 bases — an end-to-end pair wants about U + 8
diagonals, the bound across an insertion of G bases is 2 G - 51, and the bound pass gives up beyond pattern + text + 64 scores, so the
4096 window wants G above 1 046 and below 2 L + 115 behind a core of L bases, L + G above 1 500 — and their waves have a queue each: the stretch grows to 1 400 and 2 600 bases (STRETCH below),
on a core of 900 bases as in the routing test.  Their windows stay below 3 200 diagonals, which tier A behind them can finish.
The inputs were established on the parent of the change that derived both flags from the queue length: there, as here, all 8, 8, 4 and 4
overflowing pairs of the four batches that have them were routed to the window's tier and finished by tier A, every other pair by its tier."""
import numpy as np
import pytest
from helpers import rand_seq, pair_tasks
from test_gpu_affine_routing import CUT, PEN, _insertion_pair, _ends_free, _expected_tiers, _check_chain, _report

pytestmark = pytest.mark.gpu

HOMO = 80            # the letter of the stretch in front of the other sequence: a run of 80 > 64 on every start diagonal that is deep enough in the stretch
RUNS = (65, 72, 90, 101, 130, 66, 85, 118, 70, 97, 125, 68, 110)      # 1 197 bases and 12 edits: below 1 500


def _runs_pair(rng, rep):
    """exact runs beyond 64 bases between single edits (a mismatch, an insertion of 1 to 3 bases on either side)"""
    a, b = bytearray(), bytearray()
    for j, r in enumerate(np.roll(RUNS, rep)):
        run = rand_seq(rng, int(r))
        a += run; b += run
        kind = (j + rep) % 3
        if kind == 0:
            a += b"A"; b += b"C"
        elif kind == 1:
            a += rand_seq(rng, 1 + j % 3)
        else:
            b += rand_seq(rng, 1 + j % 2)
    return (bytes(a), bytes(b)) if rep % 2 else (bytes(b), bytes(a))


def _overflow_pair(rng, tier, G, kind):
    """test_gpu_affine_routing's begin-free pair (form `kind`: 0, 1, 4 free the pattern's begin, 2 the text's) in the layout that keeps the
    whole start range — the insertion in the sequence whose begin is NOT free — with the free stretch a homopolymer of STRETCH[tier] bases,
    core and insertion both beginning with HOMO bases of its letter"""
    core = b"A" * HOMO + rand_seq(rng, CORE[tier] - HOMO)
    ins = b"A" * HOMO + rand_seq(rng, G - HOMO)
    p, t = _insertion_pair(core, ins, 0, kind == 2)
    (p, t), form = _ends_free(rng, p, t, kind, STRETCH[tier])
    if kind == 2:
        t = b"A" * STRETCH[tier] + t[STRETCH[tier]:]
    else:
        p = b"A" * STRETCH[tier] + p[STRETCH[tier]:]
    return (p, t), form


def _window_runs_pair(rng, tier, G, rep):
    """a runs pair whose window is selected by one insertion of G bases behind it (end to end)"""
    a, b = _runs_pair(rng, rep)
    return (a, b + rand_seq(rng, G)) if rep % 2 else (b + rand_seq(rng, G), a)


# Waves that share an alignment own its pair-slots in turn and each has a queue of its own, so a score must push more than 384 from the
# slots of ONE wave: the stretch grows with the waves.  A wave's share of D pushing cells in consecutive slots is at least (D - 254) / NW
# (the first and the last slot may be partly covered); before its last push of 128 it holds
#   one wave,  D = 641:   641 - 128 = 513 > 384
#   two waves, D = 1401:  (1401 - 254) / 2 - 128 = 445 > 384
#   four,      D = 2601:  (2601 - 254) / 4 - 128 = 458 > 384
STRETCH = {0: CUT, 2: 1400, 3: 2600}
CORE = {0: 820, 2: 900, 3: 900}              # the 1024 window's sequences stay within 1 500 bases: 640 + 820
# per window: (insertion lengths of the overflow pairs, their forms, insertion lengths of the runs pairs of the multi-wave windows)
OVER = {0: ((300, 330, 360, 390, 420, 330, 360, 390), (0, 1, 2, 4, 0, 1, 2, 4), None),
        2: ((880, 900, 920, 940), (0, 2, 0, 2), (900, 920, 940, 960)),
        3: ((1100, 1150, 1200, 1250), (0, 2, 4, 0), (1350, 1400, 1450, 1500))}

_cache = {}


def _batch(name, oracle):
    if name not in _cache:
        kind, tier = name.split(":")
        tier = int(tier)
        rng = np.random.default_rng(5100 + 10 * tier + len(kind))
        gs, forms_k, g_runs = OVER[tier]
        over = [_overflow_pair(rng, tier, G, k) for G, k in zip(gs, forms_k)]
        if g_runs is None:
            runs = [(_runs_pair(rng, rep), None) for rep in range(8)]
        else:
            runs = [(_window_runs_pair(rng, tier, G, rep), None) for rep, G in enumerate(g_runs)]
        if kind == "runs":
            items, is_over = runs, [False] * len(runs)
        elif kind == "overflow":
            items, is_over = over, [True] * len(over)
        else:
            items, is_over = [], []
            for o, r in zip(over, runs):
                items += [o, r]; is_over += [True, False]
        arena, tasks = pair_tasks([x[0] for x in items], [x[1] for x in items])
        _cache[name] = (arena, tasks, np.array(is_over), oracle.affine_align_batch(arena, tasks, *PEN, want_cells=True))
    return _cache[name]


def _run(gpu, oracle, name):
    arena, tasks, is_over, (es, ec, ecells) = _batch(name, oracle)
    assert len(tasks) <= 32
    gs, gc, gcells = gpu.affine_align_batch(arena, tasks, *PEN, want_cells=True)
    r = gpu.affine_last_routing(len(tasks))
    _report(name, tasks, r)
    assert np.array_equal(gs, es), (name, [(int(i), int(gs[i]), int(es[i])) for i in np.flatnonzero(gs != es)[:8]])
    bad = [i for i in range(len(tasks)) if gc[i] != ec[i]]
    assert not bad, (name, bad[:10])
    assert np.array_equal(gcells, ecells), name
    _check_chain(name, tasks, es, r)
    return tasks, is_over, r


def _check_exits(name, tier, tasks, is_over, r):
    if not r["mask"]:          # OTG_AFFINE_REG=0: no register tier runs, nothing to say about its queue
        return
    exp = _expected_tiers(tasks, r, mask=31)
    routed, finished = r["routed"], r["finished"]
    # conditions on the inputs: every pair is the window's
    assert np.all(exp == tier), (name, exp.tolist())
    if (r["mask"] >> tier) & 1:
        normal = ~is_over
        assert np.all(finished[normal] == routed[normal]), (name, "a pair with a working queue was given up", finished.tolist())
        if np.any(is_over):
            assert np.all(routed[is_over] == tier), (name, routed.tolist())
            assert np.count_nonzero(finished[is_over] == 5) >= 4, (name, "overflowed pairs that took the tier-A exit", finished[is_over].tolist())
            assert np.all(finished[is_over] == 5), (name, finished[is_over].tolist())


def test_queue_in_use_every_score(gpu, oracle):
    """(a): eight pairs of the 1024 window whose queue, drain and fold-back run in most scores; finished by the tier they were routed to."""
    tasks, is_over, r = _run(gpu, oracle, "runs:0")
    assert max(int(tasks["pattern_len"].max()), int(tasks["text_len"].max())) <= 1500
    _check_exits("runs:0", 0, tasks, is_over, r)


def test_queue_overflow_goes_to_tier_a(gpu, oracle):
    """(b): eight begin-free pairs whose score 0 pushes more than the queue holds: routed to the 1024 window, given up there, finished by tier A."""
    tasks, is_over, r = _run(gpu, oracle, "overflow:0")
    assert max(int(tasks["pattern_len"].max()), int(tasks["text_len"].max())) <= 1500
    _check_exits("overflow:0", 0, tasks, is_over, r)


@pytest.mark.parametrize("tier", [0, 2, 3], ids=["one-wave-1024", "two-wave-2048", "four-wave-4096"])
def test_queue_exits_interleaved(gpu, oracle, tier):
    """(c): overflowing and normal pairs alternate in one batch: the normal ones finish in their tier, the others in tier A, whichever wave took them."""
    name = "mixed:%d" % tier
    tasks, is_over, r = _run(gpu, oracle, name)
    _check_exits(name, tier, tasks, is_over, r)

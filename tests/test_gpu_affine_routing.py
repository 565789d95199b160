"""GPU: which tier of the exact gap-affine chain finishes each alignment, not only the result.

The chain (score-bound pass, counting sort, five register tiers, HBM-row tiers A and B, the generic kernel C) hands an alignment a tier cannot
finish to the next one, so a register tier that gives up on what it was built for, a sort that admits what the kernel then refuses, or a bound
that is too low all leave score and op string exact — a later tier does the work.  otg_affine_last_routing reads the
chain's counters and lists back after a launch; these tests compare every batch with the oracle (score, op string, cells) AND assert
  1. partition: every task has one finisher, no list holds a task twice, the sort's output is a permutation, the segments add up,
     finished >= routed in chain order;
  2. routing: the tier the sort assigned equals affine_window / reg_tier restated below in plain integers;
  3. the score bound is a bound: U * g >= the oracle's score (g = the gcd of the penalties: 2 for 4,6,2; one window also runs 2,3,1 and 6,9,3);
  4. a register tier finishes what it admits: finished == routed, exactly;
  5. a pair with bytes outside ACGT is routed to its register tier, given up by it (the pack check) and finished by tier A;
  6. nothing reaches the generic kernel.

Inputs: a random core and ONE random insertion of G bases.  The bound pass follows the alignment with a band of 64 diagonals that moves one
diagonal every second score, so across a long gap its bound is about 2 G (an insertion behind the core: 2 G - 50 measured), not the optimum
G + 3, and no bound exists beyond pattern + text + 64 scores.  The G of each batch is chosen for that bound; the per-tier minimum asserted
below is a condition on these inputs (a tighter bound pass moves the G, not the minimum).

The ends-free pairs of every window have a free begin of 640 bases and more: score 0 then has more start diagonals than a register tier's
match-run queue holds (QCAP entries, and a push needs room for two per lane).  The tiers once pushed every start diagonal through that
queue and handed such alignments to tier A; a tier that did so again would fail invariant 4 in every window."""
import math
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
from helpers import rand_seq, mutate, pair_tasks

pytestmark = pytest.mark.gpu

# ---- the admission rule, restated from wfa_affine_common.hpp (affine_window) and wfa_affine.hip (reg_tier); not imported from the library
CAP = (1024, 1536, 2048, 4096, 8192)        # diagonals of window per register tier
SEQB = (4096, 4608, 6144, 8192, 12288)      # bytes of 2-bit packed sequence pair per register tier
NONE = 5                                     # routed: no register tier; finished: 5 = A, 6 = B, 7 = C
PEN = (4, 6, 2)                              # the default penalties; (2,3,1) and (6,9,3) reduce to the same (2,4,1) with another gcd


def gcd_unit(pen):
    """g of wfa_affine_common.hpp (affine_penalties): the gcd of mismatch, gap open + extension and gap extension."""
    x, o, e = pen
    return math.gcd(math.gcd(x, o + e), e)


QCAP, QPUSH = 384, 128                       # entries of a register tier's match-run queue; room one push asks for (`qn + 128 > QCAP`)


def affine_window(t, U):
    """(start diagonals of score 0, diagonals of window wanted) for task t under the bound U."""
    pl, tl, ef = int(t["pattern_len"]), int(t["text_len"]), int(t["endsfree"]) != 0
    kend = tl - pl
    elo = kend - (int(t["text_end_free"]) if ef else 0)
    ehi = kend + (int(t["pattern_end_free"]) if ef else 0)
    lo0 = max(-int(t["pattern_begin_free"]), -pl) if ef else 0
    hi0 = min(int(t["text_begin_free"]), tl) if ef else 0
    lo0, hi0 = max(lo0, elo - U), min(hi0, ehi + U)
    wlo = max((lo0 + elo - U) >> 1, -pl) - 1
    whi = min((hi0 + ehi + U + 1) >> 1, tl) + 1
    return max(hi0 - lo0 + 1, 0), whi - (wlo - 2) + 4


def seq_bytes(t):
    return ((int(t["pattern_len"]) + 15) // 16 + 3 + (int(t["text_len"]) + 15) // 16 + 3) * 4


def reg_tier(t, U, mask):
    if U < 0 or U >= 0x40000000 or int(t["pattern_len"]) >= 32766 or int(t["text_len"]) >= 32766:
        return NONE
    starts, need = affine_window(t, U)
    if not starts:
        return NONE
    for tier in range(5):
        if (mask >> tier) & 1 and need < CAP[tier] and seq_bytes(t) <= SEQB[tier]:
            return tier
    return NONE


# ---- batches (built once per process; the oracle's result is shared and never modified)
_cache = {}


def _batch(name, oracle, pen=PEN):
    if name not in _cache:
        pairs, forms = BUILDERS[name]()
        _cache[name] = pair_tasks(pairs, forms)
    if (name, pen) not in _cache:
        arena, tasks = _cache[name]
        _cache[(name, pen)] = (arena, tasks, oracle.affine_align_batch(arena, tasks, *pen, want_cells=True))
    return _cache[(name, pen)]


def _insertion_pair(core, ins, pos, flip):
    a = core[:pos] + ins + core[pos:]
    return (a, core) if flip else (core, a)


def _ends_free(rng, p, t, kind, cut):
    """The ends-free forms of test_affine_wide_free_begin around an end-to-end pair (p, t): a free stretch of `cut` random bases in front of
    the pattern (exactly / with slack), in front of the text, behind the pattern, and both begins free."""
    junk = rand_seq(rng, cut)
    if kind == 0: return (junk + p, t), (cut, 0, 0, 0)
    if kind == 1: return (junk + p, t), (cut + 150, 0, 0, 0)
    if kind == 2: return (p, junk + t), (0, 0, cut + 40, 0)
    if kind == 3: return (p + junk, t), (0, cut + 25, 0, 0)
    return (junk + p, t), (cut + 60, 0, 30, 0)


# per register window: core length, insertion lengths of the end-to-end pairs (the insertion lies behind the core), gap lengths of the
# begin-free pairs, and which sequence of those carries the insertion.  The 8192 window takes a longer core: the tier only runs when a
# sequence is longer than 4096, and the bound pass gives up beyond pattern + text + 64 scores, which a 900-base core reaches before its
# bound fills half of that window.
#   The begin-free pairs have a free stretch of CUT random bases (plus the forms' slack) in front of one sequence and the insertion in
# front of the core.  Only start diagonals within U of the end diagonals are kept, and half of the start range counts towards the wanted
# window, so two layouts are needed:
#   - insertion in the sequence whose begin is free, lengthened by the form's slack (which may be skipped for free): the gap must be opened,
#     U = 2 G - 51 as for the end-to-end pairs, about G - 50 start diagonals up to the whole range.  More than QCAP + QPUSH of them need
#     G > 560, which wants about 1 400 diagonals: the 2048 window and up.
#   - insertion in the other sequence: it can also be aligned against the end of the free stretch, the pass finds a bound of 1.1 to 1.4 G
#     (measured; it varies from pair to pair) and the whole start range stays.  This is what fits the 1024 and 1536 windows.
CUT = 640
FREE_KINDS = (0, 1, 2, 4, 0, 1, 2, 4, 0, 2)       # the begin-free forms of _ends_free
SLACK = {0: 0, 1: 150, 2: 40, 4: 60}              # what each of them leaves free beyond the stretch itself
WINDOW = {
    0: (900, range(200, 300, 10), range(300, 450, 15), False),
    1: (900, range(620, 720, 10), range(700, 790, 9), False),
    2: (900, range(880, 980, 10), range(700, 820, 12), True),
    3: (900, range(1300, 1700, 40), range(1000, 1500, 50), True),
    4: (2600, range(2700, 3200, 50), range(2400, 2900, 50), True),
}


def _build_window(tier):
    def build():
        rng = np.random.default_rng(4100 + tier)
        L, g_e2e, g_free, same_side = WINDOW[tier]
        core = rand_seq(rng, L)
        pairs, forms = [], []
        for i, G in enumerate(g_e2e):
            pairs.append(_insertion_pair(core, rand_seq(rng, G), L, i % 2)); forms.append(None)
        # (a free begin makes the bound pass run on the reversed pair: the insertion lies in front of the core here, behind it in that run)
        for G, kind in zip(g_free, FREE_KINDS):
            on_pattern = (kind != 2) == same_side          # kind 2 frees the text's begin, the others the pattern's
            p, t = _insertion_pair(core, rand_seq(rng, G + (SLACK[kind] if same_side else 0)), 0, on_pattern)
            pr, f = _ends_free(rng, p, t, kind, CUT)
            pairs.append(pr); forms.append(f)
        # the end-free form (one start diagonal; the bound pass runs forwards): a short free stretch, the insertion behind the core
        for i in (0, 5):
            pr, f = _ends_free(rng, *_insertion_pair(core, rand_seq(rng, g_e2e[i] - 40), L, i % 2), 3, 120)
            pairs.append(pr); forms.append(f)
        return pairs, forms
    return build


# window edge: the insertion grows by one base per pair (prefixes of one random string, so the bound grows steadily) across the G at which
# the wanted window reaches the tier's capacity.  The bound grows by 1, 1 and 4 over three steps of G, so `need` skips values; the pairs
# nearest to the capacity are repeated with 2, 4, 6 and 8 free bases at the pattern's end, each pair of which widens the window by one
# diagonal and leaves the bound alone, so that `need` takes every value around the capacity.
# cap: (core length, the sweep of G, which of them get the free-end forms)
EDGE = {1024: (900, range(518, 537), slice(12, 16)), 1536: (900, range(774, 793), slice(12, 16)), 2048: (900, range(1030, 1049), slice(12, 16)),
        4096: (1400, range(2054, 2073), slice(12, 16)), 8192: (2600, range(4113, 4119), slice(3, 4))}


def _build_edge(cap):
    def build():
        rng = np.random.default_rng(4200 + cap)
        L, gs, near = EDGE[cap]
        core = rand_seq(rng, L)
        ins = rand_seq(rng, max(gs) + 1)
        pairs = [(core, core + ins[:G]) for G in gs]
        forms = [None] * len(pairs)
        for G in list(gs)[near]:
            for pef in (2, 4, 6, 8):
                pairs.append((core, core + ins[:G])); forms.append((0, pef, 0, 0))
        return pairs, forms
    return build


def _build_seq_edge():
    """Near-identical pairs whose packed size is exactly SEQB[t] (admitted by tier t: their window is tiny) and SEQB[t] + 4 (the next tier)."""
    rng = np.random.default_rng(4300)
    base = rand_seq(rng, 24600)
    pairs = []
    for cap in SEQB:
        for words in (cap // 4 - 6, cap // 4 - 5):
            for la, lb in ((16 * (words // 2), 16 * (words - words // 2)), (16 * (words // 2) - 15, 16 * (words - words // 2) - 3)):
                a, b = bytearray(base[:la]), bytearray(base[:lb])
                for s_ in (a, b):
                    for _ in range(3):
                        i = int(rng.integers(0, len(s_)))
                        s_[i] = b"ACGT"[(b"ACGT".index(s_[i]) + 1) % 4]
                pairs.append((bytes(a), bytes(b)))
    return pairs, None


QUEUE_RUNS = [65, 96, 129, 257, 400]


def _build_queue(noisy_len):
    """The layout of test_affine_probe_boundaries: a noisy stretch selects the window, behind it exact runs beyond 64 bases (the queue)
    between single edits.  Ten runs per pair: far below the 384 unfinished runs of one score at which a tier hands the alignment on."""
    def build():
        rng = np.random.default_rng(4400 + noisy_len)
        pairs = []
        for rep in range(8):
            base = rand_seq(rng, noisy_len)
            a = bytearray(mutate(rng, base, 0.07)); b = bytearray(mutate(rng, base, 0.07))
            for j, ri in enumerate(list(rng.permutation(len(QUEUE_RUNS))) * 2):
                r = rand_seq(rng, QUEUE_RUNS[ri])
                a += r; b += r
                kind = (j + rep) % 3
                if kind == 0:
                    a += b"A"; b += b"C"
                elif kind == 1:
                    a += rand_seq(rng, 1 + j % 3)
                else:
                    b += rand_seq(rng, 1 + j % 2)
            pairs.append((bytes(a), bytes(b)) if rep % 2 else (bytes(b), bytes(a)))
        return pairs, None
    return build


def _build_non_acgt():
    """Sixteen pairs of the 1024 ... 4096 windows, every one with a register tier, with a few bytes outside ACGT (N, lower case).  Tier A's own window is 4096 diagonals less a margin
    of 134, so the pairs of the 4096 register window stay below 3 000 diagonals: tier A must be able to finish what it is handed."""
    rng = np.random.default_rng(4500)
    core = rand_seq(rng, 900)
    pairs, forms = [], []
    for i, G in enumerate([150, 200, 250, 300, 640, 660, 680, 700, 900, 920, 940, 960, 1200, 1250, 1300, 1350]):
        p, t = _insertion_pair(core, rand_seq(rng, G), 0 if i % 4 == 3 and i % 5 != 3 else 900, i % 2)
        if i % 4 == 3:
            (p, t), f = _ends_free(rng, p, t, i % 5, 100)
        else:
            f = None
        p, t = bytearray(p), bytearray(t)
        for s_ in ((p, t) if i % 3 == 0 else (p,) if i % 3 == 1 else (t,)):
            for _ in range(1 + i % 4):
                s_[int(rng.integers(0, len(s_)))] = b"NnacgtN"[int(rng.integers(0, 7))]
        pairs.append((bytes(p), bytes(t))); forms.append(f)
    return pairs, forms


def _build_small():
    rng = np.random.default_rng(4600)
    pairs = []
    for i in range(12):
        a = rand_seq(rng, 300 + 20 * i)
        pairs.append((a, mutate(rng, a, 0.05)))
    return pairs, None


BUILDERS = {"seq_edge": _build_seq_edge, "non_acgt": _build_non_acgt, "small": _build_small, "queue1024": _build_queue(1400), "queue4096": _build_queue(8000)}
BUILDERS.update({"window%d" % t: _build_window(t) for t in range(5)})
BUILDERS.update({"edge%d" % c: _build_edge(c) for c in EDGE})


# ---- the checks
def _align(ctx, oracle, name, pen=PEN):
    """Runs batch `name` on ctx under penalties `pen`, compares it with the oracle (score, op string, cells) and returns (tasks, oracle scores, routing)."""
    arena, tasks, (es, ec, ecells) = _batch(name, oracle, pen)
    gs, gc, gcells = ctx.affine_align_batch(arena, tasks, *pen, want_cells=True)
    r = ctx.affine_last_routing(len(tasks))
    assert np.array_equal(gs, es), (name, [(int(i), int(gs[i]), int(es[i])) for i in np.flatnonzero(gs != es)[:8]])
    bad = [i for i in range(len(tasks)) if gc[i] != ec[i]]
    assert not bad, (name, bad[:10])
    assert np.array_equal(gcells, ecells), name
    return tasks, es, r


def _expected_tiers(tasks, r, mask=None):
    return np.array([reg_tier(tasks[i], int(r["bound"][i]), r["mask"] if mask is None else mask) for i in range(len(tasks))], dtype=np.int8)


def _report(name, tasks, r):
    win = [affine_window(tasks[i], int(r["bound"][i])) if 0 <= r["bound"][i] < 0x40000000 else (-1, -1) for i in range(len(tasks))]
    print("%s: mask %d, routed %s, finished %s" % (name, r["mask"], np.bincount(r["routed"], minlength=6).tolist(), np.bincount(np.maximum(r["finished"], 0), minlength=8).tolist()))
    print("  bound %s" % r["bound"].tolist())
    print("  need %s" % [w[1] for w in win])
    print("  starts %s" % [w[0] for w in win])
    print("  routed %s" % r["routed"].tolist())
    print("  finished %s" % r["finished"].tolist())


def _check_chain(name, tasks, es, r, pen=PEN):
    """Invariants 1, 2, 3 and 6."""
    g_unit = gcd_unit(pen)
    _report(name, tasks, r)
    n = len(tasks)
    routed, finished, seg, mask = r["routed"], r["finished"], r["seg"], r["mask"]
    a_in, a_out, b_out = r["tier_a_input"], r["tier_a_gave_up"], r["tier_b_gave_up"]
    everyone = np.arange(n, dtype=np.uint32)
    # 1. partition
    if mask:
        assert np.array_equal(np.sort(r["sorted"]), everyone), name
        assert seg[0] == 0 and seg[6] == n and np.all(np.diff(seg) >= 0), (name, seg)
        rest = r["sorted"][seg[5]:seg[6]]
        assert np.array_equal(a_in[:len(rest)], rest), name
        handed_on = a_in[len(rest):]
        assert len(np.unique(a_in)) == len(a_in), name
        assert np.all(routed[handed_on] < NONE), name
        for t in range(6):
            assert np.all(routed[r["sorted"][seg[t]:seg[t + 1]]] == t), (name, t)
    else:
        assert len(r["sorted"]) == 0 and len(a_in) == 0 and not np.any(seg), name
        handed_on = np.zeros(0, dtype=np.uint32)
        a_in = everyone
    assert len(np.unique(a_out)) == len(a_out) and np.all(np.isin(a_out, a_in)), name
    assert len(np.unique(b_out)) == len(b_out) and np.all(np.isin(b_out, a_out)), name
    fin = routed.copy()                          # the finisher, derived from the lists alone
    fin[handed_on] = 5
    fin[a_out] = 6
    fin[b_out] = 7
    assert np.array_equal(fin, finished), (name, np.flatnonzero(fin != finished)[:8])
    assert np.all((finished >= routed) & (finished <= 7)), name
    # 2. the sort's routing is the restated rule
    exp = _expected_tiers(tasks, r)
    assert np.array_equal(routed, exp), (name, [(int(i), int(routed[i]), int(exp[i]), int(r["bound"][i])) for i in np.flatnonzero(routed != exp)[:8]])
    # 3. the bound is a bound (in units of g)
    assert np.all(r["bound"] >= 0), name
    assert np.all(r["bound"].astype(np.int64) * g_unit >= es), (name, [(int(i), int(r["bound"][i]), int(es[i])) for i in np.flatnonzero(r["bound"].astype(np.int64) * g_unit < es)[:8]])
    # 6. nothing reaches the generic kernel
    assert not np.any(finished == 7), (name, np.flatnonzero(finished == 7)[:8])
    if not mask:                                 # the control: without register tiers the accessor reports what ran, not what was planned
        assert np.all(routed == NONE) and np.all((finished == 5) | (finished == 6)), name


def _check_finishes(name, r):
    """Invariant 4: exact, for every task the sort gave a register tier (what it gave none runs on tier A, or on tier B beyond A's window).
    Without register tiers (OTG_AFFINE_REG=0) there is nothing to assert."""
    if not r["mask"]:
        return
    gave_up = np.flatnonzero((r["routed"] < NONE) & (r["finished"] != r["routed"]))
    assert len(gave_up) == 0, (name, [(int(i), int(r["routed"][i]), int(r["finished"][i]), int(r["bound"][i])) for i in gave_up[:12]])


def _routing_per_window(gpu, oracle, tier, pen):
    name = "window%d" % tier
    tasks, es, r = _align(gpu, oracle, name, pen)
    _check_chain(name, tasks, es, r, pen)
    mine = _expected_tiers(tasks, r, mask=31) == tier
    ef = tasks["endsfree"] != 0
    assert np.count_nonzero(mine & ~ef) >= 8 and np.count_nonzero(mine & ef) >= 8, (name, np.count_nonzero(mine & ~ef), np.count_nonzero(mine & ef))
    begin_free = (tasks["pattern_begin_free"] > 0) | (tasks["text_begin_free"] > 0)
    starts = np.array([affine_window(tasks[i], int(r["bound"][i]))[0] for i in range(len(tasks))])
    wide = mine & ef & begin_free & (starts > QCAP + QPUSH)
    assert np.count_nonzero(wide) >= 8, (name, starts[ef].tolist())
    _check_finishes(name, r)
    return es, r


@pytest.mark.parametrize("tier", range(5))
def test_routing_per_window(gpu, oracle, tier):
    """Ten end-to-end and twelve ends-free pairs built for one register window; at least 8 of each must be that window's by the restated
    rule (with every tier enabled), and at least 8 of that window's ends-free pairs must have a free begin with more start diagonals than
    the tier's match-run queue has room for (both conditions on the inputs); every pair is finished by the tier it was routed to."""
    _routing_per_window(gpu, oracle, tier, PEN)


@pytest.mark.parametrize("pen", [(2, 3, 1), (6, 9, 3)], ids=["2-3-1", "6-9-3"])
def test_routing_per_window_other_gcd(gpu, oracle, pen):
    """The 1536 window's batch under penalties that reduce to the same (2,4,1) with g = 1 and g = 3: the same assertions, the bound scaled
    by that g; bounds and routing are those of the default penalties (the chain works in units of g), the scores are theirs times g / 2."""
    es, r = _routing_per_window(gpu, oracle, 1, pen)
    _, es_default, r_default = _align(gpu, oracle, "window1")
    assert np.array_equal(es.astype(np.int64) * 2, es_default.astype(np.int64) * gcd_unit(pen))
    for k in ("bound", "routed", "finished"):
        assert np.array_equal(r[k], r_default[k]), k


@pytest.mark.parametrize("cap", sorted(EDGE))
def test_routing_window_edge(gpu, oracle, cap):
    """Insertions one base apart across the point where the wanted window reaches the tier's capacity: a task that wants exactly cap - 1
    diagonals is admitted, one that wants exactly cap is passed on, both occur, and whoever is admitted is finished there."""
    name = "edge%d" % cap
    tasks, es, r = _align(gpu, oracle, name)
    _check_chain(name, tasks, es, r)
    need = np.array([affine_window(tasks[i], int(r["bound"][i]))[1] for i in range(len(tasks))])
    assert np.any(need == cap - 1) and np.any(need == cap), (name, sorted(set(need.tolist())))
    _check_finishes(name, r)


def test_routing_packed_sequence_edge(gpu, oracle):
    """Near-identical pairs whose packed size is exactly a tier's SEQB (that tier's) and four bytes more (the next tier's; tier A beyond the
    last): the sort's size test and the kernels' agree, so everybody finishes where they were routed."""
    name = "seq_edge"
    tasks, es, r = _align(gpu, oracle, name)
    _check_chain(name, tasks, es, r)
    sb = np.array([seq_bytes(t) for t in tasks])
    for t in range(5):
        assert np.count_nonzero(sb == SEQB[t]) == 2 and np.count_nonzero(sb == SEQB[t] + 4) == 2, (t, sb.tolist())
    exp = _expected_tiers(tasks, r, mask=31)
    assert [int(np.count_nonzero(exp == t)) for t in range(6)] == [2, 4, 4, 4, 4, 2], exp.tolist()      # exactly SEQB[t]: tier t; four bytes more: the next
    _check_finishes(name, r)


@pytest.mark.parametrize("window", [1024, 4096])
def test_routing_queue_path(gpu, oracle, window):
    """Match runs that outlive both probes of a slot visit go through the per-wave queue and the patch table; the one-wave body (1024) and the
    multi-wave body (4096: export tables, a barrier per score) both finish such pairs themselves."""
    name = "queue%d" % window
    tasks, es, r = _align(gpu, oracle, name)
    _check_chain(name, tasks, es, r)
    assert np.all(_expected_tiers(tasks, r, mask=31) == CAP.index(window)), name      # a condition on the inputs: every pair is that window's
    _check_finishes(name, r)


def test_routing_non_acgt_lands_in_tier_a(gpu, oracle):
    """Invariant 5: a byte outside ACGT cannot be packed, so the register tier the pair is routed to gives it up at its pack check, and tier A
    (byte compares) finishes it — not tier B, not the generic kernel."""
    name = "non_acgt"
    tasks, es, r = _align(gpu, oracle, name)
    _check_chain(name, tasks, es, r)
    exp = _expected_tiers(tasks, r)
    assert np.all(r["finished"] == 5), (name, r["finished"].tolist())
    if r["mask"]:
        assert np.all(exp < NONE), exp.tolist()                                       # a condition on the inputs: every pair has a register tier
        handed_on = r["tier_a_input"][r["seg"][6] - r["seg"][5]:]
        assert np.array_equal(np.sort(handed_on), np.flatnonzero(exp < NONE)), name


def test_routing_snapshots_do_not_leak(gpu, oracle):
    """Two contexts alternate, and one context repeats a call and then runs a clean batch behind one with give-ups: every snapshot describes
    the launch in front of it and nothing older."""
    with otter_amd.Context(0) as other:
        ta, ea, ra = _align(gpu, oracle, "non_acgt")
        tb, eb, rb = _align(other, oracle, "small")
        ra2 = gpu.affine_last_routing(len(ta))                       # the other context's launch in between changes nothing here
        for k in ("bound", "routed", "finished"):
            assert np.array_equal(ra[k], ra2[k]), k
        _check_chain("small (second context)", tb, eb, rb)
        _check_finishes("small (second context)", rb)
        tc, ec, rc = _align(other, oracle, "non_acgt")
        for k in ("bound", "routed", "finished"):
            assert np.array_equal(ra[k], rc[k]), k
    # the same call again on the session's context, then a clean batch: no give-up of the earlier launches shows
    t1, e1, r1 = _align(gpu, oracle, "non_acgt")
    for k in ("bound", "routed", "finished", "seg"):
        assert np.array_equal(ra[k], r1[k]), k
    assert np.array_equal(np.sort(ra["tier_a_input"]), np.sort(r1["tier_a_input"]))
    t2, e2, r2 = _align(gpu, oracle, "small")
    _check_chain("small", t2, e2, r2)
    _check_finishes("small", r2)
    assert len(r2["tier_a_input"]) == 0 or not r2["mask"]
    assert len(r2["tier_a_gave_up"]) == 0 and len(r2["tier_b_gave_up"]) == 0


def test_routing_refusals(gpu, oracle):
    arena, tasks, _ = _batch("small", oracle)
    n = len(tasks)
    gpu.affine_align_batch(arena, tasks)
    assert gpu.affine_last_routing(n)["routed"].shape == (n,)
    with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\).*%d tasks" % n):      # another task count
        gpu.affine_last_routing(n - 1)
    gpu.edit_distance_batch(arena, tasks)
    with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\).*not the exact gap-affine chain"):
        gpu.affine_last_routing(n)
    gpu.set_heuristic(abi.OTG_HEURISTIC_WFADAPTIVE)
    try:
        gpu.affine_align_batch(arena, tasks)
        with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\).*WFadaptive"):
            gpu.affine_last_routing(n)
    finally:
        gpu.set_heuristic(abi.OTG_HEURISTIC_NONE)
    gpu.affine_align_batch(arena, tasks)
    gpu.affine_last_routing(n)
    gpu.trim()                                                                      # releases the bounds
    with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\)"):
        gpu.affine_last_routing(n)

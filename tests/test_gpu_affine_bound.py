"""GPU: the score bound U of the gap-affine chain's bound pass, task by task, against a plain-Python restatement.

Any valid U leaves scores and op strings exact, but the SAME U keeps the sort's routing, the tiers' populations and every A/B comparison of
the chain exact, so the kernel may be rewritten only as long as it computes this, for penalties that reduce to (2,4,1):
  * a band of 64 diagonals, one per lane; lane 0 starts on diagonal ((lo0 + hi0) >> 1) - 32, where [lo0, hi0] = [-pbf, tbf] are the start
    diagonals (free begins clipped to the sequences' lengths); at most 40 start diagonals, otherwise no bound (INT_MAX);
  * the reversal rule: when pbf + tbf + 1 > 40 and min(pef, pl) + min(tef, tl) + 1 <= 40 the pass runs on both sequences reversed, free
    begins and free ends exchanged;
  * per score s = 1, 2, ... the rows M(s-1) .. M(s-4), I and D of the (2,4,1) recurrence, a cell null when its offset is negative, beyond the
    text or beyond the pattern; cells outside the band are null;
  * on every even score, before the recurrence: the leader is the lowest lane with the largest 2 h - k among the cells of row s-1 with
    h >= 0; when that lane is >= 40 the band moves up one diagonal, when it is < 24 it moves down one;
  * every cell is extended along its matches; the pass ends at the first score with a cell for which one sequence is consumed and the rest of
    the other is free (end to end: both consumed);
  * scores up to smax = pl + tl + 64, then no bound; INT_MAX also for an empty sequence or one of 32 766 bases and more.
`Context.affine_last_routing(n)["bound"]` is what the kernel wrote; score and op string of every pair are compared with the oracle as well."""
import numpy as np
import pytest
from helpers import rand_seq, mutate, pair_tasks

pytestmark = pytest.mark.gpu

NULL = -(1 << 29)
INT_MAX = 0x7fffffff


def _lcp(a, b, v, h, n):
    """equal leading bytes of a[v:] and b[h:], at most n"""
    m, c = 0, 32
    while m < n:
        c2 = min(c, n - m)
        ne = np.flatnonzero(a[v + m:v + m + c2] != b[h + m:h + m + c2])
        if ne.size:
            return m + int(ne[0])
        m += c2
        c *= 4
    return n


def bound_pass(p, t, form):
    """U of one pair; p, t: bytes; form: None (end to end) or (pbf, pef, tbf, tef)."""
    pl, tl = len(p), len(t)
    ef = form is not None
    pbf = min(form[0], pl) if ef else 0
    tbf = min(form[2], tl) if ef else 0
    pef = form[1] if ef else 0
    tef = form[3] if ef else 0
    if pbf + tbf + 1 > 40 and min(pef, pl) + min(tef, tl) + 1 <= 40:
        pbf, pef = min(pef, pl), pbf
        tbf, tef = min(tef, tl), tbf
        p, t = p[::-1], t[::-1]
    lo0, hi0 = -pbf, tbf
    if not (hi0 - lo0 + 1 <= 40 and pl > 0 and tl > 0 and pl < 32766 and tl < 32766):
        return INT_MAX
    pa, ta = np.frombuffer(p, dtype=np.uint8), np.frombuffer(t, dtype=np.uint8)
    bk0 = ((lo0 + hi0) >> 1) - 32
    lanes = range(64)

    def cell(h, k):
        return h if 0 <= h <= tl and h - k <= pl else NULL

    def extend_and_test(row):
        done = False
        for l in lanes:
            h = row[l]
            if h < 0:
                continue
            v = h - (bk0 + l)
            n = min(pl - v, tl - h)
            if n > 0 and p[v] == t[h]:
                h += _lcp(pa, ta, v, h, n)
                v = h - (bk0 + l)
                row[l] = h
            if (h >= tl and pl - v <= pef) or (v >= pl and tl - h <= tef):
                done = True
        return done

    cur = []
    for l in lanes:
        k = bk0 + l
        h = max(k, 0)
        cur.append(h if lo0 <= k <= hi0 and h <= tl and h - k <= pl else NULL)
    if extend_and_test(cur):
        return 0
    M1 = M2 = M3 = M4 = I = D = [NULL] * 64
    for s in range(1, pl + tl + 64 + 1):
        M4, M3, M2, M1 = M3, M2, M1, cur
        if s % 2 == 0:
            prog = [2 * M1[l] - (bk0 + l) if M1[l] >= 0 else NULL for l in lanes]
            best = max(prog)
            if best > NULL:
                bl = prog.index(best)
                if bl >= 40:
                    M1, M2, M3, M4, I, D = (r[1:] + [NULL] for r in (M1, M2, M3, M4, I, D))
                    bk0 += 1
                elif bl < 24:
                    M1, M2, M3, M4, I, D = ([NULL] + r[:-1] for r in (M1, M2, M3, M4, I, D))
                    bk0 -= 1
        nI, nD, cur = [], [], []
        for l in lanes:
            k = bk0 + l
            ins = cell(max(I[l - 1], M4[l - 1]) + 1, k) if l > 0 else NULL
            dele = cell(max(D[l + 1], M4[l + 1]), k) if l < 63 else NULL
            nI.append(ins)
            nD.append(dele)
            cur.append(cell(max(dele, M2[l] + 1, ins), k))
        I, D = nI, nD
        if extend_and_test(cur):
            return s
    return INT_MAX


# ---- the cases (seeded; 8 to 32 pairs each, a batch of 65 for the refill order)
def _ont(rng, n, lmin, lmax, rate=0.1):
    out = []
    for _ in range(n):
        a = rand_seq(rng, int(rng.integers(lmin, lmax + 1)))
        out.append((mutate(rng, a, rate), mutate(rng, a, rate)))
    return out


def _case_ont():
    rng = np.random.default_rng(9100)
    return _ont(rng, 16, 300, 900), None


def _case_long_gap():
    """120 to 200 inserted bases behind a 300-base core, in the text (the band moves up) or in the pattern (down); then more bases follow"""
    rng = np.random.default_rng(9101)
    pairs = []
    for i, g in enumerate(range(120, 201, 10)):
        core, tail = rand_seq(rng, 300), rand_seq(rng, 60 * (i % 3))
        a, b = core + tail, core + rand_seq(rng, g) + tail
        pairs.append((a, b) if i % 2 else (b, a))
    a = rand_seq(rng, 300)
    pairs.append((a + rand_seq(rng, 150) + a, a + a + rand_seq(rng, 130)))         # both ways in one pair
    return pairs, None


def _case_leader_ties():
    rng = np.random.default_rng(9102)
    pairs = []
    for i in range(12):
        unit = [b"A", b"AC", b"T", b"GA", b"CAG", b"G"][i % 6]
        n = 40 + 7 * i
        left, right = rand_seq(rng, 30 + i), rand_seq(rng, 25)
        a = left + unit * n + right
        b = left + unit * (n + (i % 5) - 2) + right
        pairs.append((a, mutate(rng, b, 0.02)) if i % 2 else (b, a))
    pairs.append((b"A" * 200, b"A" * 231))
    pairs.append((b"AC" * 120, b"CA" * 100))
    return pairs, None


def _case_ends_free():
    rng = np.random.default_rng(9103)
    pairs, forms = [], []
    for i in range(4):                                   # a free end at the pattern's end, at the text's end
        a = rand_seq(rng, 400 + 30 * i)
        b = mutate(rng, a, 0.08)
        junk = rand_seq(rng, 20 + 10 * i)
        pairs.append((b + junk, a)); forms.append((0, len(junk) + 5 * (i % 2), 0, 0))
        pairs.append((a, b + junk)); forms.append((0, 0, 0, len(junk) + 3))
    for i, cut in enumerate((41, 45, 52, 60)):           # a free begin of 41 to 60 diagonals: the reversed run
        a = rand_seq(rng, 350)
        b = mutate(rng, a, 0.06)
        junk = rand_seq(rng, cut - 1 - i)
        if i % 2:
            pairs.append((junk + a, b)); forms.append((cut, 0, 0, 0))
        else:
            pairs.append((a, junk + b)); forms.append((0, 3 * i, cut, 0))
    for i in range(3):                                   # at most 40 start diagonals: forwards
        a = rand_seq(rng, 300)
        pairs.append((rand_seq(rng, 12 + i) + a, rand_seq(rng, 9) + mutate(rng, a, 0.05))); forms.append((20 + i, 0, 19 - i, 0))
    for i in range(3):                                   # more than 40 on both sides: no bound
        a = rand_seq(rng, 300)
        pairs.append((rand_seq(rng, 30) + a + rand_seq(rng, 33), mutate(rng, a, 0.05))); forms.append((41 + 20 * i, 60, 0, 0))
    return pairs, forms


def _near(rng, base, la, lb, edits=3):
    a, b = bytearray(base[:la]), bytearray(base[:lb])
    for s_ in (a, b):
        for _ in range(edits):
            i = int(rng.integers(0, len(s_)))
            s_[i] = b"ACGT"[(b"ACGT".index(s_[i]) + 1) % 4]
    return bytes(a), bytes(b)


def _case_packed_small():
    """lengths 0, 1 and 15 mod 16; one pair just under and one just over 800 words of packed pair (397 + 397 + 6, then one word more)"""
    rng = np.random.default_rng(9104)
    pairs = _ont(rng, 2, 320, 320) + _ont(rng, 2, 321, 321) + _ont(rng, 2, 335, 335)
    pairs = [(a[:n], b[:m]) for (a, b), (n, m) in zip(pairs, ((320, 304), (288, 320), (321, 305), (289, 321), (335, 319), (303, 335)))]
    base = rand_seq(rng, 6400)
    pairs += [_near(rng, base, 6352, 6352), _near(rng, base, 6353, 6352), _near(rng, base, 6337, 6368)]
    return pairs, None


def _case_packed_long(n):
    """near-identical pairs whose longest read selects each wider shape of the pass; the last: the limit of 32 766 bases, 16 bases around it"""
    def build():
        rng = np.random.default_rng(9105 + n)
        base = rand_seq(rng, n + 40)
        if n < 32000:
            return [_near(rng, base, n, n - 17), _near(rng, base, n - 33, n)] + _ont(rng, 6, 200, 500), None
        pairs = [_near(rng, base, 32765, 32765), _near(rng, base, 32749, 32765), _near(rng, base, 32765 - 31, 32750),
                 _near(rng, base, 32766, 32700), _near(rng, base, 32700, 32782)] + _ont(rng, 3, 200, 500)
        return pairs, None
    return build


def _case_non_acgt():
    rng = np.random.default_rng(9106)
    pairs = []
    for i, (a, b) in enumerate(_ont(rng, 8, 300, 600)):
        a, b = bytearray(a), bytearray(b)
        if i % 2 == 0 or i == 7:
            a[int(rng.integers(0, len(a)))] = b"NnacgtNR"[i]
        if i % 2 == 1:
            b[int(rng.integers(0, len(b)))] = b"NnacgtNR"[i]
        pairs.append((bytes(a), bytes(b)))
    return pairs + _ont(rng, 2, 300, 400), None


def _case_tiny():
    rng = np.random.default_rng(9107)
    a = rand_seq(rng, 50)
    pairs = [(b"A", b"A"), (b"A", b"C"), (b"G", a), (a, b"T"), (b"AC", b"A"), (b"A", b"CA"), (a, a), (a[:1], a[:2])]
    forms = [None, None, None, None, (0, 1, 0, 0), (0, 0, 1, 0), None, (0, 0, 0, 1)]
    return pairs, forms


def _case_empty():
    rng = np.random.default_rng(9108)
    a = rand_seq(rng, 40)
    return [(b"", a), (a, b""), (a, mutate(rng, a, 0.1)), (b"", a)], [None, None, None, (0, 0, 0, 40)]


def _case_count(n):
    def build():
        rng = np.random.default_rng(9110 + n)
        return _ont(rng, n, 100, 250 if n > 8 else 400), None
    return build


def _case_alternating():
    """a 200-base pair, then a 3 000-base pair, and so on: neighbours of the work list finish far apart"""
    rng = np.random.default_rng(9109)
    pairs = []
    for i in range(6):
        pairs += _ont(rng, 1, 200, 200, 0.08) + _ont(rng, 1, 3000, 3000, 0.02)
    return pairs, None


CASES = {"ont": _case_ont, "long_gap": _case_long_gap, "leader_ties": _case_leader_ties, "ends_free": _case_ends_free,
         "packed_small": _case_packed_small, "packed_12288": _case_packed_long(12288), "packed_16384": _case_packed_long(16384),
         "packed_32766": _case_packed_long(32766), "non_acgt": _case_non_acgt, "tiny": _case_tiny, "empty": _case_empty,
         "count1": _case_count(1), "count2": _case_count(2), "count3": _case_count(3), "count65": _case_count(65), "alternating": _case_alternating}
_cache = {}


def _case(name, oracle):
    if name not in _cache:
        pairs, forms = CASES[name]()
        arena, tasks = pair_tasks(pairs, forms)
        want = np.array([bound_pass(p, t, forms[i] if forms else None) for i, (p, t) in enumerate(pairs)], dtype=np.int64)
        _cache[name] = (arena, tasks, want, oracle.affine_align_batch(arena, tasks))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_bound_is_the_restated_pass(gpu, oracle, name):
    arena, tasks, want, (es, ec) = _case(name, oracle)
    gs, gc = gpu.affine_align_batch(arena, tasks)
    got = gpu.affine_last_routing(len(tasks))["bound"].astype(np.int64)
    print("%s: bound %s" % (name, got.tolist()))
    assert np.array_equal(got, want), (name, [(int(i), int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)[:8]])
    assert np.array_equal(gs, es), (name, [(int(i), int(gs[i]), int(es[i])) for i in np.flatnonzero(gs != es)[:8]])
    bad = [i for i in range(len(tasks)) if gc[i] != ec[i]]
    assert not bad, (name, bad[:10])


def test_cases_are_what_they_claim(oracle):
    """conditions on the inputs: the reversed run, the missing bound, a bound far above the optimum across a long gap, both paths around the
    limit of 32 766 bases"""
    _, tasks, want, _ = _case("ends_free", oracle)
    assert np.count_nonzero(want == INT_MAX) == 3 and np.count_nonzero(want < INT_MAX) == len(want) - 3, want.tolist()
    _, tasks, want, (es, _) = _case("long_gap", oracle)
    assert np.all(want * 2 >= es) and np.count_nonzero(want * 2 > es + 100) >= 8, (want.tolist(), es.tolist())
    _, tasks, want, _ = _case("packed_32766", oracle)
    assert want[:3].max() < 64 and np.all(want[3:5] == INT_MAX), want.tolist()
    _, tasks, want, _ = _case("empty", oracle)
    assert want.tolist() == [INT_MAX, INT_MAX, want[2], INT_MAX] and want[2] < 64, want.tolist()

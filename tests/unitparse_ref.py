"""The rule of the joint unit parse (include/otter_gpu.h) restated in plain Python: the DP of step 2 and the traceback of step 3 as written
(unitparse), the same rows vectorised for long alleles (unitparse_np), and the language of step 1 enumerated as an independent witness
(unitparse_brute).  A result is (record, segments): record = (edits, switches, unit_bases, n_segments, end_unit, end_phase, flags), a segment
(unit, begin, end, unit_bases, edits, start_phase)."""
import numpy as np

MAX_UNITS = 8
MAX_UNIT = 256
MAX_LANES = 64
FIELD = 21                                  # bits of the two low key fields
MAX_LEN = ((1 << FIELD) - 1 - 2 * MAX_UNIT + 1) // 2
TOO_LONG = 1
SW = 1 << FIELD                             # one switch
E = 1 << (2 * FIELD)                        # one edit
W = E + 1                                   # one edit and one unit base

_CODE = {ord(a): i for i, pair in enumerate(("Aa", "Cc", "Gg", "Tt")) for a in pair}


def codes(b):
    return [_CODE.get(x, 4) for x in bytes(b)]


def check_units(units):
    """the refusals of step 5 that are the caller's"""
    if not 1 <= len(units) <= MAX_UNITS:
        raise ValueError("%d units in a set" % len(units))
    if any(not 1 <= len(u) <= MAX_UNIT for u in units):
        raise ValueError("a unit of %s bytes" % [len(u) for u in units])
    if sum((len(u) + 3) // 4 for u in units) > MAX_LANES:
        raise ValueError("the unit set does not fit one wave")


def _fields(key):
    return key >> (2 * FIELD), (key >> FIELD) & (SW - 1), key & (SW - 1)


def _trace(cs, cu, rows, L):
    """step 3 over the stored rows of keys rows[i][k][j]; -> (end_unit, end_phase, segments)"""
    last = rows[L]
    best = min(min(r) for r in last)
    k, j = next((k, j) for k in range(len(cu)) for j in range(len(cu[k])) if last[k][j] == best)
    end_unit, end_phase = k, j
    i = L
    segs = []
    cur = [k, None, L, 0, 0, 0]             # unit, begin, end, unit_bases, edits, start_phase
    while True:
        v = rows[i][k][j]
        if i == 0:
            assert v == 0
            break
        p = len(cu[k])
        jp = (j - 1) % p
        miss = not (cs[i - 1] == cu[k][jp] and cs[i - 1] < 4)
        if rows[i - 1][k][jp] + (E if miss else 0) + 1 == v:
            cur[3] += 1; cur[4] += miss
            i, j = i - 1, jp
        elif rows[i - 1][k][j] + E == v:
            cur[4] += 1
            i -= 1
        elif rows[i][k][jp] + W == v:
            cur[3] += 1; cur[4] += 1
            j = jp
        else:
            assert j == 0
            src = next(q for q in range(len(cu)) if q != k and rows[i][q][0] + SW == v)
            cur[1] = i
            segs.append(tuple(cur))
            k = src
            cur = [k, None, i, 0, 0, 0]
    cur[1], cur[5] = 0, j
    segs.append(tuple(cur))
    return end_unit, end_phase, segs[::-1]


def _result(cs, cu, rows, L):
    end_unit, end_phase, segs = _trace(cs, cu, rows, L)
    e, sw, ub = _fields(rows[L][end_unit][end_phase])
    return (e, sw, ub, len(segs), end_unit, end_phase, 0), segs


def unitparse(s, units):
    """steps 2 and 3 as written: rows of keys, the skip and the switch relaxed together until nothing changes"""
    s, units = bytes(s), [bytes(u) for u in units]
    check_units(units)
    L = len(s)
    if L > MAX_LEN:
        return (0, 0, 0, 0, 0, 0, TOO_LONG), []
    if L == 0:
        return (0, 0, 0, 0, 0, 0, 0), []
    cs, cu = codes(s), [codes(u) for u in units]
    K = len(cu)
    rows = [[[0] * len(u) for u in cu]]
    for i in range(L):
        V = rows[-1]
        T = []
        for k in range(K):
            p = len(cu[k])
            t = [V[k][j] + E for j in range(p)]
            for j in range(p):
                jn = (j + 1) % p
                t[jn] = min(t[jn], V[k][j] + (0 if cs[i] == cu[k][j] and cs[i] < 4 else E) + 1)
            T.append(t)
        changed = True
        while changed:
            changed = False
            for k in range(K):
                p = len(cu[k])
                for j in range(p):
                    jn = (j + 1) % p
                    if T[k][j] + W < T[k][jn]:
                        T[k][jn] = T[k][j] + W; changed = True
                for q in range(K):
                    if q != k and T[k][0] + SW < T[q][0]:
                        T[q][0] = T[k][0] + SW; changed = True
        rows.append(T)
    return _result(cs, cu, rows, L)


def unitparse_np(s, units):
    """the same rows vectorised: per unit the biased running minimum, the phase-0 candidates and one minimum over them"""
    s, units = bytes(s), [bytes(u) for u in units]
    check_units(units)
    L = len(s)
    if L > MAX_LEN:
        return (0, 0, 0, 0, 0, 0, TOO_LONG), []
    if L == 0:
        return (0, 0, 0, 0, 0, 0, 0), []
    cs = codes(s)
    cu = [codes(u) for u in units]
    K = len(cu)
    prev = [np.roll(np.array(u, dtype=np.int64), 1) for u in cu]
    jj = [np.arange(len(u), dtype=np.int64) for u in cu]
    V = [np.zeros(len(u), dtype=np.int64) for u in cu]
    rows = [V]
    for i in range(L):
        T, last = [], []
        for k in range(K):
            p = len(cu[k])
            miss = (prev[k] != cs[i]) | (cs[i] >= 4)
            t = np.minimum(np.roll(V[k], 1) + miss * E + 1, V[k] + E)
            bias = (p - 1 - jj[k]) * W
            t = np.minimum.accumulate(t + bias) - bias
            T.append(t); last.append(int(t[p - 1]))
        G = min(min(int(T[k][0]), last[k] + W) for k in range(K))
        V = [np.minimum(T[k], min(last[k] + W, G + SW) + jj[k] * W) for k in range(K)]
        rows.append(V)
    return _result(cs, cu, [[[int(x) for x in r] for r in row] for row in rows] if L < 2000 else _Rows(rows), L)


class _Rows:
    """rows of numpy arrays read as Python integers"""

    def __init__(self, rows):
        self.rows = rows

    def __getitem__(self, i):
        return [_Row(r) for r in self.rows[i]]


class _Row:
    def __init__(self, r):
        self.r = r

    def __getitem__(self, j):
        return int(self.r[j])

    def __iter__(self):
        return (int(x) for x in self.r)


def _edit(cs, ct):
    n = len(ct)
    V = list(range(n + 1))
    for c in cs:
        T = [V[0] + 1] + [0] * n
        for k in range(n):
            T[k + 1] = min(V[k + 1] + 1, V[k] + (0 if c == ct[k] and c < 4 else 1), T[k] + 1)
        V = T
    return V[n]


def unitparse_brute(s, units):
    """step 1 directly: every concatenation of pieces up to 2 L bases (a longer one cannot be the minimum) -> (edits, switches, unit_bases)"""
    cs, cu = codes(bytes(s)), [codes(bytes(u)) for u in units]
    cap = 2 * len(cs)
    found = {(): 0}                          # the bases of t -> the fewest switches that spell them

    def grow(t, k, sw):
        # t ends with the last base of a copy of unit k; the next piece starts another unit at its base 0
        for q in range(len(cu)):
            if q != k:
                piece(t, q, 0, sw + 1)

    def piece(t, k, a, sw):
        p = len(cu[k])
        for n in range(1, cap - len(t) + 1):
            t = t + (cu[k][(a + n - 1) % p],)
            if found.get(t, 1 << 30) > sw:
                found[t] = sw
            if (a + n) % p == 0:
                grow(t, k, sw)

    for k in range(len(cu)):
        for a in range(len(cu[k])):
            piece((), k, a, 0)
    return min((_edit(cs, t), sw, len(t)) for t, sw in found.items())


def fmt_copies(ub, p):
    return b"%d" % (ub // p) if ub % p == 0 else b"%.2f" % (ub / p)


def row(region, i, seq_len, units, rec, segs):
    """the row of otter_unitparse for allele i of a region; units = the set as given ([]: the region has none)"""
    edits, sw, ub, _, _, _, flags = rec
    counted = len(units) != 0 and flags == 0
    span = max(seq_len, ub)
    identity = 1.0 - edits / span if counted and span else 0.0
    if not units:
        return region + b"\t%d\t%d\t.\t0\t0\t0\t%.4f\t.\t.\n" % (i, seq_len, identity)
    counts = b",".join(b"%.2f" % (sum(g[3] for g in segs if g[0] == k) / len(u)) for k, u in enumerate(units))
    structure = b"".join(b"(" + units[g[0]] + b")" + fmt_copies(g[3], len(units[g[0]])) + (b"~%d" % g[4] if g[4] else b"") for g in segs) or b"."
    return region + b"\t%d\t%d\t%s\t%d\t%d\t%d\t%.4f\t%s\t%s\n" % (i, seq_len, b",".join(units), edits, sw, ub, identity, counts, structure)

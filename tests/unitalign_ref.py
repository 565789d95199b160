"""The rule of the cyclic unit alignment (include/otter_gpu.h) restated in plain Python, in two forms, and the brute-force form of its
step 2 as an independent witness.  Every function returns (edits, unit_bases, end_phase, flags)."""
import numpy as np

MAX_UNIT = 256
MAX_LEN = 1048575
NO_UNIT, TOO_LONG, UNIT_TOO_LONG = 1, 2, 4
E = 1 << 32
W = E + 1

_CODE = {ord(a): i for i, pair in enumerate(("Aa", "Cc", "Gg", "Tt")) for a in pair}


def codes(b):
    return [_CODE.get(x, 4) for x in bytes(b)]


def refusal(L, p, chained=False):
    """the flags of a pair that is not aligned (step 6-8); 0: it is"""
    if p == 0:
        return NO_UNIT
    if p > MAX_UNIT:
        if not chained:
            raise ValueError("a unit of %d bytes" % p)
        return UNIT_TOO_LONG
    if L > MAX_LEN:
        return TOO_LONG
    return 0


def unitalign(s, u, chained=False):
    """step 3 as written: rows of keys, the skipped-unit-base step by 2 p sequential relaxations"""
    s, u = bytes(s), bytes(u)
    L, p = len(s), len(u)
    f = refusal(L, p, chained)
    if f:
        return (0, 0, 0, f)
    cs, cu = codes(s), codes(u)
    V = [0] * p
    for i in range(L):
        T = [None] * p
        for j in range(p):
            jn = (j + 1) % p
            d = V[j] + (0 if cs[i] == cu[j] and cs[i] < 4 else E) + 1
            T[jn] = d if T[jn] is None else min(T[jn], d)
        for j in range(p):
            T[j] = min(T[j], V[j] + E)
        for k in range(2 * p):
            j = k % p
            jn = (j + 1) % p
            T[jn] = min(T[jn], T[j] + W)
        V = T
    best = min(V)
    return (best >> 32, best & (E - 1), V.index(best), 0)


def unitalign_np(s, u, chained=False):
    """the same rows vectorised: the closure as one biased running minimum and the wrap term"""
    s, u = bytes(s), bytes(u)
    L, p = len(s), len(u)
    f = refusal(L, p, chained)
    if f:
        return (0, 0, 0, f)
    cs = np.array(codes(s), dtype=np.int64)
    cu = np.array(codes(u), dtype=np.int64)
    cu_prev = np.roll(cu, 1)
    j = np.arange(p, dtype=np.int64)
    bias = (p - 1 - j) * W
    wrap = (j + 1) * W
    V = np.zeros(p, dtype=np.int64)
    for i in range(L):
        miss = (cu_prev != cs[i]) | (cs[i] >= 4)
        T = np.minimum(np.roll(V, 1) + miss * E + 1, V + E)
        H1 = np.minimum.accumulate(T + bias) - bias
        V = np.minimum(H1, H1[p - 1] + wrap)
    b = int(V.min())
    return (b >> 32, b & (E - 1), int(np.argmin(V)), 0)


def row(region, i, seq_len, source, unit, rec):
    """the row of otter_copies for allele i of a region; rec = (edits, unit_bases, end_phase, flags)"""
    edits, ub, _, flags = rec
    p = len(unit)
    counted = p != 0 and flags == 0
    span = max(seq_len, ub)
    copies = ub / p if counted else 0.0
    identity = 1.0 - edits / span if counted and span else 0.0
    return region + b"\t%d\t%d\t%s\t%s\t%d\t%d\t%.2f\t%.4f\n" % (i, seq_len, source, unit or b".", edits, ub, copies, identity)


def _semiglobal(cs, ct):
    """for t = ct: min over substrings t[a:b] of (edit distance to s, b - a), by a DP that is free in where it starts and stops on t"""
    n = len(ct)
    V = [0] * (n + 1)                       # key = edits * E + length of the substring used
    for c in cs:
        T = [V[0] + E] + [0] * n
        for k in range(n):
            T[k + 1] = min(V[k + 1] + E, V[k] + (0 if c == ct[k] and c < 4 else E) + 1, T[k] + W)
        V = T
    return min(V)


def unitalign_brute(s, u):
    """step 2 directly: s against u repeated 2 L / p + 3 times, from every start phase"""
    s, u = bytes(s), bytes(u)
    L, p = len(s), len(u)
    cs, cu = codes(s), codes(u)
    reps = 2 * L // p + 3
    best = None
    for ph in range(p):
        ct = (cu[ph:] + cu[:ph]) * reps
        b = _semiglobal(cs, ct)
        best = b if best is None else min(best, b)
    return (best >> 32, best & (E - 1))

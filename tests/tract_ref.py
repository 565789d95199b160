"""The rule of the tract mode (include/otter_gpu.h, "Tract mode") restated in plain Python: the local wraparound alignment in two forms,
the brute-force local alignment as an independent witness of the score, and the tract record built on the unit alignment's own reference.
tract() and tract_np() return (score, begin, end, edits, unit_bases, end_phase, start_phase, flags)."""
import numpy as np
import unitalign_ref as U

MAX_UNIT = U.MAX_UNIT
MAX_LEN = 1048575
NO_UNIT, TOO_LONG, UNIT_TOO_LONG, NONE = 1, 2, 4, 8
DEFAULT = (2, 7, 7, 24)                    # match, mismatch, indel, min_score
E = 1 << 32


def params_ok(match, mismatch, indel, min_score):
    return 1 <= match <= 16 and 1 <= mismatch <= 64 and 1 <= indel <= 64 and 0 <= min_score <= 1 << 24


def refusal(L, p, chained=False):
    if p == 0:
        return NO_UNIT
    if p > MAX_UNIT:
        if not chained:
            raise ValueError("a unit of %d bytes" % p)
        return UNIT_TOO_LONG
    if L > MAX_LEN:
        return TOO_LONG
    return 0


def local(s, u, match=2, mismatch=7, indel=7):
    """steps 1-4 as written: cells are (score, begin) pairs, the skipped-unit-base step by 2 p sequential relaxations -> (score, begin, end)"""
    cs, cu = U.codes(s), U.codes(u)
    L, p = len(cs), len(cu)
    C = [(0, 0)] * p
    best = (0, 0, 0, 0)                     # (score, -end, begin, -j): the largest wins
    for i in range(L):
        T = [(0, i + 1)] * p
        for j in range(p):
            jn = (j + 1) % p
            sc = C[j][0] + (match if cs[i] == cu[j] and cs[i] < 4 else -mismatch)
            if sc > 0:
                T[jn] = max(T[jn], (sc, C[j][1]))
            if C[j][0] - indel > 0:
                T[j] = max(T[j], (C[j][0] - indel, C[j][1]))
        for k in range(2 * p):
            j = k % p
            jn = (j + 1) % p
            if T[j][0] - indel > 0:
                T[jn] = max(T[jn], (T[j][0] - indel, T[j][1]))
        C = T
        for j in range(p):
            best = max(best, (C[j][0], -(i + 1), C[j][1], -j))
    return best[0], best[2], -best[1]


def local_np(s, u, match=2, mismatch=7, indel=7):
    """the same rows vectorised on keys score * 2^32 + begin: the closure as one biased running maximum and the wrap term"""
    cs = np.array(U.codes(s), dtype=np.int64)
    cu = np.array(U.codes(u), dtype=np.int64)
    L, p = len(cs), len(cu)
    cu_prev = np.roll(cu, 1)
    j = np.arange(p, dtype=np.int64)
    bias, wrap = j * indel * E, (j + 1) * indel * E
    V = np.zeros(p, dtype=np.int64)
    bk, be = np.zeros(p, dtype=np.int64), np.zeros(p, dtype=np.int64)
    for i in range(L):
        hit = (cu_prev == cs[i]) & (cs[i] < 4)
        D = np.roll(V, 1)
        T = np.maximum(np.where(hit, D + match * E, np.maximum(D - mismatch * E, 0)), np.maximum(V - indel * E, 0))
        T = np.maximum(T, i + 1)
        H1 = np.maximum.accumulate(T + bias) - bias
        V = np.maximum(H1, np.maximum(H1[p - 1] - wrap, 0))
        up = (V >> 32) > (bk >> 32)
        bk = np.where(up, V, bk)
        be = np.where(up, i + 1, be)
    order = sorted(range(p), key=lambda q: (-(int(bk[q]) >> 32), int(be[q]), -(int(bk[q]) & (E - 1)), q))
    q = order[0]
    return int(bk[q]) >> 32, int(bk[q]) & (E - 1), int(be[q])


def _record(s, u, loc, min_score, chained):
    s, u = bytes(s), bytes(u)
    f = refusal(len(s), len(u), chained)
    if f:
        return (0, 0, 0, 0, 0, 0, 0, f)
    score, begin, end = loc(s, u)
    if score == 0 or score < min_score:
        return (score, 0, 0, 0, 0, 0, 0, NONE)
    e, ub, ph, _ = U.unitalign_np(s[begin:end], u)
    return (score, begin, end, e, ub, ph, (ph - ub) % len(u), 0)


def tract(s, u, match=2, mismatch=7, indel=7, min_score=24, chained=False):
    return _record(s, u, lambda a, b: local(a, b, match, mismatch, indel), min_score, chained)


def tract_np(s, u, match=2, mismatch=7, indel=7, min_score=24, chained=False):
    return _record(s, u, lambda a, b: local_np(a, b, match, mismatch, indel), min_score, chained)


def score_brute(s, u, match=2, mismatch=7, indel=7):
    """the score alone: a plain local alignment of s against u repeated 2 L / p + 3 times, from every start phase"""
    cs, cu = U.codes(s), U.codes(u)
    L, p = len(cs), len(cu)
    best = 0
    for ph in range(p):
        ct = (cu[ph:] + cu[:ph]) * (2 * L // p + 3)
        n = len(ct)
        H = [0] * (n + 1)
        for c in cs:
            N = [0] * (n + 1)
            for k in range(n):
                N[k + 1] = max(0, H[k] + (match if c == ct[k] and c < 4 else -mismatch), H[k + 1] - indel, N[k] - indel)
            H = N
            best = max(best, max(H))
    return best


def narrow_len(match, indel, p):
    """the longest allele of the 32-bit key (otg_tract_core.hpp): begin <= L and match * L + (p - 1) * indel stay below 2^16"""
    return min(65535, (65535 - (p - 1) * indel) // match)


def row(region, i, seq_len, source, unit, rec):
    """the row of otter_tracts for allele i of a region; rec = the eight fields of tract()"""
    score, begin, end, edits, ub, _, _, flags = rec
    p = len(unit)
    counted = p != 0 and flags == 0
    span = max(end - begin, ub)
    copies = ub / p if counted else 0.0
    identity = 1.0 - edits / span if counted and span else 0.0
    return region + b"\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%.2f\t%.4f\n" % (i, seq_len, source, unit or b".", begin, end, score, edits, ub, copies, identity)

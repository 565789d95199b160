"""The rule of the locus mode (include/otter_gpu.h, "Locus mode") restated in plain Python: the local wraparound alignment over a unit set in
two forms (step 3 as written, relaxed to its fixed point; the closed form per row, vectorised), a brute-force witness of the score over the
enumerated language, and the record built on the joint parse's own reference.  locus() and locus_np() return (record, segments): record =
(score, begin, end, edits, switches, unit_bases, n_segments, flags), a segment (unit, begin, end, unit_bases, edits, start_phase) in allele
positions."""
import numpy as np
import unitparse_ref as P

MAX_LEN = P.MAX_LEN
TOO_LONG, NONE = 1, 2
DEFAULT = (2, 7, 7, 24)                    # match, mismatch, indel, min_score
E = 1 << 32
codes = P.codes


def local(s, units, match=2, mismatch=7, indel=7):
    """steps 1-4 as written: cells are (score, begin) pairs; the skipped unit base and the switch relaxed together until nothing changes
    -> (score, begin, end)"""
    cs, cu = codes(s), [codes(u) for u in units]
    K = len(cu)
    C = [[(0, 0)] * len(u) for u in cu]
    best = (0, 0, 0, 0, 0)                  # (score, -end, begin, -k, -j): the largest wins
    for i in range(len(cs)):
        T = [[(0, i + 1)] * len(u) for u in cu]
        for k in range(K):
            p = len(cu[k])
            for j in range(p):
                jn = (j + 1) % p
                sc = C[k][j][0] + (match if cs[i] == cu[k][j] and cs[i] < 4 else -mismatch)
                if sc > 0:
                    T[k][jn] = max(T[k][jn], (sc, C[k][j][1]))
                if C[k][j][0] - indel > 0:
                    T[k][j] = max(T[k][j], (C[k][j][0] - indel, C[k][j][1]))
        changed = True
        while changed:
            changed = False
            for k in range(K):
                p = len(cu[k])
                for j in range(p):
                    jn = (j + 1) % p
                    cand = (T[k][j][0] - indel, T[k][j][1])
                    if cand[0] > 0 and cand > T[k][jn]:
                        T[k][jn] = cand; changed = True
                for q in range(K):
                    if q != k and T[k][0][0] > 0 and T[k][0] > T[q][0]:
                        T[q][0] = T[k][0]; changed = True
        C = T
        for k in range(K):
            for j in range(len(cu[k])):
                best = max(best, (C[k][j][0], -(i + 1), C[k][j][1], -k, -j))
    return best[0], best[2], -best[1]


def _sub(x, pen):
    """the saturating subtract of a key: a score that would not stay positive leaves less than every fresh start"""
    return np.maximum(x, pen) - pen


def local_np(s, units, match=2, mismatch=7, indel=7):
    """the same rows on keys score * 2^32 + begin by the closed form: per unit the biased running maximum, the phase-0 candidates, one
    maximum over them, the entry and the way on"""
    cs = codes(s)
    cu = [np.array(codes(u), dtype=np.int64) for u in units]
    K = len(cu)
    prev = [np.roll(u, 1) for u in cu]
    jj = [np.arange(len(u), dtype=np.int64) for u in cu]
    V = [np.zeros(len(u), dtype=np.int64) for u in cu]
    g = indel * E
    bk = [np.zeros(len(u), dtype=np.int64) for u in cu]
    be = [np.zeros(len(u), dtype=np.int64) for u in cu]
    for i in range(len(cs)):
        H1, last = [], []
        for k in range(K):
            hit = (prev[k] == cs[i]) & (cs[i] < 4)
            D = np.roll(V[k], 1)
            T = np.maximum(np.where(hit, D + match * E, _sub(D, mismatch * E)), _sub(V[k], g))
            T = np.maximum(T, i + 1)
            bias = jj[k] * g
            h = np.maximum.accumulate(T + bias) - bias
            H1.append(h); last.append(int(h[-1]))
        best0 = max(max(int(H1[k][0]), int(_sub(last[k], g))) for k in range(K))
        for k in range(K):
            entry = max(int(_sub(last[k], g)), best0)
            V[k] = np.maximum(H1[k], _sub(np.full(len(jj[k]), entry, dtype=np.int64), jj[k] * g))
            up = (V[k] >> 32) > (bk[k] >> 32)
            bk[k] = np.where(up, V[k], bk[k])
            be[k] = np.where(up, i + 1, be[k])
    cells = [(-(int(bk[k][j]) >> 32), int(be[k][j]), -(int(bk[k][j]) & (E - 1)), k, j) for k in range(K) for j in range(len(cu[k]))]
    sc, end, nb, _, _ = min(cells)
    return -sc, -nb, end


def _record(s, units, loc, min_score):
    s, units = bytes(s), [bytes(u) for u in units]
    P.check_units(units)
    if len(s) > MAX_LEN:
        return (0, 0, 0, 0, 0, 0, 0, TOO_LONG), []
    score, begin, end = loc(s, units)
    if score == 0 or score < min_score:
        return (score, 0, 0, 0, 0, 0, 0, NONE), []
    (e, sw, ub, ns, _, _, _), segs = P.unitparse_np(s[begin:end], units)
    return (score, begin, end, e, sw, ub, ns, 0), [(u, b + begin, x + begin, n, ed, ph) for u, b, x, n, ed, ph in segs]


def locus(s, units, match=2, mismatch=7, indel=7, min_score=24):
    return _record(s, units, lambda a, b: local(a, b, match, mismatch, indel), min_score)


def locus_np(s, units, match=2, mismatch=7, indel=7, min_score=24):
    return _record(s, units, lambda a, b: local_np(a, b, match, mismatch, indel), min_score)


def words(units, n):
    """the words of exactly n bases of the language of the joint parse (step 1 there), as code tuples: every shorter word is a substring of one"""
    cu = [codes(u) for u in units]
    out = set()

    def grow(t, k, j):
        if len(t) == n:
            out.add(t)
            return
        t = t + (cu[k][j],)
        if j + 1 < len(cu[k]):
            grow(t, k, j + 1)
        else:
            for q in range(len(cu)):
                grow(t, q, 0)

    for k in range(len(cu)):
        for j in range(len(cu[k])):
            grow((), k, j)
    return sorted(out)


def word_cap(L, match, indel):
    """no local alignment of positive score consumes more unit bases: L by diagonal steps, and fewer skips than match * L / indel"""
    return L + (match * L - 1) // indel if L else 0


def score_brute(s, units, match=2, mismatch=7, indel=7):
    """the score alone: the language is closed under taking substrings, so it is the largest plain Smith-Waterman score of s against a word"""
    cs = codes(s)
    n = word_cap(len(cs), match, indel)
    if n == 0:
        return 0
    W = np.array(words(units, n), dtype=np.int64)
    H = np.zeros((len(W), n + 1), dtype=np.int64)
    best = 0
    for c in cs:
        N = np.zeros_like(H)
        for k in range(n):
            sub = np.where((W[:, k] == c) & (c < 4), match, -mismatch)
            N[:, k + 1] = np.maximum(np.maximum(0, H[:, k] + sub), np.maximum(H[:, k + 1] - indel, N[:, k] - indel))
        H = N
        best = max(best, int(H.max()))
    return best


def narrow_len(match, indel, p_max):
    """the longest allele of the 32-bit key (otg_locus_core.hpp): that of the tract mode for the largest unit of the set"""
    return min(65535, (65535 - (p_max - 1) * indel) // match)


def unit_class(lens, seg64=False):
    """the class of a unit set (otg_unitparse_core.hpp: up_class), 4 at least when every task takes a whole wave"""
    for c, r in ((None, 1), (5, 2), (6, 4)):
        n = sum((p + r - 1) // r for p in lens)
        if n <= 64:
            if c is None:
                c = 4 if n > 32 else 3 if n > 16 else 2 if n > 8 else 1 if n > 4 else 0
            return max(c, 4) if seg64 else c
    raise ValueError("the unit set does not fit one wave")


def row(region, i, seq_len, units, rec, segs):
    """the row of otter_loci for allele i of a region; units = the set as given ([]: the region has none)"""
    score, begin, end, edits, sw, ub, _, flags = rec
    if not units:
        return region + b"\t%d\t%d\t.\t0\t0\t0\t0\t0\t0\t0.0000\t.\t.\n" % (i, seq_len)
    span = max(end - begin, ub)
    identity = 1.0 - edits / span if flags == 0 and span else 0.0
    counts = b",".join(b"%.2f" % (sum(g[3] for g in segs if g[0] == k) / len(u)) for k, u in enumerate(units))
    structure = b"".join(b"(" + units[g[0]] + b")" + P.fmt_copies(g[3], len(units[g[0]])) + (b"~%d" % g[4] if g[4] else b"") for g in segs) or b"."
    return region + b"\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.4f\t%s\t%s\n" % (i, seq_len, b",".join(units), begin, end, score, edits, sw, ub, identity, counts,
                                                                            structure)

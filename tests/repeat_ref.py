"""The repeat-structure rule of include/otter_gpu.h ("Repeat structure of alleles"), restated from that text in plain Python: every comparison
is on Python integers; numpy only finds the run boundaries of the match bits, so that 32-k and 1-M alleles stay cheap.

structure(seq, ...) -> dict(segs=[(begin, period, copies, length)], n_segments, n_repeats, covered, flags, depth, best_calls, moved):
depth = the deepest horizon stack, best_calls = the number of best() evaluations, moved = the placements where step 6 moved st."""
import numpy as np

MAX_PERIOD = 4096
MAX_LEN = 1048575
TOO_LONG = 1
TEXT_LITERAL = 24

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[ord(chr(_ch).lower())] = _i


def codes(seq):
    return _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]


def enough(k, p, min_copies, min_span):
    return k >= min_copies and k * p >= min_span


def kept_runs(c, max_period, min_copies, min_span):
    """steps 2 and 3: the kept runs (p, a, e), in (p, a) order"""
    L = len(c)
    out = []
    for p in range(1, min(max_period, L // 2) + 1):
        e = ((c[:L - p] == c[p:]) & (c[:L - p] < 4)).astype(np.int8)
        d = np.diff(np.concatenate(([0], e, [0])))
        for a, b in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):
            end = b + p
            if enough((end - a) // p, p, min_copies, min_span):
                out.append((p, a, end))
    return out


def best(runs, lo, hi, min_copies, min_span):
    """step 4: (g, w, st, run) of the best run under [lo, hi), or None"""
    win = None
    for run in runs:
        p, a, e = run
        st, en = max(a, lo), min(e, hi)
        if en <= st:
            continue
        k = (en - st) // p
        if not enough(k, p, min_copies, min_span):
            continue
        g, w = st - lo + k * p, st - lo + p
        if win is None:
            win = (g, w, st, run)
            continue
        x, y = g * win[1], win[0] * w
        if x > y or (x == y and (st < win[2] or (st == win[2] and p < win[3][0]))):
            win = (g, w, st, run)
    return win


def structure(seq, max_period=256, min_copies=2, min_span=12):
    assert 1 <= max_period <= MAX_PERIOD and 2 <= min_copies <= 1024 and 2 <= min_span <= 65535
    L = len(seq)
    segs = []
    info = dict(depth=0, best_calls=0, moved=0, n_runs=0)

    def literal(b, e):
        if e <= b:
            return
        if segs and segs[-1][1] == 0 and segs[-1][0] + segs[-1][3] == b:
            segs[-1] = (segs[-1][0], 0, 0, segs[-1][3] + e - b)
        else:
            segs.append((b, 0, 0, e - b))

    flags = 0
    if L > MAX_LEN:
        flags = TOO_LONG
        literal(0, L)
    elif L:
        c = codes(seq)
        runs = kept_runs(c, max_period, min_copies, min_span)
        info["n_runs"] = len(runs)
        cl = c.tolist() if runs else None
        x, H, stack, prev = 0, L, [], None

        def place(run, x, H, prev):
            p, a, e = run
            en, st = min(e, H), x
            if prev is not None and prev[0] == p:
                pb = prev[1]
                for t in range(x, min(x + p, en - p + 1)):
                    if cl[t:t + p] == cl[pb:pb + p]:
                        if enough((en - t) // p, p, min_copies, min_span):
                            if t != x:
                                info["moved"] += 1
                            st = t
                        break
            literal(x, st)
            k = (en - st) // p
            segs.append((st, p, k, k * p))
            return st + k * p, (p, st)

        while True:
            info["best_calls"] += 1
            b = best(runs, x, H, min_copies, min_span)
            if b is None:
                literal(x, H)
                x = H
                if not stack:
                    break
                run, H = stack.pop()
                x, prev = place(run, x, H, prev)
            elif b[2] > x:
                stack.append((b[3], H))
                info["depth"] = max(info["depth"], len(stack))
                H = b[2]
            else:
                x, prev = place(b[3], x, H, prev)
    reps = [s for s in segs if s[1]]
    return dict(segs=segs, n_segments=len(segs), n_repeats=len(reps), covered=sum(s[3] for s in reps), flags=flags, **info)


_cache = {}


def structure_cached(seq, max_period=256, min_copies=2, min_span=12):
    key = (bytes(seq), max_period, min_copies, min_span)
    if key not in _cache:
        _cache[key] = structure(*key)
    return _cache[key]


def check_invariants(seq, segs):
    """the three things that follow from the rule: the segments tile [0, L) in order, expanding them gives the allele back up to letter case,
    no two literals are adjacent"""
    seq = bytes(seq)
    pos, out, last_lit = 0, [], False
    up = seq.upper()
    for b, p, k, ln in segs:
        assert b == pos and ln > 0, (segs, pos)
        if p:
            assert ln == p * k and k >= 2
            out.append(up[b:b + p] * k)
            last_lit = False
        else:
            assert k == 0 and not last_lit, segs
            out.append(up[b:b + ln])
            last_lit = True
        pos += ln
    assert pos == len(seq) and b"".join(out) == up


def text(seq, segs):
    """the structure column of otg_repeat_emit"""
    seq = bytes(seq)
    if not segs:
        return b"."
    o = []
    for b, p, k, ln in segs:
        if p:
            o.append(b"(" + bytes(b"ACGT"[int(x)] for x in codes(seq[b:b + p])) + b")" + str(k).encode())
        else:
            o.append(seq[b:b + ln] if ln <= TEXT_LITERAL else b"[%d]" % ln)
    return b"".join(o)


def row(region, i, seq, r):
    return region + b"\t%d\t%d\t%d\t%d\t" % (i, len(seq), r["n_repeats"], r["covered"]) + text(seq, r["segs"]) + b"\n"

"""The tandem-repeat motif rule (include/otter_gpu.h) restated in plain Python / numpy from its text: byte compares on the
codes, Python integers in every comparison.  No bit-planes, no reduction trees: what tests/test_motif_host.py and tests/test_gpu_motif.py
hold the product against."""
import numpy as np

MAX_PERIOD = 4096
MAX_LEN = 1048575
TOO_LONG = 1

_CODE = np.full(256, 4, dtype=np.int64)
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_c] = _v


def motif(seq, max_period=256, slack=50):
    """-> dict(period, matches, compared, best_period, flags, unit) for one allele (bytes)"""
    assert 1 <= max_period <= MAX_PERIOD and 0 <= slack <= 999
    none = dict(period=0, matches=0, compared=0, best_period=0, flags=0, unit=b"")
    L = len(seq)
    if L > MAX_LEN:                                                      # 10
        return dict(none, flags=TOO_LONG)
    c = _CODE[np.frombuffer(seq, dtype=np.uint8)]                        # 1
    P = min(max_period, L // 2)                                          # 2
    if P == 0:
        return none
    m = [0] * (P + 1)
    for p in range(1, P + 1):                                            # 3
        a, b = c[:L - p], c[p:]
        m[p] = int(np.count_nonzero((a == b) & (a < 4)))
    best = 1
    for p in range(2, P + 1):                                            # 4
        if m[p] * (L - best) > m[best] * (L - p):
            best = p
    if m[best] == 0:                                                     # 6
        return none
    period = next(p for p in range(1, best + 1) if m[p] * (L - best) * 1000 >= (1000 - slack) * m[best] * (L - p))      # 5
    unit = bytearray()
    for j in range(period):                                              # 7
        counts = np.bincount(c[j::period], minlength=5)[:4]
        unit.append(b"ACGT"[int(np.argmax(counts))] if counts.max() > 0 else ord("N"))        # argmax: the first of equal counts
    unit = bytes(unit)
    rots = [unit[k:] + unit[:k] for k in range(period)]                  # 8
    k = min(range(period), key=lambda i: (rots[i], i))
    return dict(period=period, matches=m[period], compared=L - period, best_period=best, flags=0, unit=rots[k])          # 9


_CACHE = {}


def motif_cached(seq, max_period=256, slack=50):
    """motif(), computed once per (sequence, max_period, slack) of a test session"""
    key = (seq, max_period, slack)
    if key not in _CACHE:
        _CACHE[key] = motif(seq, max_period, slack)
    return _CACHE[key]


def row(region, i, seq, r):
    """the text row of otg_motif_emit for allele i of a record"""
    p = r["period"]
    return b"%s\t%d\t%d\t%d\t%s\t%s\t%s\n" % (region, i, len(seq), p, r["unit"] if p else b".",
                                             ("%.2f" % (len(seq) / p if p else 0.0)).encode(), ("%.4f" % (r["matches"] / r["compared"] if p else 0.0)).encode())


def same(rec, unit_row, exp):
    """does a record of abi.motif_dt with its unit slot equal the expectation?  (the slot is zero behind the unit)"""
    got = tuple(int(rec[k]) for k in ("period", "matches", "compared", "best_period", "flags", "reserved"))
    want = (exp["period"], exp["matches"], exp["compared"], exp["best_period"], exp["flags"], 0)
    u = bytes(unit_row)
    return got == want and u[:exp["period"]] == exp["unit"] and not any(u[exp["period"]:])

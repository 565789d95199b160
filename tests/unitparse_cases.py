"""Inputs of the joint unit parse shared by the CPU and the GPU tests: the table the rule was prototyped with, seeded random tasks, and the
sets that reach every lane layout of the kernel.  A task is (allele bytes, [unit bytes, ...])."""
import numpy as np

CAG, CCG = b"CAG", b"CCG"
HTT = [b"CAG", b"CAA", b"CCG", b"CCA", b"CCT"]

# (allele, unit set, (edits, switches, unit_bases), segments as (unit, begin, end, unit_bases, edits, start_phase) or None, (end_unit, end_phase))
TABLE = [
    (CAG * 20 + CCG * 20, [CAG, CCG], (0, 1, 120), [(0, 0, 60, 60, 0, 0), (1, 60, 120, 60, 0, 0)], (1, 0)),
    (CCG * 20 + CAG * 20, [CAG, CCG], (0, 1, 120), [(1, 0, 60, 60, 0, 0), (0, 60, 120, 60, 0, 0)], (0, 0)),
    (CAG * 10 + b"T" + CAG * 10 + CCG * 7, [CAG, CCG], (1, 1, 81), [(0, 0, 61, 60, 1, 0), (1, 61, 82, 21, 0, 0)], (1, 0)),
    (CAG * 10 + CCG + CAG * 10, [CAG, CCG], (0, 2, 63), [(0, 0, 30, 30, 0, 0), (1, 30, 33, 3, 0, 0), (0, 33, 63, 30, 0, 0)], (0, 0)),
    (CAG * 10 + CCG + CAG * 10, [CAG], (1, 0, 63), [(0, 0, 63, 63, 1, 0)], (0, 0)),
    (CAG * 17 + b"CAA" + CAG + CCG + b"CCA" + CCG * 7 + b"CCT" * 2, HTT, (0, 6, 90), 7, (4, 0)),
    (b"GAA" * 31 + b"AGAA" * 5 + b"GAA" * 11, [b"GAA", b"AGAA"], (0, 2, 146), [(0, 0, 93, 93, 0, 0), (1, 93, 113, 20, 0, 0), (0, 113, 146, 33, 0, 0)], (0, 0)),
    (b"AG" + CAG * 5 + b"CA", [CAG], (0, 0, 19), [(0, 0, 19, 19, 0, 1)], (0, 2)),
]


def rs(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


def tiny_set(n=300, seed=5):
    """the sizes the brute-force witness can enumerate: L <= 4, K <= 2, p <= 3, alphabet ACGN"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        units = [rs(rng, int(rng.integers(1, 4)), b"ACGN") for _ in range(int(rng.integers(1, 3)))]
        out.append((rs(rng, int(rng.integers(0, 5)), b"ACGN"), units))
    return out


def tracts(rng, units, n_tracts, max_copies, rate):
    """an allele made of tracts of the set's units, then substitutions, insertions and deletions at `rate` per base: ties between the diagonal,
    the outside base and the skip are what the edits produce"""
    s = bytearray()
    for _ in range(n_tracts):
        u = units[int(rng.integers(0, len(units)))]
        s += u * int(rng.integers(1, max_copies + 1))
    out = bytearray()
    for b in s:
        x = rng.random()
        if x < rate / 3:
            continue                                                   # a deletion
        if x < 2 * rate / 3:
            out.append(b"ACGT"[int(rng.integers(0, 4))])               # a substitution (or the same base)
            continue
        if x < rate:
            out.append(b"ACGTN"[int(rng.integers(0, 5))])              # an insertion
        out.append(b)
    return bytes(out)


def random_set(n=300, seed=9, max_len=40, max_units=3):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        units = [rs(rng, int(rng.integers(1, 7)), b"ACGT" if rng.random() < 0.8 else b"ACGN") for _ in range(int(rng.integers(1, max_units + 1)))]
        if rng.random() < 0.2:
            units.append(units[0])                                     # a duplicate: the lower index wins
        if rng.random() < 0.3:
            s = rs(rng, int(rng.integers(0, max_len + 1)), b"ACGTN")
        else:
            s = tracts(rng, units, int(rng.integers(1, 5)), 5, 0.15)[:max_len]
        if rng.random() < 0.2:
            s = s.lower()
        out.append((s, units[:max_units + 1]))
    return out


# unit lengths per set -> (lanes, positions per lane): every width 4 .. 64 at one position per lane, then two and four
LAYOUTS = [
    ([3], 4, 1), ([2, 2], 4, 1), ([3, 3], 8, 1), ([3, 5], 8, 1), ([3, 5, 7], 16, 1), ([4, 4, 4, 4], 16, 1), ([1] * 8, 8, 1),
    ([10, 10], 32, 1),                 # the second unit lies across lane 16
    ([3, 3, 3, 3, 3], 16, 1), ([29, 3], 32, 1),
    ([20, 20], 64, 1),                 # the second unit lies across lane 32
    ([13, 30, 21], 64, 1), ([7, 9, 5, 3, 11, 2, 13, 6], 64, 1), ([64], 64, 1),
    ([65], 64, 2), ([40, 41], 64, 2), ([33, 30, 25, 17], 64, 2), ([128], 64, 2),
    ([129], 64, 4), ([256], 64, 4), ([100, 60, 37, 5, 3], 64, 4), ([31, 31, 31, 31, 31, 31, 31, 32], 64, 4),
]
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 33, 64, 100, 177, 300]


def layout_set(seed=21):
    """per layout: alleles of every length of LENGTHS (tracts with edits, cut), one random allele, one with N and lower case"""
    rng = np.random.default_rng(seed)
    out = []
    for lens, _, _ in LAYOUTS:
        units = [rs(rng, p) for p in lens]
        if len(lens) > 1 and lens[0] == lens[1]:
            units[1] = units[0]                                        # duplicate units in a set
        pick = [LENGTHS[i] for i in rng.permutation(len(LENGTHS))[:5]] + [300]
        for L in pick:
            s = b""
            while len(s) < L:
                s += tracts(rng, units, 3, max(1, 40 // max(lens)), 0.08)
            out.append((s[:L], units))
        out.append((rs(rng, 50, b"ACGTN"), units))
        noisy = [bytes(u).lower() if k % 2 else u for k, u in enumerate(units)]
        if len(lens[0:1]) and lens[0] > 2:
            noisy[0] = noisy[0][:1] + b"N" + noisy[0][2:]
        out.append((tracts(rng, noisy, 3, 3, 0.1)[:120].swapcase(), noisy))
    return out


def shared_wave_set(seed=33):
    """tasks of different L and different K in one class: sixteen, eight, four neighbours in a wave that end at different rows"""
    rng = np.random.default_rng(seed)
    out = []
    for sets in ([[CAG], [CAG, b"C"], [b"AT", b"GC"], [b"ACGT"]], [[CAG, CCG], HTT, [b"AAAAG", b"AG"], [b"CAGCAGC"]], [HTT + [b"GAA", b"AGAA"], [b"ACGTACGTAC", b"TTAGGG"]]):
        for i in range(40):
            units = sets[i % len(sets)]
            out.append((tracts(rng, units, 4, 6, 0.1)[:int(rng.integers(1, 90))], units))
    return out


def pack(tasks):
    """tasks -> (seqs, unit_sets, task_seq, task_set) with every allele and every distinct set stored once"""
    seqs, sets, ts, tq = [], [], [], []
    si, qi = {}, {}
    for s, units in tasks:
        key = tuple(units)
        if s not in si:
            si[s] = len(seqs); seqs.append(s)
        if key not in qi:
            qi[key] = len(sets); sets.append(list(units))
        ts.append(si[s]); tq.append(qi[key])
    return seqs, sets, ts, tq


def check(got_rec, got_segs, want):
    """a result of the library (a unitparse_sum_dt record, its unitparse_seg_dt rows) against (record, segments) of unitparse_ref"""
    rec, segs = want
    assert tuple(int(got_rec[f]) for f in ("edits", "switches", "unit_bases", "n_segments", "end_unit", "end_phase", "flags")) == rec and int(got_rec["reserved"]) == 0
    assert [tuple(int(x) for x in g) for g in got_segs] == segs

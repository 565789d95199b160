"""The allele sets of the repeat-structure tests beyond tests/motif_cases.py: the hand-derived table, the word and carry edges of the run
walk, and an allele whose parse nests its horizons.  tests/test_repeat_host.py runs them through the reference and the host harness,
tests/test_gpu_repeat.py on the device."""
import numpy as np
import motif_cases as Cs

# (allele, segments (begin, period, copies, length), structure text) at the defaults 256 / 2 / 12
TABLE = [
    (b"CAG" * 20 + b"CCG" * 20, [(0, 3, 20, 60), (60, 3, 20, 60)], b"(CAG)20(CCG)20"),
    (b"CAG" * 10 + b"CTG" + b"CAG" * 9, [(0, 3, 10, 30), (30, 0, 0, 3), (33, 3, 9, 27)], b"(CAG)10CTG(CAG)9"),
    (b"CAG" * 10 + b"T" + b"CAG" * 10, [(0, 3, 10, 30), (30, 0, 0, 1), (31, 3, 10, 30)], b"(CAG)10T(CAG)10"),
    (b"CGG" * 10 + b"AGG" + b"CGG" * 9 + b"AGG" + b"CGG" * 20, [(0, 3, 10, 30), (30, 0, 0, 3), (33, 3, 9, 27), (60, 0, 0, 3), (63, 3, 20, 60)],
     b"(CGG)10AGG(CGG)9AGG(CGG)20"),
    (b"CAG" * 20 + b"CAACAG" + b"CCGCCA" + b"CCG" * 10, [(0, 3, 20, 60), (60, 0, 0, 12), (72, 3, 10, 30)], b"(CAG)20CAACAGCCGCCA(CCG)10"),
    (b"AC" * 40 + b"N" * 7 + b"AC" * 40, [(0, 2, 40, 80), (80, 0, 0, 7), (87, 2, 40, 80)], b"(AC)40NNNNNNN(AC)40"),
    (b"T" * 12 + b"GATTACAG" + b"CAG" * 100, [(0, 1, 12, 12), (12, 0, 0, 5), (17, 3, 101, 303)], b"(T)12GATTA(CAG)101"),
    (b"GAA" * 30 + b"GAAA" * 5 + b"GAA" * 12, [(0, 3, 31, 93), (93, 4, 5, 20), (113, 3, 11, 33)], b"(GAA)31(AGAA)5(GAA)11"),
    (b"ACGT" * 2 + b"T" * 11 + b"ACGT" * 3, [(0, 0, 0, 7), (7, 1, 12, 12), (19, 4, 3, 12)], b"ACGTACG(T)12(ACGT)3"),
    (b"A" * 30, [(0, 1, 30, 30)], b"(A)30"),
    (b"ACAC", [(0, 0, 0, 4)], b"ACAC"),
    (b"N" * 20, [(0, 0, 0, 20)], b"NNNNNNNNNNNNNNNNNNNN"),
    (b"", [], b"."),
]

PARAM_SETS = [(256, 2, 12), (1, 2, 2), (2, 2, 2), (64, 2, 2), (256, 3, 20), (4096, 2, 12)]
EDGE_PERIODS = (1, 2, 63, 64, 65)
EDGE_ENOUGH = ((2, 2), (3, 20), (5, 40))


def word_edge_set(seed=23):
    """runs of the match bits that start or end on bit 31, 32 or 33, span three words, reach L - p exactly; units next to 32 and 64 bases;
    an N at a word boundary inside a run"""
    rng = np.random.default_rng(seed)
    out = [b"T" * 64, b"T" * 65, b"G" * 31 + b"T" + b"G" * 32]
    for start in (31, 32, 33):                                             # a homopolymer and a 3-base repeat that begin on these bits ...
        for end in (31, 32, 33, 63, 64, 65, 95, 96, 97, 130):              # ... and whose bits end on these (e_1 ends at end - 1, e_3 at end - 3)
            if end > start + 1:
                out.append(b"CA" * (start // 2) + b"C" * (start % 2) + b"T" * (end - start) + b"GA" * 9)
            if end > start + 8:
                body = (b"GTT" * 50)[:end - start]
                out.append(Cs.rs(rng, start, b"AC") + body + Cs.rs(rng, 11, b"AC"))
    out.append(Cs.rs(rng, 9, b"AC") + b"GTT" * 40)                        # reaches L - p exactly, three words and more
    out.append(Cs.rs(rng, 30, b"AC") + b"G" * 70)                         # bits 30 .. 98 at p = 1: three words, open behind the last one
    out.append(b"G" * 100)
    for u in (31, 32, 33, 63, 64, 65):
        unit = Cs.rs(rng, u)
        for copies in (2, 3, 5):
            out.append(unit * copies)
            out.append(Cs.rs(rng, 5) + unit * copies + Cs.rs(rng, 3))
    base = b"ACGGT" * 30
    for pos in (31, 32, 33, 63, 64, 65, 95, 96):
        s = bytearray(base); s[pos] = ord("N"); out.append(bytes(s))
        s = bytearray(b"T" * 130); s[pos] = ord("n"); out.append(bytes(s))
    return out


def deep_stack():
    """stronger runs further right, each beating everything in front of it from x = 0: best() picks the last, then under its start the one
    before it, and so on; the first run begins behind one literal base, so it is pushed too"""
    return b"C" + b"A" * 12 + b"C" + b"G" * 84 + b"T" + b"C" * 560 + b"A" + b"T" * 4500


def as_tuples(sums, seg_off, segs, i):
    """segments of allele i of a (sums, seg_off, segs) result as the reference's tuples"""
    a, b = int(seg_off[i]), int(seg_off[i + 1])
    return [(int(g["begin"]), int(g["period"]), int(g["copies"]), int(g["length"])) for g in segs[a:b]]

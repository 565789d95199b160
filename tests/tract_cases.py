"""The (allele, unit) sets of the tract-mode tests, generated from fixed seeds: tests/test_tract_host.py runs them through the references and
the host harness, tests/test_gpu_tract.py and tests/tract_switch_child.py on the device.  The generators of unitalign_cases are reused and
given flanks; the shapes are those at which the lane layout can go wrong, plus tract starts and ends on both sides of a 16-byte load."""
import numpy as np
import motif_cases as Cs
import unitalign_cases as Uc

# the values the rule was prototyped with at the default scores: (allele, unit, (score, begin, end, edits, unit_bases, end_phase) | None)
TABLE = [
    (b"GATTACA" + b"CAG" * 20 + b"TTGACCA", b"CAG", (120, 7, 67, 0, 60, 0)),
    (b"GATTACA" + b"CAG" * 10 + b"T" + b"CAG" * 10 + b"TTGACCA", b"CAG", (113, 7, 68, 1, 60, 0)),
    (b"GATTACA" + b"CAG" * 10 + b"CTG" + b"CAG" * 9 + b"TTGACCA", b"CAG", (111, 7, 67, 1, 60, 0)),
    (b"CAG" * 20 + b"CCG" * 20, b"CAG", (122, 0, 61, 0, 61, 1)),
    (b"CAG" * 20 + b"CCG" * 20, b"CCG", (122, 59, 120, 0, 61, 0)),
    (b"TT" + b"GAA" * 31 + b"AGAA" * 5 + b"GAA" * 11 + b"CC", b"GAA", (247, 2, 148, 5, 141, 0)),
    (b"NNNN" + b"CAG" * 4 + b"NN", b"CAG", (24, 4, 16, 0, 12, 0)),
    (b"TTT" + b"CAG" * 3 + b"TTT", b"CAG", 18),            # none at min_score 24; [3, 12) at 0
    (b"ACGTTGCA" * 3, b"CAG", 6),                          # none
]
GLOBAL = [(9, 69), (10, 69), (10, 69), (20, 120), (20, 119), (9, 141)]      # what the global unit alignment gives for rows 1-6

EDGE_P = Uc.EDGE_P
SCORES = ((2, 7, 7), (1, 1, 1), (3, 2, 5))


def tiny_set(seed=43, n=360):
    """a short noisy repeat between 0-3 random flank bases: p <= 7, L <= 14 over ACGTN, small enough for the brute-force witness"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = int(rng.integers(1, 8))
        unit = Cs.rs(rng, p, b"ACGTN" if len(out) % 6 == 0 else b"ACGT")
        core = Uc.indels(rng, Uc.repeat_from(unit, int(rng.integers(0, p)), int(rng.integers(0, 11))), 0.06, 0.06)
        s = Cs.rs(rng, int(rng.integers(0, 4)), b"ACGTN") + core + Cs.rs(rng, int(rng.integers(0, 4)), b"ACGTN")
        if len(s) <= 14:
            out.append((s, unit))
    return out


def flanked(rng, core, left, right):
    return Cs.rs(rng, left) + core + Cs.rs(rng, right)


def edge_set(seed=47):
    rng = np.random.default_rng(seed)
    out = [(s, u) for s, u, _ in TABLE]
    for p in EDGE_P:
        unit = Cs.rs(rng, p)
        copies = 5 if p <= 64 else 3
        whole = unit * copies
        for left in (0, 1, 15, 16, 17):                                     # tract starts and ends on both sides of a 16-byte load
            right = (17, 16, 0, 1, 15)[(left + p) % 5]
            out.append((flanked(rng, Uc.repeat_from(unit, int(rng.integers(0, p)), copies * p + int(rng.integers(0, p))), left, right), unit))
        out.append((Uc.repeat_from(unit, int(rng.integers(0, p)), p - 1), unit))      # L < p
        out.append((flanked(rng, Uc.repeat_from(unit, 1 % p, max(p - 1, 1)), 3, 2), unit))
        for c in (0, copies // 2, copies - 1):                              # one edit in the first, a middle and the last copy
            at = c * p + int(rng.integers(0, p))
            k = int(rng.integers(0, 4))
            sub = bytearray(whole)
            sub[at] = b"ACGT"[(b"ACGT".index(whole[at:at + 1]) + 1 + int(rng.integers(0, 3))) % 4]
            for core in (whole[:at] + b"ACGT"[k:k + 1] + whole[at:], whole[:at] + whole[at + 1:], bytes(sub)):
                out.append((flanked(rng, core, int(rng.integers(0, 20)), int(rng.integers(0, 20))), unit))
        n_al = bytearray(whole); n_al[len(whole) // 2] = ord("N")
        n_un = bytearray(unit); n_un[p // 2] = ord("n")
        out += [(flanked(rng, bytes(n_al), 5, 6), unit), (flanked(rng, whole, 4, 18), bytes(n_un)), (b"NNN" + whole.lower() + b"NN", unit),
                (whole, unit.lower())]
        out.append((Cs.rs(rng, 2 * p + 3), unit))                           # unrelated sequence
    return out


def random_set(seed=53, n=300):
    """noisy repeats of units of 1-40 bases, rotated, 0-300 bases, between flanks of 0-30 random bases"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p = int(rng.integers(1, 41)) if i % 3 else int(rng.integers(1, 8))
        unit = Cs.rs(rng, p, b"ACGTN" if i % 5 == 0 else b"ACGT")
        core = Uc.indels(rng, Uc.repeat_from(unit, int(rng.integers(0, p)), int(rng.integers(0, 301))), 0.04, 0.04)
        out.append((Cs.rs(rng, int(rng.integers(0, 31)), b"ACGTN") + core + Cs.rs(rng, int(rng.integers(0, 31))), unit))
    return out


def one_wave_batch(p, seed=59):
    """sixteen tasks of one unit length whose alleles have 0, 1, 2, 5, 3 000 and eleven times about 60 bases, flanked, in shuffled order"""
    rng = np.random.default_rng(seed + p)
    unit = Cs.rs(rng, p)
    lens = [0, 1, 2, 5, 3000] + [int(x) for x in rng.integers(40, 56, 11)]
    pairs = []
    for L in lens:
        if L <= 5:
            pairs.append((Uc.repeat_from(unit, 1 % p, L), unit))
        else:
            core = Uc.indels(rng, Uc.repeat_from(unit, int(rng.integers(0, p)), L), 0.03, 0.03)
            pairs.append((flanked(rng, core, int(rng.integers(0, 8)), int(rng.integers(0, 8))), unit))
    return [pairs[i] for i in rng.permutation(len(pairs))]


def bound_set(p, L, seed=61):
    """three alleles of exactly L bases for the narrow bound: a pure repeat (the largest score), a repeat behind a long flank (the largest
    begin), a noisy one"""
    rng = np.random.default_rng(seed + p)
    unit = Cs.rs(rng, p)
    noisy = Uc.indels(rng, Uc.repeat_from(unit, 3 % p, L + L // 8 + 16), 0.02, 0.02)[:L - 40]
    return [(Uc.repeat_from(unit, 5 % p, L), unit), (b"N" * (L - 3 * p) + unit * 3, unit), (Cs.rs(rng, 20) + noisy + Cs.rs(rng, 20), unit)]


pack = Uc.pack

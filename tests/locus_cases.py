"""The (allele, unit set) tasks of the locus-mode tests, generated from fixed seeds: tests/test_locus_host.py runs them through the references
and the host harness, tests/test_gpu_locus.py and tests/locus_switch_child.py on the device.  The generators of tract_cases and
unitparse_cases are reused: repeats of a set's units with edits, between flanks, rotated, with N bytes."""
import numpy as np
import motif_cases as Cs
import tract_cases as Tc
import unitalign_cases as Uc
import unitparse_cases as Pc

CAG, CCG = Pc.CAG, Pc.CCG
HTT = Pc.HTT
L5, R5 = b"GATTACA", b"TTGACCA"

# the values the rule was prototyped with at the default scores:
# (allele, set, (score, begin, end, edits, switches, unit_bases), [(unit, begin, end) of the segments])
TABLE = [
    (L5 + CAG * 20 + CCG * 7 + R5, [CAG, CCG], (162, 7, 88, 0, 1, 81), [(0, 7, 67), (1, 67, 88)]),
    (L5 + CAG * 10 + b"T" + CAG * 10 + CCG * 7 + R5, [CAG, CCG], (155, 7, 89, 1, 1, 81), [(0, 7, 68), (1, 68, 89)]),
    (L5 + CAG * 10 + CCG + CAG * 10 + R5, [CAG, CCG], (126, 7, 70, 0, 2, 63), [(0, 7, 37), (1, 37, 40), (0, 40, 70)]),
    (b"TT" + b"GAA" * 31 + b"AGAA" * 5 + b"GAA" * 11 + b"CC", [b"GAA", b"AGAA"], (292, 2, 148, 0, 2, 146), [(0, 2, 95), (1, 95, 115), (0, 115, 148)]),
    (b"TTT" + CAG * 2 + CCG * 2 + b"TTT", [CAG, CCG], (24, 3, 15, 0, 1, 12), [(0, 3, 9), (1, 9, 15)]),
    (L5 + CAG * 20 + R5, [CAG], (120, 7, 67, 0, 0, 60), [(0, 7, 67)]),
    (CAG * 20 + b"ACGTTGCATTGACA" + CCG * 20, [CAG, CCG], (207, 0, 134, 7, 3, 132), None),
]
# what the tools before this one give for the first row: the global parse (edits, unit_bases), the tracts of either unit alone
WHY = {"unitparse": (9, 90), "tract_CAG": (7, 68, 61), "tract_CCG": (66, 88, 44, 22)}

SCORES = Tc.SCORES
# unit lengths that reach every class at the smallest shapes: (lengths, class)
CLASS_SETS = [([3], 0), ([3, 5], 1), ([3, 3, 3, 3, 3], 2), ([7, 13], 3), ([29, 30], 4), ([40, 50], 5), ([256], 6), ([128, 100], 6),
              ([1, 2, 3, 4, 5, 6, 7, 8], 4)]


def tiny_set(seed=71, n=240):
    """the sizes the brute-force witness enumerates: K <= 2, p <= 3, L <= 8 over ACGTN; a short noisy repeat of the set between flanks"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        units = [Cs.rs(rng, int(rng.integers(1, 4)), b"ACGTN" if len(out) % 7 == 0 else b"ACGT") for _ in range(int(rng.integers(1, 3)))]
        core = Pc.tracts(rng, units, int(rng.integers(1, 3)), 2, 0.12)
        s = Cs.rs(rng, int(rng.integers(0, 3)), b"ACGTN") + core + Cs.rs(rng, int(rng.integers(0, 3)), b"ACGTN")
        if len(s) <= 8:
            out.append((s, units))
    return out


def flanked_tracts(rng, units, n_tracts, max_copies, rate, left, right):
    return Cs.rs(rng, left, b"ACGTN") + Pc.tracts(rng, units, n_tracts, max_copies, rate) + Cs.rs(rng, right)


def random_set(seed=73, n=200, max_p=12):
    """noisy tracts of 1-3 units of 1-max_p bases between flanks of 0-30 bases"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        units = [Cs.rs(rng, int(rng.integers(2, max_p + 1)), b"ACGTN" if i % 6 == 0 else b"ACGT") for _ in range(1 + i % 3)]
        s = flanked_tracts(rng, units, int(rng.integers(1, 5)), 6, 0.04, int(rng.integers(0, 31)), int(rng.integers(0, 31)))
        if i % 11 == 0:
            s = Cs.rs(rng, int(rng.integers(0, 60)), b"ACGTN")              # unrelated sequence
        out.append((s.lower() if i % 9 == 0 else s, units))
    return out


END_AT = (17, 16, 0, 1, 15)


def _unlike(flank, at, base):
    """the flank with its base next to the tract made to differ from the unit base that would extend the tract"""
    if not flank:
        return flank
    f = bytearray(flank)
    if f[at] == base[0]:
        f[at] = b"ACGT"[(b"ACGT".index(base) + 1) % 4]
    return bytes(f)


def edge_set(seed=79):
    """per class set: tracts that begin and end at 0, 1, 15, 16, 17 from a 16-byte load, one substitution, insertion and deletion per unit, an
    interruption that is a unit of the set, N in the allele and in a unit, L < p, unrelated sequence, L = 0"""
    rng = np.random.default_rng(seed)
    out = [(s, u) for s, u, _, _ in TABLE]
    for lens, _ in CLASS_SETS:
        units = [Cs.rs(rng, p) for p in lens]
        copies = 4 if max(lens) <= 64 else 2
        whole = b"".join(u * copies for u in units)
        for i, left in enumerate((0, 1, 15, 16, 17)):                       # the tract begins at `left` and ends at END_AT[i] from a 16-byte load
            r = int(rng.integers(0, lens[0]))
            core = Uc.repeat_from(units[0], r, copies * lens[0] - r) + b"".join(u * copies for u in units[1:])
            core += Uc.repeat_from(units[-1], 0, (END_AT[i] - left - len(core)) % 16)
            out.append((_unlike(Cs.rs(rng, left), -1, units[0][r - 1:r] or units[0][-1:]) + core +
                        _unlike(Cs.rs(rng, END_AT[(i + 2) % 5]), 0, Uc.repeat_from(units[-1], len(core) - sum(lens[:-1]) * copies, 1)), units))
        for k, u in enumerate(units):                                       # one substitution, insertion and deletion in unit k's tract
            at = sum(copies * p for p in lens[:k]) + len(u) + int(rng.integers(0, len(u)))
            sub = bytearray(whole)
            sub[at] = b"ACGT"[(b"ACGT".index(whole[at:at + 1]) + 1 + int(rng.integers(0, 3))) % 4]
            x = int(rng.integers(0, 4))
            for core in (bytes(sub), whole[:at] + b"ACGT"[x:x + 1] + whole[at:], whole[:at] + whole[at + 1:]):
                out.append((Tc.flanked(rng, core, int(rng.integers(0, 20)), int(rng.integers(0, 20))), units))
        out.append((Tc.flanked(rng, units[0] * copies + units[-1] + units[0] * copies, 5, 6), units))      # an interruption that is a unit of the set
        n_al = bytearray(whole); n_al[len(whole) // 2] = ord("N")
        n_un = [bytearray(u) for u in units]; n_un[-1][lens[-1] // 2] = ord("n")
        out += [(Tc.flanked(rng, bytes(n_al), 5, 6), units), (Tc.flanked(rng, whole, 4, 18), [bytes(u) for u in n_un]), (b"NNN" + whole.lower() + b"NN", units),
                (units[0][:lens[0] - 1], units), (Cs.rs(rng, 2 * max(lens) + 3), units), (b"", units)]
    return out


def one_wave_batch(units, seed=83):
    """sixteen tasks of one set whose alleles have 0, 1, 2, 5, 3 000 and eleven times about 60 bases, flanked, in shuffled order"""
    rng = np.random.default_rng(seed + sum(len(u) for u in units))
    out = []
    for L in [0, 1, 2, 5, 3000] + [int(x) for x in rng.integers(40, 56, 11)]:
        if L <= 5:
            out.append((Uc.repeat_from(units[0], 1 % len(units[0]), L), units))
            continue
        core = b""
        while len(core) < L:
            core += Pc.tracts(rng, units, 3, 8, 0.03)
        out.append((Tc.flanked(rng, core[:L], int(rng.integers(0, 8)), int(rng.integers(0, 8))), units))
    return [out[i] for i in rng.permutation(len(out))]


def bound_set(p, L, seed=89):
    """three alleles of exactly L bases for the narrow bound of a set {3, p}: a pure repeat of the long unit (the largest score), a repeat
    behind a long flank (the largest begin), noisy tracts of both"""
    rng = np.random.default_rng(seed + p)
    units = [b"CAG", Cs.rs(rng, p)] if p < 200 else [Cs.rs(rng, p)]
    noisy = b""
    while len(noisy) < L - 40:
        noisy += Pc.tracts(rng, units, 4, 12, 0.02)
    return [(Uc.repeat_from(units[-1], 5 % p, L), units), (b"N" * (L - 3 * p) + units[-1] * 3, units),
            (Cs.rs(rng, 20) + noisy[:L - 40] + Cs.rs(rng, 20), units)]


pack = Pc.pack


def check(got_rec, got_segs, want):
    """a result of the library (a locus_dt record, its unitparse_seg_dt rows) against (record, segments) of locus_ref"""
    rec, segs = want
    assert tuple(int(x) for x in got_rec) == rec, (tuple(int(x) for x in got_rec), rec)
    assert [tuple(int(x) for x in g) for g in got_segs] == segs

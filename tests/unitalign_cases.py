"""The (allele, unit) sets of the unit-alignment tests, generated from fixed seeds: tests/test_unitalign_host.py runs them through the
references and the host harness, tests/test_gpu_unitalign.py on the device.  Shapes chosen where the lane layout can go wrong: every
segment class and its neighbours, units that do not fill their segment, alleles shorter than the unit, edits in the first and last copy."""
import numpy as np
import motif_cases as Cs

# the values the rule was prototyped with, (allele, unit, (edits, unit_bases, end_phase))
TABLE = [
    (b"CAG" * 20, b"CAG", (0, 60, 0)),
    (b"CAG" * 10 + b"CTG" + b"CAG" * 9, b"CAG", (1, 60, 0)),
    (b"CAG" * 10 + b"T" + b"CAG" * 10, b"CAG", (1, 60, 0)),
    (b"CAG" * 10 + b"CG" + b"CAG" * 9, b"AGC", (1, 60, 2)),
    (b"CAG" * 20 + b"CCG" * 20, b"CAG", (20, 120, 0)),
    (b"CAG" * 20 + b"CCG" * 20, b"CCG", (20, 119, 0)),
    (b"GCAGCAGCA", b"CAG", (0, 9, 2)),
    (b"A", b"CAG", (0, 1, 2)),
    (b"NNN", b"N", (3, 0, 0)),
    (b"acgt", b"ACGTACGTAC", (0, 4, 4)),
    (b"", b"CAG", (0, 0, 0)),
]

EDGE_P = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 255, 256)


def tiny_set(seed=19, n=400):
    """p <= 7, L <= 14 over ACGTN: small enough for the brute-force form of step 2"""
    rng = np.random.default_rng(seed)
    return [(Cs.rs(rng, int(rng.integers(0, 15)), b"ACGTN"), Cs.rs(rng, int(rng.integers(1, 8)), b"ACGTN")) for _ in range(n)]


def indels(rng, seq, dele, ins):
    """every base deleted with probability dele, a random base inserted behind it with probability ins"""
    out = bytearray()
    for b in seq:
        if rng.random() >= dele:
            out.append(b)
        if rng.random() < ins:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
    return bytes(out)


def repeat_from(unit, phase, L):
    p = len(unit)
    return bytes(unit[(phase + i) % p] for i in range(L))


def edge_set(seed=29):
    rng = np.random.default_rng(seed)
    out = [(s, u) for s, u, _ in TABLE]
    for p in EDGE_P:
        unit = Cs.rs(rng, p)
        for L in (0, 1, p - 1, p, p + 1, 3 * p + 1, 200):                   # L < p: a unit longer than the allele
            out.append((repeat_from(unit, int(rng.integers(0, p)), L), unit))
        if p <= 5:
            out += [(repeat_from(unit, ph, 4 * p + 2), unit) for ph in range(p)]
        copies = 5 if p <= 64 else 3
        whole = unit * copies
        for c in (0, copies // 2, copies - 1):                              # one edit in the first, a middle and the last copy
            at = c * p + int(rng.integers(0, p))
            k = int(rng.integers(0, 4))
            out.append((whole[:at] + b"ACGT"[k:k + 1] + whole[at:], unit))
            out.append((whole[:at] + whole[at + 1:], unit))
            sub = bytearray(whole)
            sub[at] = b"ACGT"[(b"ACGT".index(whole[at:at + 1]) + 1 + int(rng.integers(0, 3))) % 4]
            out.append((bytes(sub), unit))
        n_al = bytearray(whole); n_al[len(whole) // 2] = ord("N")
        n_un = bytearray(unit); n_un[p // 2] = ord("n")
        out += [(bytes(n_al), unit), (whole, bytes(n_un)), (bytes(n_al), bytes(n_un)), (whole.lower(), unit), (whole, unit.lower())]
        out.append((Cs.rs(rng, 2 * p + 3), unit))                           # unrelated sequence
    one = Cs.rs(rng, 7) * 9 + b"ACG"                                         # one allele against several units
    out += [(one, one[:7]), (one, one[3:10]), (one, b"A"), (one, Cs.rs(rng, 40)), (one, one[:14]), (one, b"NNNN")]
    return out


def random_set(seed=31, n=300):
    """noisy repeats of units of 1-40 bases over ACGTN, the unit rotated, alleles of 0-300 bases"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p = int(rng.integers(1, 41)) if i % 3 else int(rng.integers(1, 8))
        unit = Cs.rs(rng, p, b"ACGTN" if i % 5 == 0 else b"ACGT")
        L = int(rng.integers(0, 301))
        s = indels(rng, repeat_from(unit, int(rng.integers(0, p)), L), 0.05, 0.05)
        if i % 7 == 0:
            s = Cs.rs(rng, int(rng.integers(0, 6)), b"ACGTN") + s + Cs.rs(rng, int(rng.integers(0, 6)))      # flanks
        out.append((s, unit))
    return out


def one_wave_batch(p, seed=37):
    """sixteen tasks of one unit length whose alleles have 0, 1, 2, 5, 3 000 and eleven times about 60 bases, in shuffled order"""
    rng = np.random.default_rng(seed + p)
    unit = Cs.rs(rng, p)
    lens = [0, 1, 2, 5, 3000] + [int(x) for x in rng.integers(55, 66, 11)]
    pairs = [(indels(rng, repeat_from(unit, int(rng.integers(0, p)), L), 0.03, 0.03) if L > 5 else repeat_from(unit, 1 % p, L), unit) for L in lens]
    return [pairs[i] for i in rng.permutation(len(pairs))]


def noisy_repeat(p, L, seed):
    """a repeat of a random p-base unit with 5 % deletions and 5 % insertions, cut or padded to exactly L bases"""
    rng = np.random.default_rng(seed)
    unit = Cs.rs(rng, p)
    s = indels(rng, repeat_from(unit, 0, L + L // 8 + 16), 0.05, 0.05)
    assert len(s) >= L
    return s[:L], unit


def pack(pairs):
    """(alleles, units, task_seq, task_unit) of a list of pairs, equal alleles and equal units stored once"""
    seqs, units, si, ui, ts, tu = [], [], {}, {}, [], []
    for s, u in pairs:
        if s not in si:
            si[s] = len(seqs); seqs.append(s)
        if u not in ui:
            ui[u] = len(units); units.append(u)
        ts.append(si[s]); tu.append(ui[u])
    return seqs, units, np.array(ts, dtype=np.uint32), np.array(tu, dtype=np.uint32)

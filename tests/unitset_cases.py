"""Inputs of the unit-set tests, shared by the host and the GPU files: the seven prototype groups of the rule with the rows DESIGN_LOG.md
records, random groups, the planted loci of the recovery property and the cases that sit on a threshold."""
import random

F, G = b"GATTACA", b"TTGACCA"


def _e(n, m):
    return F + b"CAG" * n + b"CAACAG" + b"CCGCCA" + b"CCG" * m + b"CCT" * 2 + G


# name -> (alleles, [(unit, weight, segments)], n_classes, [locus record (score, begin, end, edits, switches, unit_bases) per allele])
PROTOTYPES = {
    "A": ([F + b"CAG" * 20 + b"CCG" * 7 + G, F + b"CAG" * 10 + b"T" + b"CAG" * 10 + b"CCG" * 9 + G],
          [(b"CAG", 120, 3), (b"CCG", 48, 2)], 2, [(162, 7, 88, 0, 1, 81), (167, 7, 95, 1, 1, 87)]),
    "B": ([F + b"GAA" * 31 + b"AGAA" * 5 + b"GAA" * 11 + G, F + b"GAA" * 9 + G],
          [(b"AGA", 153, 3), (b"AAGA", 20, 1)], 2, [(294, 6, 153, 0, 2, 147), (56, 6, 34, 0, 0, 28)]),
    "C": ([b"TTTT" + b"CAG" * 12 + b"TTTT", b"GGA" + b"AGC" * 30 + b"TCT", b"AC" + b"GCA" * 8 + b"TT"],
          [(b"AGC", 150, 3)], 1, [(72, 4, 40, 0, 0, 36), (180, 3, 93, 0, 0, 90), (48, 2, 26, 0, 0, 24)]),
    "D": ([b"CAG" * 20 + b"ACGTTGCATTGACA" + b"CCG" * 20],
          [(b"CAG", 60, 1), (b"CCG", 60, 1)], 2, [(207, 0, 134, 7, 3, 132)]),
    "E": ([_e(17, 7), _e(20, 10), _e(42, 7), _e(19, 9)],
          [(b"CAG", 294, 4), (b"CCG", 99, 4)], 2,
          [(154, 7, 93, 2, 1, 86), (190, 7, 111, 2, 1, 104), (304, 7, 168, 2, 1, 161), (178, 7, 105, 2, 1, 98)]),
    "F": ([F + b"ACGTTGCA" + G, b""], [], 0, []),
    "G": ([F + b"ACGGTCATTG" * 6 + G, F + b"ACGGTCATTC" * 3 + G, F + b"ACGGTCATT" * 4 + G],
          [(b"ACGGTCATTG", 60, 1)], 3, [(120, 7, 67, 0, 0, 60), (40, 7, 36, 2, 0, 29), (51, 7, 43, 3, 0, 39)]),
}


def flat(groups):
    """groups (lists of alleles) -> (alleles, group_first)"""
    alleles, first = [], [0]
    for g in groups:
        alleles.extend(g)
        first.append(len(alleles))
    return alleles, first


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def primitive_unit(rng, p):
    while True:
        u = rand_seq(rng, p)
        if not any(p % d == 0 and u == u[:d] * (p // d) for d in range(1, p)):
            return u


def noisy(rng, s, rate):
    """per-base errors at `rate`, split evenly between deletion, insertion and substitution"""
    out = bytearray()
    for ch in s:
        if rng.random() < rate:
            kind = rng.randrange(3)
            if kind == 0:
                continue
            if kind == 1:
                out.append(rng.choice(b"ACGT")); out.append(ch)
            else:
                out.append(rng.choice([x for x in b"ACGT" if x != ch]))
        else:
            out.append(ch)
    return bytes(out)


def random_allele(rng, units, max_copies=12, rate=0.02, lower=0.0):
    """flank, a few runs over the group's units (any rotation), a spacer now and then, flank"""
    s = bytearray(rand_seq(rng, rng.randrange(0, 12)))
    for _ in range(rng.randrange(1, 4)):
        u = rng.choice(units)
        r = rng.randrange(len(u))
        s += (u[r:] + u[:r]) * rng.randrange(2, max_copies + 1)
        if rng.random() < 0.3:
            s += rand_seq(rng, rng.randrange(1, 6))
    s += rand_seq(rng, rng.randrange(0, 12))
    s = noisy(rng, bytes(s), rate)
    if lower and rng.random() < lower:
        s = s.lower()
    if rng.random() < 0.05:
        s = s[:len(s) // 2] + b"N" + s[len(s) // 2:]
    return s


def random_group(rng, size, n_units=None, p_max=9, **kw):
    units = [primitive_unit(rng, rng.randrange(1, p_max + 1)) for _ in range(n_units or rng.randrange(1, 4))]
    return [random_allele(rng, units, **kw) for _ in range(size)]


def planted_locus(rng, rate):
    """the recovery property: 1-3 distinct primitive units of 2-12 bases, four alleles, 6-30 copies per unit, flanks of 5-40 bases
    -> (alleles, the planted units)"""
    units, n_units = [], rng.randrange(1, 4)
    while len(units) < n_units:
        u = primitive_unit(rng, rng.randrange(2, 13))
        if all(len(u) != len(v) or u not in v + v for v in units):
            units.append(u)
    alleles = []
    for _ in range(4):
        s = rand_seq(rng, rng.randrange(5, 41))
        for u in units:
            s += u * rng.randrange(6, 31)
        s += rand_seq(rng, rng.randrange(5, 41))
        alleles.append(noisy(rng, s, rate))
    return alleles, units


RECOVERY_SEEDS = {0.0: 20261, 0.01: 20262, 0.03: 20263}


def blocks(*parts):
    """repeat blocks (unit, copies) kept apart by N, so that every run is exactly the block"""
    return b"N" + b"N".join(u * n for u, n in parts) + b"N"


def ranking_cases():
    """(name, alleles, params): what the class and the rank rules decide"""
    return [
        ("three rotations, one class", [blocks((b"CAG", 8)), blocks((b"AGC", 8)), blocks((b"GCA", 9))], {}),
        ("representative: the lower begin wins a tie", [blocks((b"ACG", 6), (b"CGA", 6)), blocks((b"GAC", 6))], {}),
        ("representative: the lower allele wins a tie", [b"TT" + b"CGA" * 6 + b"N", blocks((b"ACG", 6)), blocks((b"GAC", 5))], {}),
        ("equal weight: the shorter first", [blocks((b"ACG", 6), (b"AT", 9))], {}),
        ("equal weight and length: the smaller rotation first", [blocks((b"TCA", 6), (b"GTA", 6), (b"GCA", 6))], {}),
        ("letter case and N", [blocks((b"cag", 7), (b"CAG", 5)).replace(b"N", b"n"), b"", b"NNNN", blocks((b"CaG", 6))], {}),
    ]


def threshold_cases():
    """(name, alleles, params): every threshold at equality and one step beyond"""
    top = blocks((b"CAG", 100), (b"TTGCA", 3))
    g10 = PROTOTYPES["G"][0]
    g9 = [F + b"ACGGTCATT" * 6 + G, F + b"ACGGTCATC" * 3 + G]
    return [
        ("weight = min_bases", [blocks((b"ACGT", 4))], dict(min_bases=16)),
        ("weight = min_bases - 1", [blocks((b"ACGT", 4))], dict(min_bases=17)),
        ("share = min_permille", [top], dict(min_permille=50)),
        ("share just under, by the parameter", [top], dict(min_permille=51)),
        ("share just under, by the input", [blocks((b"CAG", 101), (b"TTGCA", 3))], dict(min_permille=50)),
        ("2 edits in 20 bases: redundant", g10, dict(redundant_permille=100)),
        ("2 edits in 20 bases at 99: kept", g10, dict(redundant_permille=99)),
        ("2 edits in 18 bases: kept", g9, dict(redundant_permille=100)),
        ("2 edits in 18 bases at 112: redundant", g9, dict(redundant_permille=112)),
        ("nothing is redundant at 0 but a rotation's twin", PROTOTYPES["B"][0], dict(redundant_permille=0)),
        ("everything after the first is redundant at 1000", PROTOTYPES["A"][0], dict(redundant_permille=1000)),
    ]


def budget_cases():
    """(name, alleles, params): the top sixteen, the eight units, the 64 lanes"""
    rng = random.Random(5)
    six = []
    while len(six) < 20:
        u = primitive_unit(rng, 6)
        if all(u not in v + v for v in six):
            six.append(u)
    three = [b"AAC", b"AAG", b"AAT", b"ACC", b"ACG", b"ACT", b"AGC", b"AGG", b"AGT", b"ATC"]
    long = [primitive_unit(rng, p) for p in (200, 100, 40)]
    return [
        ("twenty classes: sixteen ranked", [blocks(*[(u, 4 + i) for i, u in enumerate(six[:10])]), blocks(*[(u, 14 + i) for i, u in enumerate(six[10:])])],
         dict(min_permille=0)),
        ("ten 3-base units: eight taken", [blocks(*[(u, 5 + i) for i, u in enumerate(three)])], dict(min_permille=0)),
        ("200 + 100 + 40 bases: the second does not fit", [blocks((long[0], 3)), blocks((long[1], 3)), blocks((long[2], 3))], {}),
    ]


def overflow_group(n_classes=2100, per_allele=70):
    """more distinct classes than the table admits: random 8-base units twice in a row, N between them"""
    rng = random.Random(11)
    seen, units = set(), []
    while len(units) < n_classes:
        u = primitive_unit(rng, 8)
        key = min(u[r:] + u[:r] for r in range(8))
        if key not in seen:
            seen.add(key); units.append(u)
    return [blocks(*[(u, 2) for u in units[i:i + per_allele]]) for i in range(0, n_classes, per_allele)]


def random_groups(seed, sizes, **kw):
    rng = random.Random(seed)
    return [random_group(rng, n, **kw) for n in sizes]

"""The allele sets of the motif tests (tests/test_motif_host.py runs them through the host harness, tests/test_gpu_motif.py on the device):
shapes chosen where the plane logic and the reductions can go wrong."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rs(rng, n, alpha=b"ACGT"):
    a = np.frombuffer(alpha, dtype=np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def substitute(rng, seq, n):
    s = bytearray(seq)
    for _ in range(n):
        i = int(rng.integers(0, len(s)))
        s[i] = b"ACGT"[(b"ACGT".index(bytes([s[i]]).upper()) + int(rng.integers(1, 4))) % 4]
    return bytes(s)


LITERALS = [b"CAG" * 20, b"CAG" * 10 + b"CTG" + b"CAG" * 9, b"CAG" * 20 + b"CCG" * 20, b"A" * 30, b"AAAG" * 25, b"ACAC", b"AC", b"A", b"", b"N" * 20]


def edge_set(seed=7):
    """word and lane edges, bytes that exercise the masks; every allele at most a few hundred bases"""
    rng = np.random.default_rng(seed)
    out = list(LITERALS) + [s.lower() for s in LITERALS[:6]]
    for L in (0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        out.append(rs(rng, L))                                            # random: near-ties
        out.append((rs(rng, 5) * (L // 5 + 1))[:L])                        # periodic, cut at the word edge
    for u in (31, 32, 33, 63, 64, 65):                                     # periods at and next to multiples of 32 and 64
        unit = rs(rng, u)
        for copies in (2, 3, 5):
            out.append(unit * copies)                                      # copies == 2: P = L / 2 exactly
        out.append(unit * 2 + unit[:1])                                    # L odd
        out.append(substitute(rng, unit * 4, 2))
    base = rs(rng, 7) * 30
    for pos in (0, 31, 32, 33, 63, 64, 100, len(base) - 1):                 # non-ACGT in the middle and at word boundaries
        s = bytearray(base); s[pos] = ord("N"); out.append(bytes(s))
    s = bytearray(base); s[60:70] = b"NNNNRYKMSW"; out.append(bytes(s))
    out += [b"N" * 64, base.lower(), b"acgtNNacgt" * 9, b"N" * 33 + b"ACG" * 20, rs(rng, 200, b"ACGTN"), b"N" * 200, rs(rng, 90)]
    out += [b"AC" * 40 + b"N" * 7 + b"AC" * 40, b"T" * 64, b"T" * 65, b"GT" * 32, b"G" * 31 + b"T" + b"G" * 32]
    # majority ties and the N phase: two copies that disagree (tie -> lower code), a phase that is N in every copy
    out += [b"ACGTAACGTC", b"ANGTANGTANGT", b"TTTTGTTTTG" * 3 + b"TTTTC"]
    return out


def random_set(seed=11, n=300):
    """300 alleles of 2-600 bases: half random sequence, half random units of 1-40 bases x random copies with 0-3 substitutions"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(2, 601))
        if i % 2 == 0:
            out.append(rs(rng, L))
        else:
            u = rs(rng, int(rng.integers(1, 41)))
            out.append(substitute(rng, (u * (L // len(u) + 1))[:L], int(rng.integers(0, 4))))
    return out

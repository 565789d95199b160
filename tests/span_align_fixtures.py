"""Shared pieces of the ends-free edit alignment tests: the C++ restatement (tests/edit_align_endsfree_ref.cpp) built with g++, the named
input sets (pairs with their free-end forms) and the restatement's answers computed once per (set, mode) for all tests of a session."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from compare_fixtures import ROOT, REF_SRC
from helpers import rand_seq, mutate, tr_seq

SPAN_REF_SRC = os.path.join(ROOT, "tests", "edit_align_endsfree_ref.cpp")

DEFAULT = (10, 50, 1)
OTHER = (2, 3, 2)
WIDTHS = (0, 1, 63, 64, 65, 130)


def reference_form(a, b, kind, on_text=False):
    """align_anreads' ends-free calls (src/analignments.cpp:85-97).  The longer read is the pattern; the free ends, length_diff long, are the
    pattern's when the longer read is the spanning one (:94-96) and the text's when it is the partial one (:88-90, on_text); kind 0: the
    partial read spans the left side (free end), 1: the right side (free begin), 2: neither (half / half).  -> (pattern, text, form)"""
    if len(a) < len(b):
        a, b = b, a
    d = len(a) - len(b)
    halves = [(0, d), (d, 0), (d // 2, d // 2)][kind]
    return (a, b, (0, 0) + halves) if on_text else (a, b, halves + (0, 0))


def _partial(rng, full, kind, err):
    """a read that covers one part of `full`: its left part (kind 0), its right part (1) or its middle (2)"""
    n = len(full)
    cut = int(rng.integers(max(1, n // 3), max(2, n - 1)))
    if kind == 0:
        part = full[:cut]
    elif kind == 1:
        part = full[n - cut:]
    else:
        a = (n - cut) // 2
        part = full[a:a + cut]
    return mutate(rng, part, err) or b"A"


def _forms_set(seed, n, lmin, lmax):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(lmin, lmax))
        full = tr_seq(rng, L) if i % 2 else rand_seq(rng, L)
        kind = i % 3
        part = _partial(rng, full, kind, [0.01, 0.05, 0.15][(i // 3) % 3])
        out.append(reference_form(full, part, kind, on_text=(i // 9) % 2 == 1))
    return out


def _widths_set():
    """free widths around the chunk boundaries of the score-0 row and of the end test, on each of the four ends: the short sequence is a
    mutated copy of the long one without its first (last) `w` bases, so the free end is what the alignment uses"""
    rng = np.random.default_rng(72)
    out = []
    for w in WIDTHS:
        for side in range(4):
            core = tr_seq(rng, 180) if w % 2 else rand_seq(rng, 180)
            extra = rand_seq(rng, w)
            short = mutate(rng, core, 0.04) or b"A"
            if side == 0:
                out.append((extra + core, short, (w, 0, 0, 0)))       # pattern begin free
            elif side == 1:
                out.append((core + extra, short, (0, w, 0, 0)))       # pattern end free
            elif side == 2:
                out.append((short, extra + core, (0, 0, w, 0)))       # text begin free
            else:
                out.append((short, core + extra, (0, 0, 0, w)))       # text end free
        # all four at once, and the free end larger than what the alignment wants
        a, b = rand_seq(rng, 150), rand_seq(rng, 150)
        out.append((a, mutate(rng, a, 0.1) or b"A", (w, w, w, w)))
        out.append((a, b, (w, w, w, w)))
    return out


def _edge_set():
    rng = np.random.default_rng(73)
    p = rand_seq(rng, 120)
    out = [
        # free values larger than the sequences (clamping)
        (p, p[30:90], (500, 500, 0, 0)), (p[30:90], p, (0, 0, 500, 500)), (p, mutate(rng, p[10:100], 0.05), (1000, 1000, 1000, 1000)),
        (b"ACGT", b"ACGT", (9, 9, 9, 9)), (b"ACGT", b"TTTT", (100, 100, 100, 100)),
        # an empty pattern or text
        (b"", b"", (0, 0, 0, 0)), (b"", b"", (3, 3, 3, 3)), (b"ACGT", b"", (0, 0, 0, 0)), (b"ACGT", b"", (4, 0, 0, 0)), (b"ACGT", b"", (0, 4, 0, 0)),
        (b"ACGT", b"", (2, 2, 0, 0)), (b"ACGT", b"", (1, 1, 0, 0)), (b"", b"ACGT", (0, 0, 0, 0)), (b"", b"ACGT", (0, 0, 4, 0)), (b"", b"ACGT", (0, 0, 1, 2)),
        (b"", b"ACGT", (7, 7, 7, 7)),
        # score-0 endings: the text is an infix, a prefix, a suffix of the pattern, and the other way round
        (p, p[40:80], (40, 40, 0, 0)), (p, p[:80], (0, 40, 0, 0)), (p, p[40:], (40, 0, 0, 0)), (p, p[40:80], (60, 60, 0, 0)),
        (p[40:80], p, (0, 0, 40, 40)), (p[:80], p, (0, 0, 0, 40)), (p[40:], p, (0, 0, 40, 0)),
        # the same with one free base too few on either side
        (p, p[40:80], (39, 40, 0, 0)), (p, p[40:80], (40, 39, 0, 0)), (p[40:80], p, (0, 0, 39, 40)), (p[40:80], p, (0, 0, 40, 39)),
        # single bases
        (b"A", b"C", (0, 0, 0, 0)), (b"A", b"C", (1, 0, 0, 0)), (b"A", b"C", (0, 1, 0, 0)), (b"A", b"C", (0, 0, 1, 0)), (b"A", b"C", (0, 0, 0, 1)),
        (b"AB", b"BA", (1, 1, 1, 1)), (b"AB", b"BA", (0, 1, 1, 0)), (b"AB", b"BA", (1, 0, 0, 1)),
    ]
    return out


def _ties_set():
    """tandem repeats and homopolymers: many diagonals of one score satisfy the end test; the lowest has to win"""
    rng = np.random.default_rng(74)
    out = []
    for n, m in ((40, 25), (100, 64), (200, 130), (300, 171)):
        out.append((b"A" * n, b"A" * m, (n - m, n - m, 0, 0)))
        out.append((b"A" * m, b"A" * n, (0, 0, n - m, n - m)))
        out.append((b"A" * n, b"A" * m, (n, n, n, n)))
        out.append((b"A" * n, b"A" * (m // 2) + b"C" + b"A" * (m - m // 2), ((n - m) // 2, n - m, 0, 0)))
        for motif in (b"AC", b"ACG", b"AACGT"):
            a = (motif * (n // len(motif) + 1))[:n]
            b = (motif * (m // len(motif) + 1))[:m]
            out.append((a, b, (n - m, n - m, 0, 0)))
            out.append((b, a, (0, 0, n - m, n - m)))
            out.append((a, mutate(rng, b, 0.06) or b"A", ((n - m) // 2, (n - m + 1) // 2, 0, 0)))
            out.append((mutate(rng, b, 0.06) or b"A", a, (0, 0, n - m, 3)))
            out.append((a, mutate(rng, b, 0.06) or b"A", (n, n, 7, 7)))
    return out


def _wide_set():
    """[0]: S = E = 2 201 diagonals for every score: past the 2 048 diagonals of the LDS window in exact mode, and a start wider than the
    LDS window of the adaptive pass; [1]: above 32 766 bases (what 16-bit offsets hold) with small free ends; [2]: the reference's
    left-spanning form on a pair of about 2 kb"""
    rng = np.random.default_rng(75)
    x, y, z = rand_seq(rng, 2200), rand_seq(rng, 400), rand_seq(rng, 2200)
    a = rand_seq(rng, 33000)
    full = rand_seq(rng, 2000)
    return [(x + y, (mutate(rng, y, 0.05) or b"A") + z, (2200, 0, 0, 2200)),
            (rand_seq(rng, 5) + a + rand_seq(rng, 7), mutate(rng, a, 0.003), (5, 7, 0, 0)),
            reference_form(full, mutate(rng, full[:1500], 0.03), 0)]


def _host_set():
    """a few hundred pairs for the CPU checks: the reference's forms, the chunk-boundary widths, the edge cases, the tie-heavy pairs, random
    forms on all four ends and forms that are all zero"""
    rng = np.random.default_rng(76)
    out = _forms_set(77, 120, 30, 400) + _widths_set() + _edge_set() + _ties_set()
    for i in range(120):
        n = int(rng.integers(1, 300))
        a = tr_seq(rng, n) if i % 2 else rand_seq(rng, n)
        b = mutate(rng, a, float(rng.choice([0.02, 0.1, 0.4]))) or b"C"
        if i % 4 == 0:
            b = b[int(rng.integers(0, len(b))):] or b"C"
        f = (0, 0, 0, 0) if i % 6 == 5 else tuple(int(x) for x in rng.integers(0, [3, 20, 150][i % 3], 4))
        out.append((a, b, f) if i % 3 else (b, a, f))
    return out


@functools.lru_cache(maxsize=None)
def input_set(name):
    """-> tuple of (pattern, text, (pbf, pef, tbf, tef))"""
    if name == "HOST":
        return tuple(_host_set())
    if name == "WIDTHS":
        return tuple(_widths_set())
    if name == "EDGE":
        return tuple(_edge_set())
    if name == "TIES":
        return tuple(_ties_set())
    if name == "FORMS":
        return tuple(_forms_set(71, 60, 30, 400))
    if name == "WIDE":
        return tuple(_wide_set())
    raise KeyError(name)


def split(cases):
    """-> ([(pattern, text)], [form]) for helpers.pair_tasks"""
    return [(p, t) for p, t, _ in cases], [f for _, _, f in cases]


@functools.lru_cache(maxsize=None)
def _exes():
    tmp = tempfile.mkdtemp(prefix="span_align_ref_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = {}
    for key, src in (("span", SPAN_REF_SRC), ("exact", REF_SRC)):
        exe = os.path.join(tmp, key)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, src])
        out[key] = exe
    return out


def run_span_ref(cases, mode):
    """[(pattern, text, form)] -> [(score, cells, op string)]; mode: ("full",), ("hexagon",) or ("adaptive", a, b, c)"""
    inp = "".join("%s %s %d %d %d %d\n" % ((p.decode() or "-", t.decode() or "-") + tuple(f)) for p, t, f in cases).encode()
    r = subprocess.run([_exes()["span"]] + [str(x) for x in mode], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-500:]
    out = []
    for line in r.stdout.decode().splitlines():
        s, c, o = line.split(" ")
        out.append((int(s), int(c), b"" if o == "-" else o.encode()))
    assert len(out) == len(cases)
    return out


def run_exact_ref(pairs):
    """[(pattern, text)] -> [(score, op string)] from tests/edit_align_ref.cpp (end to end, full wavefronts)"""
    inp = "".join("%s %s\n" % (p.decode() or "-", t.decode() or "-") for p, t in pairs).encode()
    r = subprocess.run([_exes()["exact"], "align"], input=inp, capture_output=True, timeout=600, check=True)
    out = []
    for line in r.stdout.decode().splitlines():
        s, o = line.split(" ")
        out.append((int(s), b"" if o == "-" else o.encode()))
    assert len(out) == len(pairs)
    return out


@functools.lru_cache(maxsize=None)
def span_ref(name, mode=("full",)):
    """the restatement on a named input set: computed once, shared by the tests, never changed"""
    return tuple(run_span_ref(input_set(name), mode))


def mode_of(params):
    """None -> exact, (a, b, c) -> wfadaptive"""
    return ("full",) if params is None else ("adaptive",) + tuple(params)

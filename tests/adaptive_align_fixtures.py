"""Shared pieces of the adaptive-mode edit alignment tests: the C++ restatement (tests/edit_align_adaptive_ref.cpp) built with g++, the
pair generator and the four input sets, and the restatement's answers computed once per (set, parameters) for all tests of a session."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from compare_fixtures import ROOT, REF_SRC
from helpers import rand_seq, mutate

ADAPTIVE_REF_SRC = os.path.join(ROOT, "tests", "edit_align_adaptive_ref.cpp")

DEFAULT = (10, 50, 1)
NEVER_CUTS = (10, 3000, 1)
SMALL_PARAMS = [(10, 50, 1), (1, 0, 1), (10, 50, 3), (64, 20, 2), (4, 8, 1)]
MID_PARAMS = [DEFAULT, NEVER_CUTS]


def oriented(a, b):
    """the longer sequence first, the second on ties: every pair goes in as (pattern, text) in this orientation"""
    return (a, b) if len(a) > len(b) else (b, a)


def tr_pair(rng, L, err, dl=0.0):
    m = int(rng.integers(2, 7)); motif = rand_seq(rng, m)
    fl, fr = rand_seq(rng, 60), rand_seq(rng, 60)
    a = fl + (motif * (L // m + 1))[:L] + fr
    Lb = max(m, int(L * (1.0 - dl)))
    b = fl + (motif * (Lb // m + 1))[:Lb] + fr
    return mutate(rng, a, err), mutate(rng, b, err)


def pairs(seed, n, lmin, lmax):
    rng = np.random.default_rng(seed); out = []
    for i in range(n):
        L = int(rng.integers(lmin, lmax)); kind = i % 5
        if kind < 4: a, b = tr_pair(rng, L, [0.002, 0.07, 0.07, 0.12][kind], dl=[0.0, 0.0, 0.2, 0.05][kind])
        else: a, b = rand_seq(rng, L), mutate(rng, rand_seq(rng, L), 0.1)
        out.append((a, b) if len(a) > len(b) else (b, a))
    return out


@functools.lru_cache(maxsize=None)
def input_set(name):
    if name == "SMALL":
        return pairs(61, 300, 5, 400)
    if name == "MID":
        return pairs(62, 48, 800, 3000)
    if name == "LONG":
        return pairs(63, 6, 6000, 12000)
    if name == "HAND":
        rng = np.random.default_rng(64)
        a = rand_seq(rng, 40000)                       # past 32 766: what 16-bit offsets hold
        return [(b"AB", b"BA"), (b"", b""), (b"ACGT", b""), (b"", b"ACGT"), (b"A", b"C"), (b"N" * 70, b"N" * 70),
                oriented(a, mutate(rng, a, 0.003))]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _exes():
    tmp = tempfile.mkdtemp(prefix="adaptive_align_ref_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = {}
    for key, src in (("adaptive", ADAPTIVE_REF_SRC), ("exact", REF_SRC)):
        exe = os.path.join(tmp, key)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, src])
        out[key] = exe
    return out


def _stdin(prs):
    return "".join("%s %s\n" % (p.decode() or "-", t.decode() or "-") for p, t in prs).encode()


def run_adaptive_ref(prs, params):
    """[(pattern, text)] -> [(score, cells, op string)] from the adaptive restatement"""
    r = subprocess.run([_exes()["adaptive"], "align"] + [str(int(x)) for x in params], input=_stdin(prs), capture_output=True, timeout=600, check=True)
    out = []
    for line in r.stdout.decode().splitlines():
        s, c, o = line.split(" ")
        out.append((int(s), int(c), b"" if o == "-" else o.encode()))
    assert len(out) == len(prs)
    return out


def run_exact_ref(prs):
    """[(pattern, text)] -> [(score, op string)] from tests/edit_align_ref.cpp (full wavefronts)"""
    r = subprocess.run([_exes()["exact"], "align"], input=_stdin(prs), capture_output=True, timeout=600, check=True)
    out = []
    for line in r.stdout.decode().splitlines():
        s, o = line.split(" ")
        out.append((int(s), b"" if o == "-" else o.encode()))
    assert len(out) == len(prs)
    return out


@functools.lru_cache(maxsize=None)
def adaptive_ref(name, params=DEFAULT):
    """the adaptive restatement on a named input set: computed once, shared by the tests, never changed"""
    return tuple(run_adaptive_ref(input_set(name), params))


@functools.lru_cache(maxsize=None)
def exact_ref(name):
    return tuple(run_exact_ref(input_set(name)))


def valid(p, t, ops, s):
    """ops is an alignment of p against t with s edit operations"""
    v = h = 0
    for c in ops.decode():
        if c == "M":
            assert p[v] == t[h]; v += 1; h += 1
        elif c == "X":
            assert p[v] != t[h]; v += 1; h += 1
        elif c == "I":
            h += 1
        elif c == "D":
            v += 1
        else:
            raise AssertionError(c)
    assert (v, h) == (len(p), len(t))
    assert len(ops) - ops.count(b"M") == s

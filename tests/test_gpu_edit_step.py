"""GPU parity of the bit-parallel edit tiers' column step (otter_amd/csrc/myers_step.hpp inside myers_edit.hip): scores against the CPU
oracle on the smallest shapes at which the step on 32-bit halves can go wrong — pattern lengths at the half-word, block and 2 / 3 / 4-block
superblock edges, the add's carry running through and out of a block, edits at rows 31 / 32 / 63 / 64 / 65, the fifth mask row, the ends-free
first and last column — plus one unrelated pair per tier, so that every <BPL, GL> body is the one that finishes something.

Every batch runs three ways: in the session process, in a child with all eight tiers enabled, and in a child with all tiers, un-routed and
un-sorted (every pair enters at tier 0 and climbs: each tier also runs its refusal path `best > K` on the pairs too wide for it, where a
wrong score that happens to be <= K would surface).  The oracle runs once, in the session process; the children read its scores from a file."""
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import rand_seq, mutate, pair_tasks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED_ENV = "OTG_TEST_EDIT_STEP_EXPECTED"      # set for the children: the .npz of oracle scores written by the session process

M_EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513)
D_EDGES = (0, 1, 2, 63, 64, 65)
EDIT_ROWS = (31, 32, 63, 64, 65)
# R = (GL - 1) * 64 * BPL + GL of each tier in launch order (myers_edit.hip), and the pattern length whose unrelated (m, 0.92 m) pair it should finish
TIER_R = (456, 904, 1352, 1936, 2896, 4000, 8128, 16192)
TIER_M = (None, 1400, 2200, 3200, 4800, 7000, 13000)


def _forms(d):
    return [None] if d == 0 else [None, (0, d, 0, 0), (d, 0, 0, 0), (d // 2, d // 2, 0, 0)]


def _edge_batch():
    rng = np.random.default_rng(2024)
    pairs, forms = [], []

    def add(a, b, fs=(None,)):
        if len(b) > len(a):
            a, b = b, a
        if len(b) < 1:
            return
        for f in fs:
            pairs.append((a, b)); forms.append(f)

    for m in M_EDGES:
        r = rand_seq(rng, m)
        unit = rand_seq(rng, 5)
        tr = (unit * (m // 5 + 1))[:m]
        for d in D_EDGES:
            n = m - d
            if n < 1:
                continue
            fs = _forms(d)
            add(b"A" * m, b"A" * n, fs)                      # every mask bit set: the add's carry ripples through all 64 bits and out of the block
            add(r, r[:n], fs); add(r, r[d:], fs)             # identical random sequences
            add(b"A" * m, b"C" * n, fs)                      # distance m
            add(r, rand_seq(rng, n), fs)                     # unrelated: far enough apart to leave the wavefront pass at every m >= ~100
            add(mutate(rng, r, 0.3), r[:n], fs)
            rn = bytearray(r); rn[m // 2] = ord("N")         # the fifth table row
            add(bytes(rn), r[:n], fs)
            for e in EDIT_ROWS:                              # a tandem repeat with one unit removed at a block edge
                if e + len(unit) <= n:
                    add(tr, tr[:e] + tr[e + len(unit):n + len(unit)], fs)
        for e in EDIT_ROWS:                                  # one substitution, insertion, deletion at a half-word / block edge
            if e >= m:
                continue
            sub = bytearray(r); sub[e] = ord("C") if r[e:e + 1] == b"A" else ord("A")
            add(r, bytes(sub))
            add(r, r[:e] + r[e + 1:])
            add(r, r[:e] + (b"G" if r[e:e + 1] != b"G" else b"T") + r[e:])
            # ... on a pair that reaches the bit-parallel tiers: a far-off second half
            if m >= 192:
                far = r[:m // 2] + rand_seq(rng, m - m // 2)
                add(far, bytes(sub)); add(far, r[:e] + r[e + 1:])
    return pairs, forms


def _tier_batch():
    rng = np.random.default_rng(4096)
    pairs = [(rand_seq(rng, m), rand_seq(rng, int(0.92 * m))) for m in TIER_M[1:]]
    pairs.append((rand_seq(rng, 16384), rand_seq(rng, 12000)))          # for <4,64>: a distance above the 8 128 of <2,64> (asserted below)
    return pairs, [None] * len(pairs)


def _batches():
    return {"edges": pair_tasks(*_edge_batch()), "tiers": pair_tasks(*_tier_batch())}


@pytest.fixture(scope="module")
def batches():
    return _batches()


@pytest.fixture(scope="module")
def expected(request, batches, tmp_path_factory):
    """name -> oracle scores, and the file that holds them"""
    path = os.environ.get(EXPECTED_ENV)
    if path:
        with np.load(path) as z:
            return {k: z[k] for k in z.files}, path
    oracle = request.getfixturevalue("oracle")
    exp = {name: oracle.edit_distance_batch(arena, tasks) for name, (arena, tasks) in batches.items()}
    t = exp["tiers"]
    for i in range(1, len(TIER_R)):       # each unrelated pair lies in the band range of its own tier, above the one before
        assert TIER_R[i - 1] < t[i - 1] <= TIER_R[i], (i, int(t[i - 1]))
    path = str(tmp_path_factory.mktemp("edit_step") / "expected.npz")
    np.savez(path, **exp)
    return exp, path


def test_edit_step_scores(gpu, batches, expected):
    exp = expected[0]
    for name, (arena, tasks) in batches.items():
        got = gpu.edit_distance_batch(arena, tasks)
        bad = [(int(i), int(tasks[i]["pattern_len"]), int(tasks[i]["text_len"]), int(got[i]), int(exp[name][i])) for i in np.nonzero(got != exp[name])[0]]
        print("%s: %d pairs, %d differ" % (name, len(got), len(bad)))
        assert not bad, (name, len(bad), bad[:10])


@pytest.mark.parametrize("switch", ["OTG_EDIT_TIERS=255", "OTG_EDIT_TIERS=255 OTG_NO_EDIT_ROUTE=1 OTG_NO_EDIT_SORT=1"], ids=["all_tiers", "all_tiers_unrouted"])
def test_edit_step_scores_child(gpu, expected, switch):
    gpu.trim()
    env = dict(os.environ)
    for kv in switch.split():
        k, _, v = kv.partition("=")
        env[k] = v
    env[EXPECTED_ENV] = expected[1]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_edit_step.py::test_edit_step_scores"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (switch, r.stdout[-3000:], r.stderr[-1000:])

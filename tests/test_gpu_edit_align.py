"""otg_edit_align_batch (WFAlignerEdit(Alignment, MemoryMed), src/compare.cpp:59-61,95) on the device: op strings and scores byte for byte
equal to the C++ restatement of WFA2-lib's edit piggy-back (tests/edit_align_ref.cpp), scores equal to otg_edit_distance_batch and the
oracle, every op string a valid alignment of its cost, the column counts of the length-only call equal to the string lengths."""
import numpy as np
import pytest

from otter_amd import abi
from compare_fixtures import build_ref, ref_align, oriented
from helpers import rand_seq, mutate, tr_seq, pair_tasks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("edit_align_ref_gpu"))


def _pairs():
    rng = np.random.default_rng(21)
    pairs = [(b"AB", b"BA"), (b"BA", b"AB"), (b"ACGT", b"ACGT"), (b"ACGT", b""), (b"", b"ACGT"), (b"", b""), (b"A", b"C"),
             (b"AAAAAAAAAA", b"AAAAAAA"), (b"ACACACACAC", b"CACACACACA")]
    for n in (3, 30, 63, 64, 65, 127, 128, 500, 1000, 2047, 2048, 2049, 4100):        # tie-heavy tandem repeats and swaps
        a = tr_seq(rng, n)
        pairs.append(oriented(a, mutate(rng, a, 0.1)))
        b = bytearray(rand_seq(rng, n))
        for i in range(0, n - 1, 7):
            b[i], b[i + 1] = b[i + 1], b[i]
        pairs.append(oriented(bytes(b), rand_seq(rng, 0) + bytes(b[::-1][:n // 2]) + bytes(b[n // 2:])))
    for n in (300, 1500, 4000, 9000):                                                   # divergent pairs: wide diamonds (the global-row tier)
        pairs.append(oriented(rand_seq(rng, n), rand_seq(rng, n - n // 10)))
    for n in (4000, 10000):                                                             # very unequal lengths: diamonds one or two diagonals wide
        a = rand_seq(rng, n)
        pairs.append((a, mutate(rng, a[: n // 10], 0.05)))
    for n in (33000, 40000):                                                            # above 32 766
        a = rand_seq(rng, n)
        pairs.append(oriented(a, mutate(rng, a, 0.003)))
    for _ in range(200):
        n = int(rng.integers(1, 400))
        a = tr_seq(rng, n) if rng.integers(0, 2) else rand_seq(rng, n)
        pairs.append(oriented(a, mutate(rng, a, float(rng.choice([0.01, 0.05, 0.2, 0.6])))))
    return pairs


def _valid(p, t, ops, s):
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


def test_edit_align_matches_restatement(gpu, oracle, ref_exe):
    pairs = _pairs()
    arena, tasks = pair_tasks(pairs)
    scores, cigs = gpu.edit_align_batch(arena, tasks)
    want = ref_align(ref_exe, pairs)
    for i, ((p, t), (s, o)) in enumerate(zip(pairs, want)):
        assert int(scores[i]) == s, (i, len(p), len(t))
        assert cigs[i] == o, (i, len(p), len(t))
        _valid(p, t, cigs[i], s)
    assert np.array_equal(scores, gpu.edit_distance_batch(arena, tasks))
    assert np.array_equal(scores, oracle.edit_distance_batch(arena, tasks))
    s2, lens = gpu.edit_align_batch(arena, tasks, want_cigars=False)
    assert np.array_equal(s2, scores)
    assert lens.tolist() == [len(c) for c in cigs]
    assert cigs[0] == b"XX"


def test_edit_align_independent_of_batch_order(gpu):
    """the same op strings whatever the order of the tasks in the batch (tier lists and tickets change, results must not)"""
    pairs = _pairs()[:60]
    arena, tasks = pair_tasks(pairs)
    a = gpu.edit_align_batch(arena, tasks)
    b = gpu.edit_align_batch(*pair_tasks(pairs[::-1]))
    assert a[1] == b[1][::-1]


def test_edit_align_refuses_endsfree_and_adaptive(gpu):
    arena, tasks = pair_tasks([(b"ACGTACGT", b"ACGTTACGT")])
    t2 = tasks.copy()
    t2["endsfree"] = 1
    with pytest.raises(Exception) as e:
        gpu.edit_align_batch(arena, t2)
    assert "ends-free" in str(e.value)
    gpu.set_heuristic(abi.OTG_HEURISTIC_WFADAPTIVE, 10, 50, 1)
    try:
        with pytest.raises(Exception) as e:
            gpu.edit_align_batch(arena, tasks)
        assert "exact alignment only" in str(e.value)
    finally:
        gpu.set_heuristic(abi.OTG_HEURISTIC_NONE)
    s, c = gpu.edit_align_batch(arena, tasks)
    assert int(s[0]) == 1 and len(c[0]) == 9

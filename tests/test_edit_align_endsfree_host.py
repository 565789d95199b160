"""The CPU restatement of ends-free edit alignment with op strings (tests/edit_align_endsfree_ref.cpp), which pins the device op strings of
otg_edit_align_span_batch: its scores equal the oracle's score chain (exact and under wfadaptive, there with the cells) and, in exact mode,
the O(nm) dynamic programme; every op string is an alignment whose operations outside the free end gaps cost its score; recomputed inside
the region the device pass keeps it gives the identical strings; with nothing free it is the end-to-end restatement."""
import pytest

import span_align_fixtures as fx
from helpers import pair_tasks

ADAPTIVE = [fx.DEFAULT, fx.OTHER, (1, 0, 1)]


def _columns(p, t, ops):
    """every op names a column of the two sequences, free gaps included"""
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


def test_input_set_is_a_few_hundred_pairs_of_every_kind():
    cases = fx.input_set("HOST")
    assert len(cases) >= 300
    assert sum(1 for _, _, f in cases if f == (0, 0, 0, 0)) >= 10
    assert sum(1 for _, _, f in cases if f[0] or f[1]) >= 50 and sum(1 for _, _, f in cases if f[2] or f[3]) >= 50


def test_exact_scores_equal_the_oracle_and_the_dynamic_programme(oracle):
    cases = fx.input_set("HOST")
    want = fx.span_ref("HOST")
    arena, tasks = pair_tasks(*fx.split(cases))
    scores, cells = oracle.edit_distance_batch(arena, tasks, want_cells=True)
    assert scores.tolist() == [w[0] for w in want]
    assert cells.tolist() == [w[1] for w in want]
    for i, ((p, t, f), (s, _, ops)) in enumerate(zip(cases, want)):
        assert oracle.dp_edit(p, t, f) == s, (i, f)
        assert oracle.cigar_score(p, t, ops, x=1, o=0, e=1, form=f) == s, (i, f, ops)
        _columns(p, t, ops)
        assert len(ops) == len(p) + ops.count(b"I")


@pytest.mark.parametrize("params", ADAPTIVE, ids=["%d-%d-%d" % p for p in ADAPTIVE])
def test_adaptive_scores_and_cells_equal_the_oracle(oracle, params):
    cases = fx.input_set("HOST")
    want = fx.span_ref("HOST", fx.mode_of(params))
    arena, tasks = pair_tasks(*fx.split(cases))
    oracle.set_heuristic(1, *params)
    try:
        scores, cells = oracle.edit_distance_batch(arena, tasks, want_cells=True)
    finally:
        oracle.set_heuristic(0)
    assert scores.tolist() == [w[0] for w in want]
    assert cells.tolist() == [w[1] for w in want]
    for i, ((p, t, f), (s, _, ops)) in enumerate(zip(cases, want)):
        assert oracle.cigar_score(p, t, ops, x=1, o=0, e=1, form=f) == s, (i, f, ops)
        _columns(p, t, ops)


def test_adaptive_input_set_separates_the_modes():
    """a condition on the inputs, not on the code under test: under (1, 0, 1) some score and some op string differ from exact"""
    want, exact = fx.span_ref("HOST", fx.mode_of((1, 0, 1))), fx.span_ref("HOST")
    assert all(w[0] >= e[0] for w, e in zip(want, exact))
    assert sum(1 for w, e in zip(want, exact) if w[0] != e[0]) >= 1 and sum(1 for w, e in zip(want, exact) if w[2] != e[2]) >= 1


def test_device_input_sets_separate_the_modes():
    """conditions on the inputs of the device tests: under the second parameter set some op strings and some scores differ from exact"""
    n_ops = n_scores = 0
    for name in ("WIDTHS", "TIES", "FORMS"):
        want, exact = fx.span_ref(name, fx.mode_of(fx.OTHER)), fx.span_ref(name)
        n_ops += sum(1 for w, e in zip(want, exact) if w[2] != e[2])
        n_scores += sum(1 for w, e in zip(want, exact) if w[0] != e[0])
    assert n_ops >= 3 and n_scores >= 1


def test_hexagon_gives_the_identical_strings():
    """the restatement's hexagon mode fails unless every pair's score and string are those of the full wavefronts"""
    for name in ("HOST", "WIDE"):
        assert fx.span_ref(name, ("hexagon",)) == fx.span_ref(name)


def test_nothing_free_is_the_end_to_end_restatement():
    cases = [(p, t, (0, 0, 0, 0)) for p, t, _ in fx.input_set("HOST")]
    got = fx.run_span_ref(cases, ("full",))
    want = fx.run_exact_ref([(p, t) for p, t, _ in cases])
    assert [(s, o) for s, _, o in got] == want
    assert [(s, o) for s, _, o in fx.run_span_ref(cases, ("hexagon",))] == want


def test_first_diagonal_in_ascending_order_wins():
    """a homopolymer text inside a longer homopolymer pattern: every start ends at score 0; the lowest diagonal that ends, k = -(n - m),
    has the whole free gap in front"""
    n, m = 40, 25
    (s, _, ops), = fx.run_span_ref([(b"A" * n, b"A" * m, (n - m, n - m, 0, 0))], ("full",))
    assert (s, ops) == (0, b"D" * (n - m) + b"M" * m)
    (s, _, ops), = fx.run_span_ref([(b"A" * m, b"A" * n, (0, 0, n - m, n - m))], ("full",))
    assert (s, ops) == (0, b"M" * m + b"I" * (n - m))

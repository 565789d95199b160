"""The CPU restatement of adaptive-mode edit alignment (tests/edit_align_adaptive_ref.cpp), which pins the device op strings of
otg_edit_align_heur_batch: its scores AND cells equal the oracle's under the same heuristic, every op string is a valid alignment of its
score, with parameters that never cut it equals the exact restatement, and the input sets do separate the two modes."""
import numpy as np
import pytest

import adaptive_align_fixtures as fx
from helpers import pair_tasks

CASES = [("SMALL", p) for p in fx.SMALL_PARAMS] + [("MID", p) for p in fx.MID_PARAMS]


@pytest.mark.parametrize("name,params", CASES, ids=["%s-%d-%d-%d" % ((n,) + p) for n, p in CASES])
def test_restatement_scores_and_cells_equal_the_oracle(oracle, name, params):
    prs = fx.input_set(name)
    want = fx.adaptive_ref(name, params)
    arena, tasks = pair_tasks(prs)
    oracle.set_heuristic(1, *params)
    try:
        scores, cells = oracle.edit_distance_batch(arena, tasks, want_cells=True)
    finally:
        oracle.set_heuristic(0)
    assert scores.tolist() == [w[0] for w in want]
    assert cells.tolist() == [w[1] for w in want]
    for (p, t), (s, _, ops) in zip(prs, want):
        fx.valid(p, t, ops, s)


def test_restatement_without_a_cut_is_the_exact_alignment():
    want = fx.adaptive_ref("MID", fx.NEVER_CUTS)
    exact = fx.exact_ref("MID")
    assert [(s, o) for s, _, o in want] == list(exact)


@pytest.mark.parametrize("name,params", [("MID", fx.DEFAULT), ("SMALL", (1, 0, 1))])
def test_input_sets_separate_the_modes(name, params):
    """conditions on the inputs, not on the code under test: some op string and some op-string length differ from exact"""
    want = fx.adaptive_ref(name, params)
    exact = fx.exact_ref(name)
    n_ops = sum(1 for (_, _, o), (_, e) in zip(want, exact) if o != e)
    n_len = sum(1 for (_, _, o), (_, e) in zip(want, exact) if len(o) != len(e))
    n_score = sum(1 for (s, _, _), (e, _) in zip(want, exact) if s != e)
    print(name, params, "op strings that differ:", n_ops, "lengths:", n_len, "scores:", n_score)
    assert n_ops >= 1 and n_len >= 1
    assert all(s >= e for (s, _, _), (e, _) in zip(want, exact))

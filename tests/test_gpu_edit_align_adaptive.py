"""otg_edit_align_heur_batch on the device: WFAlignerEdit(Alignment, MemoryMed)::alignEnd2End after setHeuristicWFadaptive.  Scores, cells
and op strings byte for byte equal to the CPU restatement of the cut with provenance (tests/edit_align_adaptive_ref.cpp, itself checked
against the oracle in test_edit_align_adaptive_host.py); both storage tiers of the provenance pass run and agree; the batch order, the
memory budget and the context's own heuristic do not change a result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from otter_amd import abi
import adaptive_align_fixtures as fx
from compare_fixtures import ROOT
from helpers import pair_tasks

pytestmark = pytest.mark.gpu

AD = abi.OTG_HEURISTIC_WFADAPTIVE
CHILD = os.path.join(ROOT, "tests", "edit_align_adaptive_child.py")
CASES = [("SMALL", p) for p in fx.SMALL_PARAMS] + [("MID", p) for p in fx.MID_PARAMS] + [("LONG", fx.DEFAULT), ("HAND", fx.DEFAULT)]


def _assert_equals_restatement(prs, want, scores, cells, cigs):
    for i, ((p, t), (s, c, o)) in enumerate(zip(prs, want)):
        assert int(scores[i]) == s, (i, len(p), len(t))
        assert int(cells[i]) == c, (i, len(p), len(t))
        assert cigs[i] == o, (i, len(p), len(t))


@pytest.mark.parametrize("name,params", CASES, ids=["%s-%d-%d-%d" % ((n,) + p) for n, p in CASES])
def test_adaptive_align_matches_restatement(gpu, name, params):
    prs = fx.input_set(name)
    want = fx.adaptive_ref(name, params)
    arena, tasks = pair_tasks(prs)
    scores, cigs, cells = gpu.edit_align_heur_batch(arena, tasks, AD, *params, want_cells=True)
    _assert_equals_restatement(prs, want, scores, cells, cigs)
    # the score chain on a context set to the same heuristic
    gpu.set_heuristic(AD, *params)
    try:
        s2, c2 = gpu.edit_distance_batch(arena, tasks, want_cells=True)
    finally:
        gpu.set_heuristic(abi.OTG_HEURISTIC_NONE)
    assert np.array_equal(scores, s2) and np.array_equal(cells, c2)
    # the length-only call
    s3, lens = gpu.edit_align_heur_batch(arena, tasks, AD, *params, want_cigars=False)
    assert np.array_equal(s3, scores)
    assert lens.tolist() == [len(c) for c in cigs]


def test_both_tiers_ran(gpu):
    """SMALL stays inside the LDS window; the widest wavefront of MID under parameters that never cut (3 065 diagonals) does not"""
    gpu.edit_align_heur_batch(*pair_tasks(fx.input_set("SMALL")), AD, *fx.DEFAULT)
    lds, glb = gpu.edit_align_last_tiers()
    assert lds >= 1 and lds + glb == len(fx.input_set("SMALL"))
    gpu.edit_align_heur_batch(*pair_tasks(fx.input_set("MID")), AD, *fx.NEVER_CUTS)
    lds, glb = gpu.edit_align_last_tiers()
    assert glb >= 1 and lds + glb == len(fx.input_set("MID"))


def _child(name, params, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, CHILD, name] + [str(x) for x in params], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_global_row_tier_alone():
    """with the LDS tier switched off every task runs on the global row: the same strings"""
    name, params = "SMALL", (4, 8, 1)
    got = _child(name, params, {"OTG_EDIT_ALIGN_ADAPTIVE_TIERS": "2"})
    assert got["tiers"] == [0, len(fx.input_set(name))]
    _assert_equals_restatement(fx.input_set(name), fx.adaptive_ref(name, params), got["scores"], got["cells"], [c.encode() for c in got["cigs"]])


@pytest.mark.parametrize("params,budget_mb", [(fx.NEVER_CUTS, 1), (fx.DEFAULT, 0)], ids=["10-3000-1-1MB", "10-50-1-0MB"])
def test_small_budget_same_results(params, budget_mb):
    """a small OTG_EDIT_ALIGN_BUDGET_MB cuts MID into several chunks of provenance: 1 MB under parameters that never cut (a task takes
    cells / 4 + 16 (score + 1) bytes of rows, 8 (score + 1) of ranges and its score in operations: close to 4 MB in all), and 0 MB, which
    gives every task a chunk of its own, under the default ones (1 MB in all)"""
    want = fx.adaptive_ref("MID", params)
    if budget_mb:
        assert sum(c // 4 + 16 * (s + 1) + 8 * (s + 1) + s for s, c, _ in want) > 2 * (budget_mb << 20)
    got = _child("MID", params, {"OTG_EDIT_ALIGN_BUDGET_MB": str(budget_mb)})
    _assert_equals_restatement(fx.input_set("MID"), want, got["scores"], got["cells"], [c.encode() for c in got["cigs"]])


def test_adaptive_align_independent_of_batch_order(gpu):
    prs = fx.input_set("SMALL")[:60]
    a = gpu.edit_align_heur_batch(*pair_tasks(prs), AD, *fx.DEFAULT)
    b = gpu.edit_align_heur_batch(*pair_tasks(prs[::-1]), AD, *fx.DEFAULT)
    assert a[1] == b[1][::-1]
    assert a[1] == [o for _, _, o in fx.adaptive_ref("SMALL")[:60]]


def test_strategy_none_is_edit_align_batch(gpu):
    arena, tasks = pair_tasks(fx.input_set("SMALL"))
    s0, c0 = gpu.edit_align_batch(arena, tasks)
    s1, c1, cells = gpu.edit_align_heur_batch(arena, tasks, abi.OTG_HEURISTIC_NONE, want_cells=True)
    assert np.array_equal(s0, s1) and c0 == c1
    assert np.array_equal(cells, gpu.edit_distance_batch(arena, tasks, want_cells=True)[1])
    s2, lens = gpu.edit_align_heur_batch(arena, tasks, abi.OTG_HEURISTIC_NONE, want_cigars=False)
    assert np.array_equal(s0, s2) and lens.tolist() == [len(c) for c in c0]


def test_context_heuristic_untouched(gpu):
    prs = fx.input_set("MID")
    arena, tasks = pair_tasks(prs)
    exact = fx.exact_ref("MID")
    want = fx.adaptive_ref("MID")
    assert any(w[0] != e[0] for w, e in zip(want, exact))         # the two modes' scores differ on this set
    # an adaptive call leaves the default context exact
    gpu.edit_align_heur_batch(arena, tasks, AD, *fx.DEFAULT)
    assert gpu.edit_distance_batch(arena, tasks).tolist() == [e[0] for e in exact]
    # an adaptive context: the exact call still refuses, the named call runs exact and leaves the context adaptive
    gpu.set_heuristic(AD, *fx.DEFAULT)
    try:
        with pytest.raises(Exception) as e:
            gpu.edit_align_batch(arena, tasks)
        assert "exact alignment only" in str(e.value)
        s, c = gpu.edit_align_heur_batch(arena, tasks, abi.OTG_HEURISTIC_NONE)
        assert [(int(a), b) for a, b in zip(s, c)] == list(exact)
        assert gpu.edit_distance_batch(arena, tasks).tolist() == [w[0] for w in want]
        # errors put the context back too
        t2 = tasks.copy()
        t2["endsfree"] = 1
        with pytest.raises(Exception) as e:
            gpu.edit_align_heur_batch(arena, t2, abi.OTG_HEURISTIC_NONE)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "ends-free" in str(e.value)
        assert gpu.edit_distance_batch(arena, tasks).tolist() == [w[0] for w in want]
    finally:
        gpu.set_heuristic(abi.OTG_HEURISTIC_NONE)
    assert gpu.edit_distance_batch(arena, tasks).tolist() == [e[0] for e in exact]


def test_refuses_endsfree_and_negative_parameters(gpu):
    arena, tasks = pair_tasks([(b"ACGTACGT", b"ACGTTACGT")])
    t2 = tasks.copy()
    t2["endsfree"] = 1
    with pytest.raises(Exception) as e:
        gpu.edit_align_heur_batch(arena, t2, AD, *fx.DEFAULT)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "ends-free" in str(e.value)
    for bad in ((-1, 50, 1), (10, -1, 1)):
        with pytest.raises(Exception) as e:
            gpu.edit_align_heur_batch(arena, tasks, AD, *bad)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "negative" in str(e.value)
    with pytest.raises(Exception) as e:
        gpu.edit_align_heur_batch(arena, tasks, 7)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    s, c = gpu.edit_align_heur_batch(arena, tasks, AD, *fx.DEFAULT)
    assert int(s[0]) == 1 and len(c[0]) == 9

"""otg_edit_align_span_batch on the device: WFAlignerEdit(Alignment, MemoryMed)::alignEndsFree / alignEnd2End + getAlignmentScore() +
getAlignmentCigar(), exact and under wfadaptive.  Scores and op strings byte for byte those of the CPU restatement
(tests/edit_align_endsfree_ref.cpp, itself checked against the oracle in test_edit_align_endsfree_host.py); scores and cells those of
otg_edit_distance_batch on the same tasks; both storage tiers run; end-to-end tasks in a mixed batch give what the end-to-end entry
points give; the batch order does not change a result; the length-only and capacity protocol."""
import ctypes as C

import numpy as np
import pytest

from otter_amd import abi
import span_align_fixtures as fx
from helpers import pair_tasks

pytestmark = pytest.mark.gpu

AD = abi.OTG_HEURISTIC_WFADAPTIVE
SETS = ["WIDTHS", "EDGE", "TIES", "FORMS", "WIDE"]
MODES = [None, fx.DEFAULT, fx.OTHER]
CASES = [(n, m) for n in SETS for m in MODES]


def _call(gpu, arena, tasks, params, **kw):
    if params is None:
        return gpu.edit_align_span_batch(arena, tasks, **kw)
    return gpu.edit_align_span_batch(arena, tasks, AD, *params, **kw)


def _chain(gpu, arena, tasks, params):
    """scores and cells of otg_edit_distance_batch on a context set to the heuristic"""
    if params is None:
        return gpu.edit_distance_batch(arena, tasks, want_cells=True)
    gpu.set_heuristic(AD, *params)
    try:
        return gpu.edit_distance_batch(arena, tasks, want_cells=True)
    finally:
        gpu.set_heuristic(abi.OTG_HEURISTIC_NONE)


@pytest.mark.parametrize("name,params", CASES, ids=["%s-%s" % (n, "exact" if m is None else "%d-%d-%d" % m) for n, m in CASES])
def test_span_align_matches_restatement(gpu, name, params):
    cases = fx.input_set(name)
    want = fx.span_ref(name, fx.mode_of(params))
    arena, tasks = pair_tasks(*fx.split(cases))
    scores, cigs, cells = _call(gpu, arena, tasks, params, want_cells=True)
    lds, glb = gpu.edit_align_last_tiers()
    for i, ((p, t, f), (s, c, o)) in enumerate(zip(cases, want)):
        assert int(scores[i]) == s, (i, len(p), len(t), f)
        assert cigs[i] == o, (i, len(p), len(t), f)
        if params is not None:
            assert int(cells[i]) == c, (i, len(p), len(t), f)
    s2, c2 = _chain(gpu, arena, tasks, params)
    assert np.array_equal(scores, s2) and np.array_equal(cells, c2)
    s3, lens = _call(gpu, arena, tasks, params, want_cigars=False)
    assert np.array_equal(s3, scores)
    assert lens.tolist() == [len(c) for c in cigs]
    assert lens.tolist() == [len(p) + o.count(b"I") for (p, _, _), o in zip(cases, cigs)]
    assert lds + glb == len(cases)
    if name == "WIDE":
        # [0] holds 2 201 diagonals at every score (exact) and at score 0 (adaptive): more than the 2 048 of either LDS window
        assert glb >= 1 and lds >= 1
    else:
        assert glb == 0


def test_wide_pair_is_wider_than_the_lds_window():
    """a condition on the input: the region of WIDE[0] is 2 201 diagonals wide at every score, and its op string uses both free ends"""
    p, t, f = fx.input_set("WIDE")[0]
    assert f == (2200, 0, 0, 2200) and len(p) == 2600 and len(t) > 2500
    s, _, ops = fx.span_ref("WIDE")[0]
    assert ops.startswith(b"D" * 2200) and ops.endswith(b"I" * 2200) and s < 100
    assert len(fx.input_set("WIDE")[1][0]) > 32766 and len(fx.input_set("WIDE")[1][1]) > 32766


@pytest.mark.parametrize("params", [None, fx.DEFAULT], ids=["exact", "10-50-1"])
def test_mixed_batch_and_batch_order(gpu, params):
    """end-to-end and ends-free tasks interleaved: the end-to-end ones give what the end-to-end entry points give, the ends-free ones what
    the restatement gives, in either order of the batch"""
    ef = list(fx.input_set("FORMS")[:24]) + list(fx.input_set("TIES")[:12])
    e2e = [(p, t) for p, t, _ in fx.input_set("WIDTHS")[:24]] + [(b"", b""), (b"ACGT", b""), (b"AB", b"BA")]
    pairs, forms, kind = [], [], []
    for i in range(max(len(ef), len(e2e))):
        if i < len(ef):
            pairs.append(ef[i][:2]); forms.append(ef[i][2]); kind.append(("ef", i))
        if i < len(e2e):
            pairs.append(e2e[i]); forms.append(None); kind.append(("e2e", i))
    want_ef = fx.run_span_ref(ef, fx.mode_of(params))
    arena2, tasks2 = pair_tasks(e2e)
    if params is None:
        want_e2e = gpu.edit_align_batch(arena2, tasks2)
    else:
        want_e2e = gpu.edit_align_heur_batch(arena2, tasks2, AD, *params)
    a = _call(gpu, *pair_tasks(pairs, forms), params)
    b = _call(gpu, *pair_tasks(pairs[::-1], forms[::-1]), params)
    assert a[0].tolist() == b[0].tolist()[::-1] and a[1] == b[1][::-1]
    for j, (what, i) in enumerate(kind):
        if what == "ef":
            assert (int(a[0][j]), a[1][j]) == (want_ef[i][0], want_ef[i][2]), (j, i)
        else:
            assert (int(a[0][j]), a[1][j]) == (int(want_e2e[0][i]), want_e2e[1][i]), (j, i)


def _raw(gpu, arena, tasks, strategy, a, b, c, cap):
    n = len(tasks)
    scores, off, ln = np.zeros(n, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    out = np.zeros(max(cap, 1), np.uint8)
    used = C.c_uint64(0)
    rc = gpu._L.otg_edit_align_span_batch(gpu._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(tasks), C.c_uint32(n), C.c_int(strategy),
                                          C.c_int(a), C.c_int(b), C.c_int(c), abi.ptr(scores), abi.ptr(off), abi.ptr(ln), abi.ptr(out),
                                          C.c_uint64(cap), C.byref(used), None)
    return rc, used.value, scores, off, ln, out


@pytest.mark.parametrize("strategy", [abi.OTG_HEURISTIC_NONE, AD], ids=["exact", "wfadaptive"])
def test_capacity_protocol(gpu, strategy):
    cases = fx.input_set("FORMS")[:16]
    want = fx.span_ref("FORMS", fx.mode_of(None if strategy == abi.OTG_HEURISTIC_NONE else fx.DEFAULT))[:16]
    need = sum(len(o) for _, _, o in want)
    arena, tasks = pair_tasks(*fx.split(cases))
    rc, used, _, _, _, _ = _raw(gpu, arena, tasks, strategy, 10, 50, 1, need - 1)
    assert rc == abi.OTG_ERR_CAPACITY and used == need
    rc, used, scores, off, ln, out = _raw(gpu, arena, tasks, strategy, 10, 50, 1, need)
    assert rc == 0 and used == need
    assert [out[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(len(cases))] == [o for _, _, o in want]
    assert scores.tolist() == [s for s, _, _ in want]


def test_parameters_and_context_heuristic(gpu):
    cases = fx.input_set("FORMS")[:30]
    arena, tasks = pair_tasks(*fx.split(cases))
    for bad in ((-1, 50, 1), (10, -1, 1)):
        with pytest.raises(Exception) as e:
            gpu.edit_align_span_batch(arena, tasks, AD, *bad)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "negative" in str(e.value)
    with pytest.raises(Exception) as e:
        gpu.edit_align_span_batch(arena, tasks, 7)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    t2 = tasks.copy()
    t2["pattern_end_free"] = -1
    with pytest.raises(Exception) as e:
        gpu.edit_align_span_batch(arena, t2)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    # the context's own heuristic is neither consulted nor changed
    exact = [w[0] for w in fx.span_ref("FORMS")[:30]]
    tight = (1, 0, 1)
    cut = [w[0] for w in fx.run_span_ref(cases, fx.mode_of(tight))]
    assert cut != exact                                           # (a condition on the inputs)
    s, _ = gpu.edit_align_span_batch(arena, tasks, AD, *tight)
    assert s.tolist() == cut
    assert gpu.edit_distance_batch(arena, tasks).tolist() == exact
    gpu.set_heuristic(AD, *tight)
    try:
        s, _ = gpu.edit_align_span_batch(arena, tasks)
        assert s.tolist() == exact
        assert gpu.edit_distance_batch(arena, tasks).tolist() == cut
    finally:
        gpu.set_heuristic(abi.OTG_HEURISTIC_NONE)

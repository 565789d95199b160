"""The four aligner chains share one device slot of counters (csrc/otg_chain.hpp).  Here they run interleaved in ONE fresh context, starting with
the exact edit chain (which used to create the slot at a smaller size than the others ask for), and every call must return what the session's
context returns for the same input; the region pipeline behind them must return what a context that ran nothing else returns, the visited-cell
statistic of the exact gap-affine tiers included — per run, not accumulated over runs."""
import numpy as np
import pytest
import otter_amd
from helpers import mutate, tr_seq, pair_tasks
from otter_amd import abi, synth

pytestmark = pytest.mark.gpu


def _pairs(rng, n):
    """ONT-like pairs of 200-600 bases; every second one a read that covers only part of its pattern (free ends)"""
    pairs, forms = [], []
    for i in range(n):
        a = tr_seq(rng, int(rng.integers(200, 601)))
        b = mutate(rng, a, 0.07)
        a = mutate(rng, a, 0.07)
        f = None
        if i % 2:
            b = b[:int(len(b) * rng.uniform(0.5, 0.9))] if i % 4 == 1 else b[int(len(b) * rng.uniform(0.1, 0.5)):]
        if len(b) > len(a):
            a, b = b, a
        if i % 2:
            d = len(a) - len(b)
            f = (0, d, 0, 0) if i % 4 == 1 else (d, 0, 0, 0)
        pairs.append((a, b))
        forms.append(f)
    return pairs, forms


def _same_records(a, b):
    assert np.array_equal(a["labels"], b["labels"])
    for k in ("regions", "alleles"):
        assert len(a[k]) == len(b[k])
        for f in a[k].dtype.names:
            assert a[k][f].tobytes() == b[k][f].tobytes(), (k, f)
    n = int(a["alleles"]["seq_len"].sum())
    assert a["seqs"][:n].tobytes() == b["seqs"][:n].tobytes()


def test_chains_interleaved_in_a_fresh_context(gpu):
    rng = np.random.default_rng(77)
    pairs, forms = _pairs(rng, 64)
    arena, tasks = pair_tasks(pairs, forms)
    arena_e2e, tasks_e2e = pair_tasks(pairs)         # the op-string edit aligner is end-to-end only: the same pairs without free ends
    batch = synth.make_batch(8, len_range=(400, 800), n_reads=12, seed=5)
    P = abi.default_params()
    ad = (abi.OTG_HEURISTIC_WFADAPTIVE, 10, 50, 1)

    # what the session's context returns, call by call
    exp = {"edit": gpu.edit_distance_batch(arena, tasks), "affine": gpu.affine_align_batch(arena, tasks),
           "edit_align": gpu.edit_align_batch(arena_e2e, tasks_e2e)}
    gpu.set_heuristic(*ad)
    try:
        exp["ad_edit"] = gpu.edit_distance_batch(arena, tasks)
        exp["ad_affine"] = gpu.affine_align_batch(arena, tasks)
    finally:
        gpu.set_heuristic(abi.OTG_HEURISTIC_NONE)

    def same_alignments(got, want):
        assert np.array_equal(got[0], want[0])
        assert got[1] == want[1]

    with otter_amd.Context(0) as ctx:
        assert np.array_equal(ctx.edit_distance_batch(arena, tasks), exp["edit"])          # first chain of the context: the exact edit one
        ctx.set_heuristic(*ad)
        assert np.array_equal(ctx.edit_distance_batch(arena, tasks), exp["ad_edit"])
        same_alignments(ctx.affine_align_batch(arena, tasks), exp["ad_affine"])
        ctx.set_heuristic(abi.OTG_HEURISTIC_NONE)
        same_alignments(ctx.affine_align_batch(arena, tasks), exp["affine"])
        same_alignments(ctx.edit_align_batch(arena_e2e, tasks_e2e), exp["edit_align"])
        ctx.trim()
        res1 = ctx.assemble(P, batch)
        visited1 = int(ctx.assemble_stats()["affine_visited_cells"])
        res2 = ctx.assemble(P, batch)
        visited2 = int(ctx.assemble_stats()["affine_visited_cells"])
    with otter_amd.Context(0) as alone:
        ref = alone.assemble(P, batch)
        visited_ref = int(alone.assemble_stats()["affine_visited_cells"])

    _same_records(res1, ref)
    _same_records(res2, ref)
    assert visited_ref > 0
    assert visited1 == visited_ref
    assert visited2 == visited1                      # per run: otg_assemble_run zeroes the counter

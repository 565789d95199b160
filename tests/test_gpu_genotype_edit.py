"""GPU parity of the genotype clustering under OTG_GT_METRIC_EDIT (otg_genotype_cluster_metric_batch) against the reference composed from the
oracle's parts (genotype_edit_ref): the matrix bit-exact, gt / gt_l / gt_k / n_gt / reps exact, hsd within 1e-9 relative as test_gpu_genotype.py
compares it, and the number of alignments = the unordered pairs of distinct byte strings per region.  Shapes: the smallest at which each route
can go wrong — A = 0, 1, 2, 3, 7, 40, 103 (103: the first size whose matrices leave LDS) and 257 (the wide kernel)."""
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
from helpers import rand_seq, mutate, tr_seq, pair_tasks
import genotype_edit_ref as ger

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _region(rng, A, lmin, lmax, specials=()):
    """a few distinct TR sequences, each repeated many times, plus near-copies at 0.5-5 % edits (cuts on both sides of 0.025); `specials`
    take the first places"""
    base = [tr_seq(rng, int(rng.integers(lmin, lmax + 1))) for _ in range(int(rng.integers(2, 5)))]
    pool = list(base)
    for rate in (0.005, 0.01, 0.02, 0.03, 0.05):
        pool.append(mutate(rng, base[int(rng.integers(0, len(base)))], rate))
    pool = [s for s in pool if lmin <= len(s) <= lmax] or base
    seqs = list(specials)[:A]
    while len(seqs) < A:
        seqs.append(pool[int(rng.integers(0, len(pool)))])
    return seqs


def _pack(regions):
    arena, off, ln = abi.pack_seqs([s for reg in regions for s in reg])
    counts = np.asarray([len(reg) for reg in regions], dtype=np.uint32)
    first = (np.cumsum(counts) - counts).astype(np.uint32)
    return arena, off, ln, first, counts


def _mixed_regions(two_empty=True):
    rng = np.random.default_rng(7301)
    m10, m20, m40 = ger.motif_order_pair(10), ger.motif_order_pair(20), ger.motif_order_pair(40)
    cased = tr_seq(rng, 90)
    long_a = rand_seq(rng, 17000)
    long_b = mutate(rng, long_a, 0.01)              # about 17 kb at 1 % divergence: beyond the 16 384-row bit-parallel tiers
    return [
        [],
        _region(rng, 1, 40, 300),
        list(m20),
        [m40[0], m40[1], m40[0]],
        _region(rng, 7, 40, 300, specials=[b"", m10[0], b"A", m10[1]]),
        _region(rng, 40, 40, 300, specials=[b"", b"A", b"N", cased, cased.lower(), m20[0], m20[1], b"N", b"A"]),
        _region(rng, 103, 40, 300, specials=[m40[1], m40[0]]),
        [long_a, long_b, long_a],
        _region(rng, 2, 40, 300),
        [b"", b""] if two_empty else [b"", b"C"],      # two empty alleles are equal (their length ratio is 0 / 0: not for the length metric)
    ]


def _wide_regions():
    rng = np.random.default_rng(7302)
    m10 = ger.motif_order_pair(10)
    return [_region(rng, 257, 40, 120, specials=[m10[0], b"", m10[1]]), _region(rng, 3, 40, 120)]


_cache = {}


def _case(name):
    """(args, expected tuple, expected matrix, expected alignments) of a batch, computed once"""
    if name not in _cache:
        regions = _wide_regions() if name == "wide" else _mixed_regions(two_empty=name == "mixed")
        args = _pack(regions)
        mats, n_pairs = ger.edit_matrices(regions)
        exp = ger.genotype_with_matrix(abi.default_params(), *args, mats)
        _cache[name] = (args, exp, np.concatenate(mats + [np.zeros(0)]), n_pairs)
    return _cache[name]


def _compare(got, exp, dist, n_pairs):
    assert got[6].shape == dist.shape and np.array_equal(got[6], dist), "dist: %d of %d differ" % (int((got[6] != dist).sum()), dist.size)
    for i, name in ((0, "gt"), (1, "gt_l"), (2, "gt_k"), (4, "n_gt"), (5, "reps")):
        assert np.array_equal(got[i], exp[i]), name
    assert np.allclose(got[3], exp[3], rtol=1e-9, atol=0, equal_nan=True)
    assert got[7] == n_pairs


def test_mixed_batch(gpu, oracle):
    args, exp, dist, n_pairs = _case("mixed")
    got = gpu.genotype_cluster_metric_batch(abi.default_params(), *args, metric="edit")
    _compare(got, exp, dist, n_pairs)
    # the motif-order pairs are two genotypes here and one under the length metric
    ln = gpu.genotype_cluster_metric_batch(abi.default_params(), *_case("mixed_for_length")[0], metric="length")
    assert got[4][2] == 2 and ln[4][2] == 1
    assert got[4][3] == 2 and ln[4][3] == 1
    # the keyword of the old entry gives the same tuple
    kw = gpu.genotype_cluster_batch(abi.default_params(), *args, metric="edit")
    assert len(kw) == 6 and all(np.array_equal(kw[i], got[i], equal_nan=True) for i in range(6))


def test_wide_region(gpu, oracle):
    args, exp, dist, n_pairs = _case("wide")
    _compare(gpu.genotype_cluster_metric_batch(abi.default_params(), *args, metric="edit"), exp, dist, n_pairs)


def test_cluster_wide_switch(gpu):
    """every region on the wide kernels (OTG_CLUSTER_WIDE=1, read once per process): the two tests above in a child process"""
    gpu.trim()
    env = dict(os.environ, OTG_CLUSTER_WIDE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_genotype_edit.py::test_mixed_batch", "tests/test_gpu_genotype_edit.py::test_wide_region"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])


def test_length_metric_is_the_old_entry(gpu, oracle):
    args = _case("mixed_for_length")[0]
    P = abi.default_params()
    old = gpu.genotype_cluster_batch(P, *args)
    new = gpu.genotype_cluster_metric_batch(P, *args, metric="length")
    for i in range(6):
        assert np.array_equal(old[i], new[i], equal_nan=True), i
    _, tr = gpu.genotype_cluster_trace_batch(P, *args)
    assert np.array_equal(new[6], tr["dl"])
    assert new[7] == 0
    e = oracle.genotype_cluster_batch(P, *args)
    for i in (0, 1, 2, 4, 5):
        assert np.array_equal(new[i], e[i]), i


def test_bad_metric_and_times(gpu):
    args = _case("wide")[0]
    with pytest.raises(otter_amd.OtterGpuError, match=r"\(-2\).*unknown genotype metric 5"):
        gpu.genotype_cluster_metric_batch(abi.default_params(), *args, metric=5)
    gpu.genotype_cluster_metric_batch(abi.default_params(), *args, metric="edit")
    a, c = gpu.genotype_metric_last_ms()
    assert a > 0 and c > 0 and abs((a + c) - gpu.last_kernel_ms()) < 1e-6 * max(1.0, a + c)
    gpu.genotype_cluster_metric_batch(abi.default_params(), *args, metric="length")
    a, c = gpu.genotype_metric_last_ms()
    assert a == 0 and c > 0


def test_exact_under_an_adaptive_context(oracle):
    """a context set to wfadaptive(10, 50, 1) gives the exact matrix, and is still adaptive afterwards"""
    rng = np.random.default_rng(7303)
    pairs = []
    for i in range(48):                 # two noisy reads of one tandem repeat: the adaptive cut costs score on a few of them
        t = tr_seq(rng, int(rng.integers(800, 3000)))
        a, b = mutate(rng, t, 0.12), mutate(rng, t, 0.12)
        pairs.append((a, b) if len(a) >= len(b) else (b, a))
    arena, tasks = pair_tasks(pairs)
    try:
        oracle.set_heuristic(1, 10, 50, 1)
        ad, ad_cells = oracle.edit_distance_batch(arena, tasks, want_cells=True)
    finally:
        oracle.set_heuristic(0)
    ex = oracle.edit_distance_batch(arena, tasks)
    assert (ad > ex).any()
    args, exp, dist, n_pairs = _case("mixed")
    with otter_amd.Context(0) as ctx:
        ctx.set_heuristic(abi.OTG_HEURISTIC_WFADAPTIVE, 10, 50, 1)
        _compare(ctx.genotype_cluster_metric_batch(abi.default_params(), *args, metric="edit"), exp, dist, n_pairs)
        got, cells = ctx.edit_distance_batch(arena, tasks, want_cells=True)
        assert np.array_equal(got, ad) and np.array_equal(cells, ad_cells)

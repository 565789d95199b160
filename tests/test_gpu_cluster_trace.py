"""GPU: the FP64 intermediates of cluster_kernel (otg_cluster_trace_batch) against the reference's own objects, bit for bit: raw KDE
densities (ref_kde_f on the launcher's grid), their sequential normalisation (== the oracle's find_clustering_dist dens_out), the window
sums, the extrema (ref_kde_maximas), the bandwidth, the decision (err, do_hclust, dist_final), the merge matrix and heights
(ref_hclust_average), the first cut (ref_cutree_cdist), cut_k and recut.  Doubles compare as uint64, NaN == NaN.  The traced call's labels /
ic / fc / bounds must equal the product call's.

The densities equal the reference's only where the host libm is the exp() build the device mirrors: when the context's probe reports
mismatches, the comparison starts from the numpy restatement of the KDE loop in the context's variant instead, and the test ends in a skip
whose reason carries the count.  The comparison of the device with the restatement in BOTH variants (test_both_exp_variants) always runs.

Error codes 1-5: the oracle run over these generators and the degenerate matrices (and over helpers.cluster_cases for 40 seeds, both
bandwidths, radius 4 and 8) ends in none of them, so no error path is compared here: none was found.  A region's `err` is still compared
with the oracle's for every region below."""
import numpy as np
import pytest
import otter_amd
from otter_amd import abi
from helpers import cluster_cases, pack_cluster_cases
import cluster_trace_ref as R

pytestmark = pytest.mark.gpu
NG = R.GRID.size
FILL64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _recut_expected(P, n, lens, labels_first):
    """the coverage test of otter_hclust (src/otterclust.cpp:187-212) on the first cut: 1 when cutree_k(max_alleles) replaces the labels"""
    if P.max_alleles == 0:
        return 0
    k = int(labels_first.max()) + 1
    cnt = np.bincount(labels_first, minlength=k)
    maxsz = np.array([int(lens[labels_first == q].max()) for q in range(k)])
    c1, c2 = int(n * P.min_cov_fraction + 0.5), int(n * P.min_cov_fraction2_f + 0.5)
    req = np.where(maxsz < P.min_cov_fraction2_l, c1, c2)
    seeds = int((cnt >= req).sum())
    return int(seeds == 0 or seeds > P.max_alleles)


def _run(gpu, oracle, cases, variant=-1, restated=None, **kw):
    """one traced batch against its expectations; returns the per-region state rows.  restated = v: expectations from the numpy
    restatement of the KDE loop with exp variant v (no oracle decision bound: the device's is used for the clustering part)."""
    P = abi.default_params(**kw)
    packed = pack_cluster_cases(cases)
    len_off = packed[3]
    labels, ic, fc, bounds, tr = gpu.cluster_trace_batch(P, *packed, exp_variant=variant)
    libm_ok = gpu.exp_probe_mismatches == 0
    if restated is None:
        pl, pic, pfc, pb = gpu.cluster_batch(P, *packed)                  # the product instantiation computes the same
        assert np.array_equal(pl, labels) and np.array_equal(pic, ic) and np.array_equal(pfc, fc) and _same(pb, bounds)
        if not libm_ok:
            restated = gpu.exp_variant
    for r, (d, lens) in enumerate(cases):
        n, st, l0 = len(lens), dict(zip(otter_amd._lib.TRACE_STATE, tr["state"][r].tolist())), int(len_off[r])
        raw = None if restated is None else (R.raw_density_restated(R.bandwidth_of(P, lens), d, restated) if n > 2 and P.max_alleles != 1 else None)
        E = R.expected_region(P, d, lens, raw=raw)
        assert st["evaluated"] == E["evaluated"] and st["n_grid"] == NG, (r, st)
        if not E["evaluated"]:      # n <= 2 or max_alleles == 1: nothing else is written
            assert [st[k] for k in ("n_max", "n_min", "do_hclust", "err", "cut_k", "recut")] == [-1] * 6, (r, st)
            assert (_bits(tr["dens_raw"][r]) == FILL64).all() and (_bits(tr["scalars"][r]) == FILL64).all()
            continue
        for name in ("dens_raw", "dens", "sums"):
            assert _same(tr[name][r][:NG], E[name]), (r, n, name, np.flatnonzero(_bits(tr[name][r][:NG]) != _bits(E[name]))[:5])
            assert (_bits(tr[name][r][NG:]) == FILL64).all()
        assert st["n_max"] == len(E["max"]) and st["n_min"] == len(E["min"]), (r, st, len(E["max"]), len(E["min"]))
        for key, mi, mv in (("max", "max_i", "max_v"), ("min", "min_i", "min_v")):
            k = len(E[key])
            assert tr[mi][r][:k].tolist() == [q[0] for q in E[key]], (r, key)
            assert _same(tr[mv][r][:k], [q[1] for q in E[key]]), (r, key)
        assert tr["scalars"][r][0] == E["bandwidth"]
        if "err" in E:
            assert st["err"] == E["err"], (r, st, E["err"])
            if E["err"] == 0:
                assert _same(bounds[r], E["bounds"]), (r, bounds[r], E["bounds"])
        if st["err"]:
            assert ic[r] == 0 and fc[r] == 0 and (labels[l0:l0 + n] == -1).all()
            continue
        b0, b1, bc = (float(v) for v in bounds[r])
        do_hclust = int(not (b1 - b0 <= P.max_error))
        assert st["do_hclust"] == do_hclust, (r, st, bounds[r])
        if not do_hclust:
            assert _bits(tr["scalars"][r][1:2])[0] == FILL64 and st["cut_k"] == -1 and st["recut"] == -1
            assert (labels[l0:l0 + n] == 0).all() and ic[r] == 1 and fc[r] == 1
            continue
        dist_final = b1 if b1 == E["bandwidth"] else bc + 0.0025
        assert _same(tr["scalars"][r][1:2], [dist_final])
        merge, height, first = R.expected_clustering(n, d, dist_final)
        assert np.array_equal(tr["merge"][2 * l0:2 * l0 + 2 * (n - 1)], merge), (r, n)
        assert _same(tr["height"][l0:l0 + n - 1], height), (r, n)
        assert np.array_equal(tr["labels_first"][l0:l0 + n], first), (r, n)
        reach = np.flatnonzero(height >= dist_final)
        assert st["cut_k"] == n - (int(reach[0]) if reach.size else n - 1), (r, st)
        assert st["recut"] == _recut_expected(P, n, lens, first), (r, st)
    if restated is None or variant == -1:
        rc, el, eic, efc, eb = oracle.cluster_batch(P, *packed)
        if libm_ok:
            assert rc == 0 and np.array_equal(labels, el) and np.array_equal(ic, eic) and np.array_equal(fc, efc) and _same(bounds, eb)
    if not libm_ok and variant == -1:
        pytest.skip("density-versus-libm comparison skipped: the host libm differs from the chosen exp variant on %d probe arguments "
                    "(compared with the numpy restatement instead)" % gpu.exp_probe_mismatches)
    return tr["state"]


def _lens(rng, n, long):
    return (rng.integers(500, 3000, n) if long else rng.integers(100, 500, n)).astype(np.uint32)


def test_storage_paths(gpu, oracle):
    """n = 0, 1, 2 (not evaluated), 3 (the smallest KDE), 64 (2 016 pairs: the last matrix clustered in LDS), 65 (the first in HBM), 256 and
    257 (the last narrow and the first wide region) in one batch; two groups, so that every region from 64 up reaches hclust."""
    rng = np.random.default_rng(71)
    cases = []
    for n in (0, 1, 2, 3, 64, 65, 256, 257):
        cases.append((R.two_groups(rng, n) if n > 1 else np.zeros(0), _lens(rng, n, n % 2 == 0)))
    st = _run(gpu, oracle, cases)
    assert st[:3, 0].tolist() == [0, 0, 0] and st[3:, 0].tolist() == [1] * 5
    assert st[4:, 4].tolist() == [1] * 4          # do_hclust at 64, 65, 256, 257


def _structure_cases(rng):
    n = 33
    npair = n * (n - 1) // 2
    far = R.two_groups(rng, n, sep=0.38, base=0.0, noise=0.01)       # z = 38 between the groups: exp() returns subnormals
    on_grid = R.GRID[rng.integers(0, 160, npair)].copy()                 # y = x - d is exactly 0 at a grid point
    quant = np.round(rng.random(npair) * 0.4, 2)                         # ties in the NN-chain
    return [("far groups", far, False), ("all 0.0", np.zeros(npair), False), ("all 0.2", np.full(npair, 0.2), True),
            ("all 2.0", np.full(npair, 2.0), False), ("on grid", on_grid, True), ("quantised", quant, False),
            ("quantised long", np.round(R.two_groups(rng, 65), 2), True), ("short reads", R.two_groups(rng, n), False),
            ("long reads", R.two_groups(rng, n), True)]


def test_structure(gpu, oracle):
    """Subnormal exp() results, all-equal distances (0.0, 0.2), densities exactly 0 (then 0/0), distances on grid points, quantised
    distances, both bandwidths."""
    rng = np.random.default_rng(72)
    sc = _structure_cases(rng)
    cases = [(d, _lens(rng, int(round((1 + (1 + 8 * d.size) ** 0.5) / 2)), long)) for _, d, long in sc]
    st = _run(gpu, oracle, cases)
    names = [q[0] for q in sc]
    # the inputs do what they are here for
    far = sc[0][1]
    z = (R.GRID[:, None] - far[None, :]) / 0.01
    e = otter_amd.exp_host(-(z * z / 2), 1)
    assert ((e > 0) & (e < 2.2250738585072014e-308)).any()
    assert st[names.index("all 2.0")][4] == 0 and st[names.index("far groups")][4] == 1


def test_all_2_is_nan_after_normalisation(gpu, oracle):
    """all distances 2.0: every density exactly 0, the normalised ones 0/0 — the same NaNs as the reference, and no clustering"""
    n = 12
    P = abi.default_params()
    cases = [(np.full(n * (n - 1) // 2, 2.0), np.full(n, 300, dtype=np.uint32))]
    _, _, _, _, tr = gpu.cluster_trace_batch(P, *pack_cluster_cases(cases))
    assert (tr["dens_raw"][0][:NG] == 0.0).all() and np.isnan(tr["dens"][0][:NG]).all()
    _run(gpu, oracle, cases)


def test_radius_8(gpu, oracle):
    """max_error 0.02: a window radius of 8 instead of 4, and another do_hclust threshold"""
    rng = np.random.default_rng(73)
    cases = [(R.two_groups(rng, 40), _lens(rng, 40, False)), (R.two_groups(rng, 65, sep=0.015, base=0.1, noise=0.004), _lens(rng, 65, True))]
    cases += cluster_cases(rng, 18)
    assert R.radius_of(abi.default_params(max_error=0.02)) == 8
    _run(gpu, oracle, cases, max_error=0.02)


def test_decision_bound_branches(gpu, oracle):
    """helpers.cluster_cases at 90 regions: unimodal, bimodal, many maxima (the sort of more than 16), singleton-only, outlier repair"""
    rng = np.random.default_rng(74)
    st = _run(gpu, oracle, cluster_cases(rng, 90))
    ev = st[st[:, 0] == 1]
    assert (ev[:, 2] == 1).any() and (ev[:, 2] == 2).any() and (ev[:, 2] > 16).any() and (ev[:, 7] == 1).any() and (ev[:, 7] == 0).any()


def _variant_cases():
    """n = 3, 64, 65 with two groups, and 120 regions of three reads: with three terms per density a last-place difference between the two
    exp() variants reaches the sum (at V = 64 the rounding of the 2 016-term sum swallows it)"""
    rng = np.random.default_rng(75)
    cases = [(R.two_groups(rng, n), _lens(rng, n, n == 64)) for n in (3, 64, 65)]
    return cases + [(rng.random(3) * 0.3, _lens(rng, 3, False)) for _ in range(120)]


@pytest.mark.parametrize("variant", [1, 0], ids=["fma", "nofma"])
def test_both_exp_variants(gpu, oracle, variant):
    """cluster_kernel<FMA> and cluster_kernel<non-FMA> at n = 3, 64, 65 against the numpy restatement of the KDE loop with exp() from
    otg_exp_host(variant): densities, normalisation, window sums, extrema; merges, heights and the first cut at the device's cut height."""
    cases = _variant_cases()
    st = _run(gpu, oracle, cases, variant=variant, restated=variant)
    assert st[1:3, 4].tolist() == [1, 1]
    if variant == gpu.exp_variant and gpu.exp_probe_mismatches == 0:      # the restatement itself, against the reference's KDE::f
        for d, lens in cases:
            h = R.bandwidth_of(abi.default_params(), lens)
            assert _same(R.raw_density_restated(h, d, variant), R.raw_density_reference(h, d))


def test_variants_differ_in_the_densities(gpu, oracle):
    """the two instantiations are different kernels: on the cases above their raw densities differ somewhere, in the last place — as the two
    restatements' do"""
    cases = _variant_cases()
    P = abi.default_params()
    a = gpu.cluster_trace_batch(P, *pack_cluster_cases(cases), exp_variant=1)[4]["dens_raw"][:, :NG]
    b = gpu.cluster_trace_batch(P, *pack_cluster_cases(cases), exp_variant=0)[4]["dens_raw"][:, :NG]
    differ = (_bits(a) != _bits(b)).any(axis=1)
    want = [bool((_bits(R.raw_density_restated(0.01, d, 1)) != _bits(R.raw_density_restated(0.01, d, 0))).any()) for d, lens in cases[3:]]
    assert differ[3:].tolist() == want and sum(want) >= 3
    assert np.allclose(a, b, rtol=1e-12, atol=0)

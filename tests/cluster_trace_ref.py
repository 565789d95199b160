"""Expected values for the trace of cluster_kernel (tests/test_gpu_cluster_trace.py), region by region, from the reference's own objects
(oracle/_ref through oracle_lib, which="ref"; the oracle's restatement of the same functions where that build is absent) plus the oracle's
find_clustering_dist for the decision bound and its error code.  What the reference does not expose is restated here operation for operation:
the normalisation (sequential), the window sums of KDE::maximas, and — for the exp variant the host libm does not run — the KDE loop itself
with exp() from otg_exp_host."""
import math
import numpy as np
import otter_amd
import oracle_lib

DINTERVAL = 0.0025


def source():
    return "ref" if oracle_lib.ref() is not None else "oracle"


def kde_grid():
    """the grid of otg_launch_cluster (src/otterclust.cpp:26): repeated x += 0.0025 from 0 while x <= 1"""
    g, x = [], 0.0
    while x <= 1.0:
        g.append(x)
        x += DINTERVAL
    return np.array(g)


GRID = kde_grid()


def seq_sum(v):
    """left-to-right sum (np.sum is pairwise)"""
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1]) if len(v) else 0.0


def bandwidth_of(P, lens):
    return P.bandwidth_long if (np.asarray(lens).astype(np.int64) >= P.bandwidth_length).any() else P.bandwidth_short


def radius_of(P):
    return max(1, int(P.max_error / DINTERVAL))


def raw_density_reference(h, d):
    """KDE::f at every grid point, by the reference's own object"""
    src = source()
    return np.array([oracle_lib.kde_f(h, d, float(x), which=src) for x in GRID])


def raw_density_restated(h, d, variant):
    """the KDE loop of cluster_kernel / KDE::f (src/ankde.cpp:8-23) in numpy: same operations, same (sequential) order, exp() of `variant`"""
    inv_sqrt_2pi = 1 / math.sqrt(2 * 3.14159265358979323846)
    inv_h = 1 / h
    z = (GRID[:, None] - d[None, :]) / h
    e = otter_amd.exp_host(-(z * z / 2), variant).reshape(z.shape)
    terms = inv_h * (inv_sqrt_2pi * e)
    total = np.cumsum(terms, axis=1)[:, -1]          # 0.0 + t0 + t1 + ...: cumsum is sequential
    return total / float(d.size)


def window_sums(dens, radius):
    """KDE::maximas' window sums (src/ankde.cpp:25-40): the centre, then the left neighbours outwards, then the right ones"""
    n = dens.size
    out = np.empty(n)
    for i in range(n):
        s = 0.0
        s += dens[i]
        for j in range(1, radius):
            if i - j >= 0:
                s += dens[i - j]
        for j in range(1, radius):
            if i + j < n:
                s += dens[i + j]
        out[i] = s
    return out


def expected_region(P, d, lens, raw=None):
    """dict of the expected trace of one region.  `raw`: the raw densities to start from (default: the reference's KDE::f).  With the
    default, `dens` is also checked against the oracle's find_clustering_dist, whose bounds and error code are returned."""
    n = len(lens)
    E = {"n": n, "evaluated": int(not (n <= 2 or P.max_alleles == 1))}
    if not E["evaluated"]:
        return E
    src = source()
    h = bandwidth_of(P, lens)
    radius = radius_of(P)
    from_ref = raw is None
    if from_ref:
        raw = raw_density_reference(h, d)
    with np.errstate(invalid="ignore", divide="ignore"):
        dens = raw / seq_sum(raw)
    E.update(bandwidth=h, dens_raw=raw, dens=dens, sums=window_sums(dens, radius))
    mx, mn = oracle_lib.kde_maximas(dens, radius, which=src)
    E["max"], E["min"] = mx, mn
    if from_ref:
        err, b, odens = oracle_lib.find_clustering_dist(d, h, radius, DINTERVAL)
        assert odens.size == dens.size and np.array_equal(odens.view(np.uint64), dens.view(np.uint64)), "oracle dens_out != normalised ref_kde_f"
        E["err"], E["bounds"] = err, b
    return E


def expected_clustering(n, d, dist_final):
    """merge, height and the first cut's labels for a region that reaches hclust, at the given cut height"""
    src = source()
    merge, height = oracle_lib.hclust_average(n, np.array(d, dtype=np.float64), which=src)
    labels = oracle_lib.cutree_cdist(n, merge, height, dist_final, which=src)
    return merge, height, labels


def two_groups(rng, n, sep=0.2, base=0.13, noise=0.03):
    g = np.arange(n) % 2
    rng.shuffle(g)
    full = np.abs(g[:, None] - g[None, :]) * sep + base + rng.random((n, n)) * noise
    return np.ascontiguousarray(full[np.triu_indices(n, 1)])

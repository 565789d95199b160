"""GPU parity away from the reference's CLI defaults: the region pipeline, the realign-only path, cluster_kernel and genotype_kernel under the
user options `-F -A -e -h -f -s` of otter_assemble and `-E -S` of otter_cohort, against the CPU oracle under the same parameters.

Every comparison is the one the default-parameter tests make (run_against of test_gpu_pipeline.py with its stats fields, the field list of
test_realign_only_reads, _compare of test_gpu_cluster.py, _check of test_gpu_genotype.py, _compare of test_gpu_genotype_edit.py), with their
tolerances: integers, labels, sequences bit-exact, `se` within 1e-6 absolute, `hsd` within 1e-9 relative.

Every value swept also carries a liveness condition, stated on the ORACLE's outputs only: the oracle's result at that value differs from the
oracle's result at the defaults in at least one region (one read on the realign-only path, one case for cluster_kernel).  A value that moves
nothing tests nothing.  Regions of the oracle's result that differ from the defaults, measured when the tests were written:

    parameters                                  ont (of 24)   hifi (of 40)   realign (of 30)
    mismatch, gap_open, gap_ext = 3, 5, 1            24             -              -
    = 6, 2, 3                                        24             -              6
    = 1, 0, 1                                        24             -             18
    bandwidth_long = 0.05                            11             3              4
    bandwidth_short = 0.03                            -             2              1
    bandwidth_length = 100000                         2             -              -
    max_error = 0.03 / 0.005                        7 / 3         3 / 2          3 / 1
    min_cov_fraction = 0.45                           3             3              3
    min_cov_fraction2_l, _f = 200, 0.45              14            10             10
    min_sim = 0.5 / 0.99                           16 / 13        - / 4         24 / 21
    flank = 50 / 80 / 150                             -             -          4 / 4 / 21
    min_sim = 0.7 / 0.8                               -             -           16 / 12
(a dash: the value moves nothing on that batch and is not run there).  The tests print the counts they see."""
import numpy as np
import pytest
from otter_amd import abi, synth
from helpers import cluster_cases, pack_cluster_cases
from test_gpu_pipeline import run_against
from test_gpu_cluster import _compare as cluster_compare
from test_gpu_genotype import _regions as genotype_regions, _check as genotype_check
from test_gpu_genotype_edit import _compare as genotype_edit_compare
import genotype_edit_ref as ger

pytestmark = pytest.mark.gpu

# ---- the three batches; `base`: what every run of the batch sets besides the value under test
BATCHES = {
    "ont": (lambda: synth.make_batch(24, len_range=(400, 1200), n_reads=20, err="ont", seed=4, frac_partial=0.2), {}),
    "hifi": (lambda: synth.make_batch(40, len_range=(200, 900), n_reads=14, err="hifi", frac_partial=0.3, seed=3, reads_range=(1, 20)), {}),
    "realign": (lambda: synth.make_batch(30, len_range=(300, 900), n_reads=16, err="hifi", realign=True, seed=6), {"realign": 1}),
}


def _pen(x, o, e):
    return {"mismatch": x, "gap_open": o, "gap_ext": e}


MCF2 = {"min_cov_fraction2_l": 200, "min_cov_fraction2_f": 0.45}
SWEEP = [
    ("ont", _pen(3, 5, 1)), ("ont", _pen(6, 2, 3)), ("ont", _pen(1, 0, 1)), ("realign", _pen(6, 2, 3)), ("realign", _pen(1, 0, 1)),
    ("ont", {"bandwidth_long": 0.05}), ("hifi", {"bandwidth_long": 0.05}), ("realign", {"bandwidth_long": 0.05}),
    ("hifi", {"bandwidth_short": 0.03}), ("realign", {"bandwidth_short": 0.03}),
    ("ont", {"bandwidth_length": 100000}),
    ("ont", {"max_error": 0.03}), ("hifi", {"max_error": 0.03}), ("realign", {"max_error": 0.03}),
    ("ont", {"max_error": 0.005}), ("hifi", {"max_error": 0.005}), ("realign", {"max_error": 0.005}),
    ("ont", {"min_cov_fraction": 0.45}), ("hifi", {"min_cov_fraction": 0.45}), ("realign", {"min_cov_fraction": 0.45}),
    ("ont", MCF2), ("hifi", MCF2), ("realign", MCF2),
    ("ont", {"min_sim": 0.5}), ("realign", {"min_sim": 0.5}),
    ("ont", {"min_sim": 0.99}), ("hifi", {"min_sim": 0.99}), ("realign", {"min_sim": 0.99}),
    ("realign", {"flank": 50}), ("realign", {"flank": 80}), ("realign", {"flank": 150}),
    ("realign", {"min_sim": 0.7}), ("realign", {"min_sim": 0.8}),
]
# two parameters at once: the kernels' argument lists are long and positional, and two values swapped at a launch site go unnoticed
# while both hold a default
PAIRS = [
    ("realign", dict(_pen(6, 2, 3), min_sim=0.8, flank=80)),
    ("ont", {"max_error": 0.03, "bandwidth_long": 0.05, "min_cov_fraction": 0.45}),
    ("hifi", {"max_error": 0.03, "bandwidth_short": 0.03, "min_cov_fraction": 0.45}),
]
# the realign-only path (otg_assemble_realign): the rows that decide which reads are rescued and where they are cut.  Reads of the oracle's
# result that differ from the defaults / reads rescued (42 at the defaults): 6,2,3: 7 / 39; 1,0,1: 33 / 9; flank 50, 80: 4 / 46; 150: 42 / 0;
# min_sim 0.5, 0.7, 0.8: 4 / 46; 0.99: 36 / 6; the set of three: 5 / 46.  (3,5,1 moves no read of this batch and is not run.)
REALIGN_SWEEP = [_pen(6, 2, 3), _pen(1, 0, 1), {"flank": 50}, {"flank": 80}, {"flank": 150}, {"min_sim": 0.5}, {"min_sim": 0.7},
                 {"min_sim": 0.8}, {"min_sim": 0.99}, dict(_pen(6, 2, 3), min_sim=0.8, flank=80)]


def _id(kw):
    return ",".join("%s=%s" % (k.replace("min_cov_fraction", "mcf").replace("bandwidth", "bw"), v) for k, v in kw.items())


_batches, _oracle_runs, _oracle_reads = {}, {}, {}


def _batch(name):
    if name not in _batches:
        _batches[name] = BATCHES[name][0]()
    return _batches[name]


def _params(name, kw):
    return abi.default_params(**dict(BATCHES[name][1], **kw))


def _oracle_run(oracle, name, kw):
    """The oracle's pipeline result for batch `name` under `kw`: computed once per process, never modified."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _oracle_runs:
        _oracle_runs[key] = oracle.assemble_batch(_params(name, kw), _batch(name))
    return _oracle_runs[key]


def _region_records(res, batch):
    """Per region, everything the pipeline reports about it, as one comparable value."""
    out = []
    for r, reg in enumerate(batch["regions"]):
        g = res["regions"][r]
        f, n = int(reg["first_read"]), int(reg["n_reads"])
        al = res["alleles"][int(g["first_allele"]):int(g["first_allele"]) + int(g["n_alleles"])]
        out.append((tuple(int(g[k]) for k in ("status", "ic", "fc", "n_valid", "n_alleles")), res["labels"][f:f + n].tobytes(),
                    tuple((int(a["label"]), int(a["scov"]), int(a["acov"]), int(a["tcov"]), int(a["ic"]), int(a["ps"]), int(a["hp"]), float(a["se"]),
                           res["seqs"][int(a["seq_off"]):int(a["seq_off"]) + int(a["seq_len"])].tobytes()) for a in al)))
    return out


def regions_moved(oracle, name, kw):
    """Liveness of a sweep value: how many regions of the ORACLE's result under `kw` differ from the ORACLE's result at the defaults."""
    b = _batch(name)
    at_default, at_value = _region_records(_oracle_run(oracle, name, {}), b), _region_records(_oracle_run(oracle, name, kw), b)
    return sum(1 for x, y in zip(at_default, at_value) if x != y)


def _run_case(gpu, oracle, name, kw):
    moved = regions_moved(oracle, name, kw)
    print("%s, %s: %d of %d regions of the oracle's result differ from the defaults" % (name, _id(kw), moved, len(_batch(name)["regions"])))
    assert moved >= 1, (name, kw)
    return run_against(gpu, _params(name, kw), _batch(name), _oracle_run(oracle, name, kw))


@pytest.mark.parametrize("name,kw", SWEEP, ids=["%s-%s" % (n, _id(k)) for n, k in SWEEP])
def test_pipeline_single_parameter(gpu, oracle, name, kw):
    _run_case(gpu, oracle, name, kw)


@pytest.mark.parametrize("name,kw", PAIRS, ids=["%s-%s" % (n, _id(k)) for n, k in PAIRS])
def test_pipeline_parameters_together(gpu, oracle, name, kw):
    """Several parameters off their defaults in one run; the result also differs from the oracle's under each of them alone (on the
    oracle), so that no value of the set can stand in for another."""
    _run_case(gpu, oracle, name, kw)
    b = _batch(name)
    together = _region_records(_oracle_run(oracle, name, kw), b)
    groups = [{k: v for k, v in kw.items() if k in _pen(0, 0, 0)}] + [{k: v} for k, v in kw.items() if k not in _pen(0, 0, 0)]
    for alone in (g for g in groups if g):
        assert together != _region_records(_oracle_run(oracle, name, alone), b), alone


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_pipeline_defaults_after_other_parameters(gpu, oracle, name):
    """No state carried from run to run: behind a run with every swept parameter off its default (and behind the sweeps above, when the
    module runs whole), the defaults give the oracle's default result on the same context."""
    far = dict(_pen(1, 0, 1), bandwidth_long=0.05, bandwidth_short=0.03, bandwidth_length=700, max_error=0.03, min_cov_fraction=0.45, min_sim=0.7, flank=80, **MCF2)
    gpu.assemble(_params(name, far), _batch(name))
    run_against(gpu, _params(name, {}), _batch(name), _oracle_run(oracle, name, {}))


READ_FIELDS = ("seq_off", "seq_len", "spanning_l", "spanning_r", "ps", "hp", "ccoord_first", "ccoord_second")


def _oracle_realign(oracle, kw):
    key = tuple(sorted(kw.items()))
    if key not in _oracle_reads:
        _oracle_reads[key] = oracle.realign_batch(_params("realign", kw), _batch("realign"))
    return _oracle_reads[key]


@pytest.mark.parametrize("kw", REALIGN_SWEEP, ids=[_id(k) for k in REALIGN_SWEEP])
def test_realign_only_parameters(gpu, oracle, kw):
    """otg_assemble_realign alone under the penalties, `flank` and `min_sim`: K_realign_apply's integer running score and its
    `best / flank >= min_sim` against local_realignment's.  Liveness: the oracle's descriptors differ from its defaults' in some read."""
    b = _batch("realign")
    exp, at_default = _oracle_realign(oracle, kw), _oracle_realign(oracle, {})
    moved = int(np.count_nonzero(np.any([exp[f] != at_default[f] for f in READ_FIELDS], axis=0)))
    rescued = int(np.count_nonzero((exp["seq_len"] != b["reads"]["seq_len"]) | (exp["seq_off"] != b["reads"]["seq_off"])))
    print("realign only, %s: %d reads of the oracle's result differ from the defaults, %d reads rescued" % (_id(kw), moved, rescued))
    assert moved >= 1, kw
    got = gpu.realign_reads(_params("realign", kw), b)
    for f in READ_FIELDS:
        assert np.array_equal(got[f], exp[f]), (f, np.flatnonzero(got[f] != exp[f])[:8].tolist())
    # and the defaults behind it
    got = gpu.realign_reads(_params("realign", {}), b)
    for f in READ_FIELDS:
        assert np.array_equal(got[f], at_default[f]), f


# ---- cluster_kernel on its own
CLUSTER_SWEEP = [{"bandwidth_short": 0.03}, {"bandwidth_long": 0.05}, {"bandwidth_length": 300}, {"bandwidth_length": 100000}, {"max_error": 0.03},
                 {"max_error": 0.005}, {"min_cov_fraction": 0.45}, MCF2, {"min_cov_fraction2_l": 1000, "min_cov_fraction2_f": 0.3},
                 {"max_error": 0.03, "bandwidth_long": 0.05, "min_cov_fraction": 0.45}]


def _cluster_cases_around(length_a, length_b):
    """helpers.cluster_cases(rng, 90) with the longest read of every case moved onto a threshold: case c has no read longer than
    L - 1, L, L + 1 (and one read of exactly that length) for L = length_a (c % 8 < 3), L = length_b (c % 8 in 3, 4, 5), or keeps its
    lengths (c % 8 >= 6).  The kernel tests `>= bandwidth_length` on every read and `< min_cov_fraction2_l` on a label's longest read."""
    rng = np.random.default_rng(36)
    cases = []
    for c, (d, lens) in enumerate(cluster_cases(rng, 90)):
        k = c % 8
        if k < 6:
            cap = (length_a, length_b)[k // 3] - 1 + k % 3
            lens = np.minimum(lens, cap).astype(np.uint32)
            lens[(c // 8) % len(lens)] = cap
        cases.append((d, lens))
    return cases


@pytest.mark.parametrize("kw", CLUSTER_SWEEP, ids=[_id(k) for k in CLUSTER_SWEEP])
def test_cluster_kernel_parameters(gpu, oracle, kw):
    """cluster_kernel through otg_cluster_batch, with read lengths one below, on and one above the two length thresholds in force.  Cases of
    the oracle's result (of 90) that differ from the defaults, in the order of CLUSTER_SWEEP: 20, 37, 14, 15, 40, 29, 15, 19, 7, 59."""
    P = abi.default_params(**kw)
    cases = _cluster_cases_around(int(P.bandwidth_length), int(P.min_cov_fraction2_l))
    at_value = cluster_compare(gpu, oracle, cases, **kw)
    _, el, eic, efc, eb = oracle.cluster_batch(abi.default_params(), *pack_cluster_cases(cases))
    _, len_off, nv = pack_cluster_cases(cases)[2:]
    moved = 0
    for c in range(len(cases)):
        s = slice(int(len_off[c]), int(len_off[c]) + int(nv[c]))
        same = (np.array_equal(at_value[0][s], el[s]) and at_value[1][c] == eic[c] and at_value[2][c] == efc[c]
                and np.array_equal(at_value[3][c], eb[c], equal_nan=True))
        moved += not same
    print("cluster_kernel, %s: %d of %d cases of the oracle's result differ from the defaults" % (_id(kw), moved, len(cases)))
    assert moved >= 1, kw


# ---- genotype_kernel
GENOTYPE_SWEEP = [{"gt_max_error": 0.0}, {"gt_max_error": 0.005}, {"gt_max_error": 0.1}, {"gt_max_error": 1.0}, {"gt_max_cosdis": 0.0},
                  {"gt_max_cosdis": 0.002}, {"gt_max_cosdis": 1.0}, {"gt_max_error": 0.1, "gt_max_cosdis": 0.002}, {"gt_max_error": 0.1, "gt_max_cosdis": 0.2}]
_genotype = {}


def _genotype_args():
    if "args" not in _genotype:
        _genotype["args"] = genotype_regions(np.random.default_rng(51), 120, 24, with_short=True)
    return _genotype["args"]


def _genotype_regions_moved(args, a, b):
    first, counts = args[3], args[4]
    moved = 0
    for r in range(len(counts)):
        s = slice(int(first[r]), int(first[r]) + int(counts[r]))
        same = all(np.array_equal(a[i][s], b[i][s], equal_nan=True) for i in (0, 1, 2, 3, 5)) and a[4][r] == b[4][r]
        moved += not same
    return moved


@pytest.mark.parametrize("kw", GENOTYPE_SWEEP, ids=[_id(k) for k in GENOTYPE_SWEEP])
def test_genotype_kernel_parameters(gpu, oracle, kw):
    """Seed 51, 120 regions: 105, 82, 24, 110, 105, 28, 69 regions of the oracle's result differ from the defaults for the seven single
    values, 24 for gt_max_error = 0.1 with gt_max_cosdis = 0.2 (gt_max_cosdis = 0.2 alone moves nothing and is not run alone)."""
    args = _genotype_args()
    at_value = genotype_check(gpu, oracle, args, **kw)
    moved = _genotype_regions_moved(args, at_value, oracle.genotype_cluster_batch(abi.default_params(), *args))
    print("genotype_kernel, %s: %d of %d regions of the oracle's result differ from the defaults" % (_id(kw), moved, len(args[4])))
    assert moved >= 1, kw


def test_genotype_kernel_parameters_edit_metric(gpu, oracle):
    """The same values under metric="edit" against genotype_edit_ref (which reads params.gt_max_error and takes gt_k from the oracle under
    the same params): the matrix does not depend on them and is computed once."""
    args = _genotype_args()
    mats, n_pairs = ger.edit_matrices(ger.region_seqs(*args))
    dist = np.concatenate(mats + [np.zeros(0)])
    at_default = ger.genotype_with_matrix(abi.default_params(), *args, mats)
    for kw in GENOTYPE_SWEEP:
        P = abi.default_params(**kw)
        exp = ger.genotype_with_matrix(P, *args, mats)
        moved = _genotype_regions_moved(args, exp, at_default)
        print("genotype_kernel (edit), %s: %d of %d regions of the reference's result differ from the defaults" % (_id(kw), moved, len(args[4])))
        assert moved >= 1, kw
        genotype_edit_compare(gpu.genotype_cluster_metric_batch(P, *args, metric="edit"), exp, dist, n_pairs)
    genotype_edit_compare(gpu.genotype_cluster_metric_batch(abi.default_params(), *args, metric="edit"), at_default, dist, n_pairs)

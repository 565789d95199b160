"""The genotype metric (OTG_GT_METRIC_EDIT) without a device: the reference helper of the GPU tests (genotype_edit_ref) against the oracle,
the motif-order pairs the length / 3-mer proxies cannot tell apart, and the C-ABI of the new entry points."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import otter_amd
from otter_amd import abi
from helpers import rand_seq, mutate, tr_seq
import genotype_edit_ref as ger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")
NEW_SYMBOLS = ("otg_genotype_cluster_metric_batch", "otg_genotype_metric_last_ms", "otg_genotype_cohort_metric")


def _pack(regions):
    seqs = [s for reg in regions for s in reg]
    arena, off, ln = abi.pack_seqs(seqs)
    counts = np.asarray([len(reg) for reg in regions], dtype=np.uint32)
    first = (np.cumsum(counts) - counts).astype(np.uint32)
    return arena, off, ln, first, counts


def test_helper_restates_the_oracle_given_the_length_matrix(oracle):
    """a few hundred small regions: with the length matrix the helper's cut, intersection and medoids are the oracle's anallele_cluster"""
    rng = np.random.default_rng(2024)
    regions = []
    for r in range(300):
        A = int(rng.integers(0, 10))
        base = [tr_seq(rng, int(rng.integers(8, 90))) if r % 3 else rand_seq(rng, int(rng.integers(8, 90))) for _ in range(int(rng.integers(1, 4)))]
        reg = []
        for a in range(A):
            s = mutate(rng, base[int(rng.integers(0, len(base)))], [0.0, 0.01, 0.05, 0.2][int(rng.integers(0, 4))])
            if a % 5 == 4:
                s = s[:int(rng.integers(1, max(2, len(s))))] or b"N"
            reg.append(s or b"N")
        regions.append(reg)
    args = _pack(regions)
    P = abi.default_params()
    e = oracle.genotype_cluster_batch(P, *args)
    h = ger.genotype_with_matrix(P, *args, ger.length_matrices(regions))
    for i, name in ((0, "gt"), (1, "gt_l"), (2, "gt_k"), (4, "n_gt"), (5, "reps")):
        assert np.array_equal(h[i], e[i]), name
    assert (e[4] > 1).sum() > 50          # the cases do split


def test_motif_order_pairs_one_genotype_by_length_two_by_edit(oracle):
    P = abi.default_params()
    for n in (20, 10, 40):
        a, b = ger.motif_order_pair(n)
        assert len(a) == len(b) == 6 * n
        args = _pack([[a, b]])
        assert oracle.genotype_cluster_batch(P, *args)[4][0] == 1            # the reference: one genotype
        mats, n_pairs = ger.edit_matrices([[a, b]])
        assert n_pairs == 1 and mats[0][0] == (2 * n) / float(6 * n)
        assert mats[0][0] == oracle.dp_edit(a, b) / float(6 * n)
        h = ger.genotype_with_matrix(P, *args, mats)
        assert h[4][0] == 2 and h[0].tolist() == [0, 1] and h[5].tolist() == [0, 1]


def test_edit_matrix_special_cases(oracle):
    seqs = [b"", b"ACGTACGT", b"", b"acgtacgt", b"ACGTACGT", b"N", b"A"]
    mats, n_pairs = ger.edit_matrices([seqs])
    d = mats[0]
    A = len(seqs)
    at = {(i, j): p for p, (i, j) in enumerate((i, j) for i in range(A) for j in range(i + 1, A))}
    assert d[at[(0, 2)]] == 0.0 and d[at[(1, 4)]] == 0.0             # equal byte strings
    assert d[at[(0, 1)]] == 1.0 and d[at[(0, 5)]] == 1.0             # empty against L bases: L / L
    assert d[at[(1, 3)]] == 1.0                                      # case-sensitive: every base differs
    assert d[at[(5, 6)]] == 1.0
    assert n_pairs == 5 * 4 // 2                                     # five distinct byte strings


def test_new_symbols_declared_exported_and_listed():
    text = open(HEADER).read()
    L = otter_amd.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in otter_amd.EXPORTS, name
        getattr(L, name)
    assert "#define OTG_GT_METRIC_LENGTH 0" in text and re.search(r"#define OTG_GT_METRIC_EDIT\s+1", text)
    assert abi.OTG_GT_METRIC_LENGTH == 0 and abi.OTG_GT_METRIC_EDIT == 1


def test_job_structs_keep_their_layout(tmp_path):
    """`reserved` became `metric` / `gt_metric`: same sizes and offsets as before (160 / 156 and 248 / 196), in the header and in abi.py"""
    assert C.sizeof(abi.GenotypeJob) == 160 and abi.GenotypeJob.metric.offset == 156 and abi.GenotypeJob.metric.size == 4
    assert C.sizeof(abi.CohortJob) == 248 and abi.CohortJob.gt_metric.offset == 196 and abi.CohortJob.gt_metric.size == 4
    assert C.sizeof(abi.otg_params) == 120
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "%s"\n'
                   'static_assert(sizeof(otg_genotype_job) == 160 && offsetof(otg_genotype_job, metric) == 156, "otg_genotype_job");\n'
                   'static_assert(sizeof(otg_cohort_job) == 248 && offsetof(otg_cohort_job, gt_metric) == 196, "otg_cohort_job");\n'
                   'static_assert(sizeof(otg_params) == 120, "otg_params");\n' % HEADER)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", str(src)])


def test_no_context_is_no_device():
    L = otter_amd.load()
    L.otg_last_error.restype = C.c_char_p
    P = abi.default_params()
    one = np.zeros(1, dtype=np.uint32)
    rc = L.otg_genotype_cluster_metric_batch(None, C.byref(P), None, C.c_uint64(0), None, None, None, abi.ptr(one), C.c_uint32(1),
                                             None, None, None, None, None, None, C.c_int32(abi.OTG_GT_METRIC_EDIT), None, None)
    assert rc == abi.OTG_ERR_NO_DEVICE
    assert b"otg_genotype_cluster_metric_batch" in L.otg_last_error(None)
    assert L.otg_genotype_cohort_metric(None, C.byref(P), C.c_int32(abi.OTG_GT_METRIC_EDIT)) == abi.OTG_ERR_NO_DEVICE


def test_bad_metric_is_an_argument_error_with_a_message(tmp_path):
    """the two file dispatchers refuse an unknown metric before they open anything"""
    bed = tmp_path / "r.bed"
    bed.write_text("chr1\t10\t20\n")
    for call, kw in ((lambda **k: otter_amd._lib.genotype_files("none.bam", str(bed), "none.fa", **k), "metric"),
                     (lambda **k: otter_amd._lib.cohort_files(["none.bam"], ["s"], str(bed), "none.fa", **k), "gt_metric")):
        try:
            call(**{kw: 7})
        except otter_amd.OtterGpuError as e:
            assert "(%d)" % abi.OTG_ERR_ARG in str(e) and "unknown genotype metric 7" in str(e), str(e)
        else:
            raise AssertionError("metric 7 was accepted")
    try:
        abi.gt_metric("hamming")
    except ValueError as e:
        assert "hamming" in str(e)
    else:
        raise AssertionError("metric 'hamming' was accepted")


def test_cli_refuses_an_unknown_metric():
    exe = os.path.join(ROOT, "tools", "otter_cohort")
    p = subprocess.run([exe, "-b", "x.bed", "-r", "x.fa", "--gt-metric", "foo", "s=x.bam"], capture_output=True)
    assert p.returncode == 1 and p.stdout == b"" and b"[ERROR] --gt-metric length | edit" in p.stderr

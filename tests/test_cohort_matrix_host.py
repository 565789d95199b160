"""CPU: the host side of the cohort k-mer matrix — the numpy restatement of the row list and of the samples' GT numbers pinned on the golden
joint VCF (no device code), the committed golden matrix re-derived by the restatement driver, and the C layout of the grown otg_cohort_job."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from otter_amd import abi
import cohort_helpers as H
import cohort_matrix_helpers as M
import vcf2mat_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_and_gt_restatement_on_the_golden_vcf(oracle, tmp_path):
    fx = H.golden_fixture(str(tmp_path))
    text, _, grp = H.oracle_cohort(oracle, fx)
    assert text == open(H.GOLDEN_VCF, "rb").read()
    S = len(fx["names"])
    P = abi.default_params()
    gt, _, _, _, ngt, reps = oracle.genotype_cluster_batch(P, grp["arena"], grp["seq_off"], grp["seq_len"], np.ascontiguousarray(grp["first_allele"][:-1]), grp["n_alleles"])
    rows = M.numpy_rows(grp["first_allele"], gt, ngt, reps, grp["sample"], S)
    seqs = M.row_seqs(rows, grp)
    lines = M.vcf_rows(text)
    regions_with_alleles = [r for r in range(len(grp["n_alleles"])) if grp["n_alleles"][r] > 0]
    assert len(lines) == len(regions_with_alleles) == 12 and rows["n_rows"] == 31
    for (_, alleles, gts), r in zip(lines, regions_with_alleles):
        r0, r1 = int(rows["row_first"][r]), int(rows["row_first"][r + 1])
        assert seqs[r0:r1] == alleles, r                                        # REF, then the ALT columns in order
        assert [tuple(p) for p in rows["sample_gt"][r].tolist()] == gts, r
    empty = [r for r in range(len(grp["n_alleles"])) if grp["n_alleles"][r] == 0]
    for r in empty:
        assert rows["row_first"][r] == rows["row_first"][r + 1] and (rows["sample_gt"][r] == -1).all()
    # the fixture exercises the restatement: samples without a call, a reference cluster that is not the first, multi-ALT lines
    assert any(g == (-1, -1) for _, _, gts in lines for g in gts)
    assert any(len(a) > 2 for _, a, _ in lines)
    ref_gt = [int(gt[int(grp["first_allele"][r + 1]) - 1]) for r in regions_with_alleles]
    assert min(ref_gt) == 0 and max(ref_gt) > 0


def test_golden_matrix_is_what_the_driver_prints(tmp_path):
    want = open(M.GOLDEN_MAT, "rb").read()
    assert want.count(b"\n") == 31 and all(len(l.split(b"\t")) == 5 + 4 ** M.GOLDEN_MAT_K + 1 for l in want.splitlines())
    ids = [l.split(b"\t")[2] for l in open(H.GOLDEN_VCF, "rb").read().split(b"\n") if l and not l.startswith(b"#")]
    assert sorted(set(l.split(b"\t")[0] for l in want.splitlines()), key=ids.index) == ids
    assert F.driver_text(F.build_driver(tmp_path), M.GOLDEN_MAT_K, H.GOLDEN_VCF) == want
    exe = F.build_driver(tmp_path, with_ref=True)           # the reference's own seq2kcounts / KUSAGE::hsdiv, where they are built
    if exe is not None:
        assert F.driver_text(exe, M.GOLDEN_MAT_K, H.GOLDEN_VCF) == want


def test_cohort_job_matrix_fields_match_c(tmp_path):
    fields = ["matrix_write", "matrix_user", "matrix_k"]
    assert [n for n, _ in abi.CohortJob._fields_][-4:-1] == fields
    src = tmp_path / "mj.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu", sizeof(otg_cohort_job));\n' +
                   "".join('printf(" %%zu", offsetof(otg_cohort_job, %s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "mj"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.CohortJob)] + [getattr(abi.CohortJob, f).offset for f in fields]
    assert C.sizeof(abi.WRITE_FN) == C.sizeof(C.c_void_p)


def test_numpy_rows_on_a_hand_made_case():
    # one region, S = 2: alleles [s0, s0, s1, ref]; clusters 0 = {a0}, 1 = {a1, ref}, 2 = {a2}; reps = first member of every cluster
    first = np.array([0, 0, 4], dtype=np.uint32)
    gt = np.array([0, 1, 2, 1], dtype=np.int32)
    reps = np.array([0, 1, 2, 0], dtype=np.int32)
    rows = M.numpy_rows(first, gt, np.array([0, 3], dtype=np.int32), reps, np.array([0, 0, 1, 2], dtype=np.int32), 2)
    # column order: REF (the reference allele itself, not its cluster's representative a1), then cluster 0, then cluster 2
    assert rows["row_first"].tolist() == [0, 0, 3] and rows["row_allele"].tolist() == [3, 0, 2]
    assert rows["sample_gt"].tolist() == [[[-1, -1], [-1, -1]], [[1, 0], [2, 2]]]


def test_entry_points_fail_loudly_without_a_context():
    import otter_amd
    lib = otter_amd.load()
    n = C.c_uint32(0)
    assert lib.otg_kmer_cohort_rows(None, C.byref(n), None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert lib.otg_kmer_cohort_usage(None, C.c_int32(3), C.c_uint32(0), C.c_uint32(0), None, None, None) == abi.OTG_ERR_NO_DEVICE
    assert lib.otg_kmer_cohort_device_rows(None, None, None, None, None) == abi.OTG_ERR_NO_DEVICE
    for m in ("cohort_kmer_rows", "cohort_kmer_usage"):
        assert callable(getattr(otter_amd.Context, m)), m

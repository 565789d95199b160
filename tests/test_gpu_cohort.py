"""GPU: the cohort path — sample BAMs to one joint VCF with the alleles staying on the device between `otter assemble` and `otter genotype`
(otg_cohort_begin / stage / regroup / genotype / collect, otg_cohort_files).

1. the device regroup against a numpy regroup of the per-sample assemble_collect outputs, byte for byte;
2. clustering on the staged data == otg_genotype_cluster_batch fed the numpy-regrouped arrays from host memory (hsd bit patterns included: same
   kernel, same inputs) and == the oracle under the tolerances of test_gpu_genotype.py (integers exact, hsd 1e-9 relative);
3. files: cohort_files returns the bytes of the round trip assemble_files per sample -> merged allele BAM -> genotype_files;
4. allele_write hands out the per-sample SAM text of assemble_files;
5. refusals;
6. the committed golden VCF (written without the product's device code, scripts/make_golden_cohort.py)."""
import os
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, synth, bamwrite
import cohort_helpers as H

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1 + 2: building blocks
def _sample_batch(seed, n_regions, empty, len_range=(150, 400), frac_het=0.8):
    b = synth.make_batch(n_regions, len_range=len_range, reads_range=(8, 14), err="hifi", seed=seed, frac_partial=0.1, frac_het=frac_het)
    for r in empty:
        b["regions"][r]["n_reads"] = 0
    return b


def _refs(rng, n_regions):
    return [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(40, 300))).tobytes()) for r in range(n_regions)]


def _stage_cohort(gpu, other, S, B, distinct=None):
    """S samples over the same B regions: region 0 empty in every sample, region 1 empty in all but sample 0, region 2 skipped for max_cov in
    the last sample, max_alleles = 4.  Runs alternate between two contexts (the cohort's own and a second one on the device).  With
    `distinct` only that many different runs are made and staged round-robin (many samples, cheap)."""
    P = abi.default_params(max_alleles=4)
    n_runs = distinct or S
    runs = []
    for k in range(n_runs):
        batch = _sample_batch(900 + k % 3, B, empty=[0] if k == 0 else [0, 1], frac_het=1.0 if distinct else 0.8)
        Pk = abi.default_params(max_alleles=4)
        if k == n_runs - 1:
            Pk.max_cov = int(batch["regions"][2]["n_reads"]) - 1
        runs.append((Pk, batch))
    gpu.cohort_begin(B, S)
    results = [None] * S
    collected = {}
    for k in (range(n_runs - 1, -1, -1) if S == 3 else range(n_runs)):          # staging order is free
        ctx = other if (k % 2) else gpu
        Pk, batch = runs[k]
        ctx.assemble_submit(Pk, batch)
        ctx.assemble_run()
        collected[k] = ctx.assemble_collect()
        for s in range(k, S, n_runs):
            gpu.cohort_stage(s, src=ctx)
            results[s] = collected[k]
    last = collected[n_runs - 1]
    assert last["regions"][2]["status"] == abi.OTG_REGION_SKIP_MAXCOV and last["regions"][2]["n_alleles"] == 0
    return P, results


def _check_blocks(gpu, oracle, S, B, distinct=None, want_wide=False):
    other = otter_amd.Context(0)
    try:
        P, results = _stage_cohort(gpu, other, S, B, distinct)
    finally:
        other.close()
    refs = _refs(np.random.default_rng(5 + S), B)
    exp = H.numpy_regroup(results, refs)
    ref_arena, ref_off, ref_len = abi.pack_seqs(refs)
    gpu.cohort_regroup(ref_arena, ref_off, ref_len)
    got = gpu.cohort_collect(clustered=False)
    H.same_regroup(got, exp)
    assert exp["n_alleles"][0] == 0                                          # empty everywhere: no reference allele either
    if S > 1 and not distinct:
        assert 2 <= exp["n_alleles"][1] <= 5 and set(exp["sample"][exp["first_allele"][1]:exp["first_allele"][2]]) == {0, S}
    assert (int(exp["n_alleles"].max()) > 256) == want_wide
    # 2: clustering on the staged data
    gpu.cohort_genotype(P)
    got = gpu.cohort_collect()
    H.same_regroup(got, exp)
    args = (exp["arena"], exp["seq_off"], exp["seq_len"], np.ascontiguousarray(exp["first_allele"][:-1]), exp["n_alleles"])
    up = gpu.genotype_cluster_batch(P, *args)
    ora = oracle.genotype_cluster_batch(P, *args)
    keys = ("gt", "gt_l", "gt_k", "hsd", "n_gt", "reps")
    for i, k in enumerate(keys):
        if k == "hsd":
            assert np.array_equal(got[k].view(np.uint64), up[i].view(np.uint64)), k
            assert np.allclose(got[k], ora[i], rtol=1e-9, atol=0, equal_nan=True)
        else:
            assert np.array_equal(got[k], up[i]), k
            assert np.array_equal(got[k], ora[i]), k
    gpu.cohort_end()
    return exp


@pytest.mark.parametrize("S", [1, 3, 8])
def test_regroup_and_clustering_against_numpy(gpu, oracle, S):
    exp = _check_blocks(gpu, oracle, S, 9)
    assert len(exp["alleles"]) > 4 * S


def test_regroup_wide_region(gpu, oracle):
    """200 samples (four distinct runs staged round-robin) x 2 alleles + the reference in one region: above 256 alleles, so
    genotype_kernel<WIDE> runs on the regrouped buffers"""
    exp = _check_blocks(gpu, oracle, 200, 5, distinct=4, want_wide=True)
    assert exp["n_alleles"].max() > 256


def test_building_block_refusals(gpu):
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError):
        gpu.cohort_stage(0)                                                   # no batch open
    gpu.cohort_begin(4, 2)
    batch = _sample_batch(900, 4, empty=[])
    gpu.assemble_submit(abi.default_params(), batch)
    gpu.assemble_run()
    gpu.cohort_stage(0)
    with pytest.raises(otter_amd.OtterGpuError, match="staged already"):
        gpu.cohort_stage(0)
    with pytest.raises(otter_amd.OtterGpuError, match="sample 2 of 2"):
        gpu.cohort_stage(2)
    ref_arena, ref_off, ref_len = abi.pack_seqs([b"ACGT"] * 4)
    with pytest.raises(otter_amd.OtterGpuError, match="sample 1 has not been staged"):
        gpu.cohort_regroup(ref_arena, ref_off, ref_len)
    gpu.assemble_submit(abi.default_params(), _sample_batch(901, 5, empty=[]))
    gpu.assemble_run()
    with pytest.raises(otter_amd.OtterGpuError, match="5 regions"):
        gpu.cohort_stage(1)
    gpu.cohort_end()


# ---------------------------------------------------------------------------------------------- 3 + 4: files
def _n_records(sam):
    return sam.count(b"\n") - sam.count(b"\n@") - int(sam.startswith(b"@"))


def _round_trip(fx, tmp, tag, P, ol, orr, with_ref_tool=False):
    """the existing entry points alone: assemble_files per sample, the SAM texts merged, written as BAM, genotype_files"""
    sams = [otter_amd.assemble_files(b, fx["bed"], fasta=fx["fasta"], read_group=n, params=P, offset_l=ol, offset_r=orr, threads=3)[0]
            for b, n in zip(fx["bams"], fx["names"])]
    merged = H.merge_sams(sams)
    bam = os.path.join(tmp, "merged_%s.bam" % tag)
    assert H.sam_to_bam_python(merged, bam) == sum(_n_records(t) for t in sams)
    out = {"sams": sams, "vcf": otter_amd.genotype_files(bam, fx["bed"], fasta=fx["fasta"], params=P, threads=3)[0]}
    if with_ref_tool:
        import oracle_lib
        if oracle_lib.ref_io() is not None:
            sam_path, bam2 = os.path.join(tmp, "merged_%s.sam" % tag), os.path.join(tmp, "merged_ref_%s.bam" % tag)
            open(sam_path, "wb").write(merged)
            assert oracle_lib.ref_io().ref_sam_to_bam(sam_path.encode(), bam2.encode()) > 0
            out["vcf_ref_tool"] = otter_amd.genotype_files(bam2, fx["bed"], fasta=fx["fasta"], params=P, threads=3)[0]
    return out


@pytest.fixture(scope="module")
def cohort(tmp_path_factory, gpu):
    tmp = str(tmp_path_factory.mktemp("cohort"))
    fx = bamwrite.make_cohort_fixture(tmp, 44, 5, depth=10, len_range=(200, 600), seed=29)
    fx["tmp"] = tmp
    fx["default"] = _round_trip(fx, tmp, "default", abi.default_params(), 1, 0, with_ref_tool=True)
    return fx


def test_files_one_pass_equals_round_trip(cohort):
    exp = cohort["default"]["vcf"]
    lines = [l for l in exp.split(b"\n") if l and not l.startswith(b"#")]
    assert len(lines) >= 40 and exp.count(b"\t./.:") > 0                      # nearly every region has a line; some samples miss some regions
    assert sum(1 for l in lines if l.split(b"\t")[4] != b".") > 20            # the loci are polymorphic
    if "vcf_ref_tool" in cohort["default"]:
        assert cohort["default"]["vcf_ref_tool"] == exp
    for batch in (0, 7):
        for devices in ([0], [0, 0]):
            text, st = otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], batch_regions=batch, devices=devices, threads=3)
            assert text == exp, (batch, devices)
            assert st["n_regions"] == 44 and st["n_regions_ok"] == len(lines) and st["n_devices"] == len(devices)
            assert st["n_alleles"] == sum(_n_records(t) for t in cohort["default"]["sams"])
            assert st["n_reads"] > 0 and st["ms_total"] > 0


@pytest.mark.parametrize("variant", ["wfadaptive", "haps", "offsets"])
def test_files_variants_equal_round_trip(cohort, variant):
    P, ol, orr = abi.default_params(), 1, 0
    if variant == "wfadaptive":
        P = abi.default_params(heuristic=abi.OTG_HEURISTIC_WFADAPTIVE, heur_min_wavefront_length=10, heur_max_distance_threshold=50, heur_steps_between_cutoffs=1)
    elif variant == "haps":
        P = abi.default_params(ignore_haps=0)
    else:
        ol, orr = 3, 2
    exp = _round_trip(cohort, cohort["tmp"], variant, P, ol, orr)["vcf"]
    text, _ = otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], params=P, offset_l=ol, offset_r=orr, threads=3)
    assert text == exp
    assert len(exp) > 10000


def test_allele_write_is_the_sample_sam_text(cohort):
    text, st, sams = otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], batch_regions=7, devices=[0, 0], threads=3, alleles=True)
    assert text == cohort["default"]["vcf"]
    assert len(sams) == len(cohort["bams"])
    for s, exp in enumerate(cohort["default"]["sams"]):
        assert sams[s] == exp, cohort["names"][s]


# ---------------------------------------------------------------------------------------------- 5: refusals
def _refused(match, *a, **kw):
    with pytest.raises(otter_amd.OtterGpuError) as e:
        otter_amd.cohort_files(*a, **kw)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and match in str(e.value), str(e.value)


def test_files_refusals(cohort, tmp_path):
    bams, names, bed, fa = cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"]
    _refused("'s01' is given twice", bams, ["s00", "s01", "s01", "s03", "s04"], bed, fa)
    _refused("empty name", bams, ["s00", "", "s02", "s03", "s04"], bed, fa)
    _refused(bams[1], bams, ["s00", "", "s02", "s03", "s04"], bed, fa)
    _refused("zero samples", [], [], bed, fa)
    _refused("no reference FASTA", bams, names, bed, None)
    dup = str(tmp_path / "dup.bed")
    lines = open(bed).read().splitlines()
    open(dup, "w").write("\n".join(lines[:5] + [lines[2]] + lines[5:]) + "\n")
    c, s, e = lines[2].split("\t")
    _refused("BED records 3 and 6", bams, names, dup, fa)
    _refused("%s:%s-%s" % (c, s, e), bams, names, dup, fa)
    other = bamwrite.make_tr_fixture(str(tmp_path), 2, depth=4, len_range=(200, 300))        # targets: chrS, not chrC
    _refused(other["bam"], bams[:2] + [other["bam"]], names[:3], bed, fa)


# ---------------------------------------------------------------------------------------------- 6: the independent expectation
def test_files_against_the_committed_golden(gpu, tmp_path):
    fx = H.golden_fixture(str(tmp_path))
    text, st = otter_amd.cohort_files(fx["bams"], fx["names"], fx["bed"], fx["fasta"], threads=2)
    assert text == open(H.GOLDEN_VCF, "rb").read()
    text7, _ = otter_amd.cohort_files(fx["bams"], fx["names"], fx["bed"], fx["fasta"], batch_regions=5, devices=[0, 0])
    assert text7 == text

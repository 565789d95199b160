"""GPU: the k-mer usage matrix of the joint alleles with the rows staying in HBM (otg_kmer_cohort_rows / otg_kmer_cohort_usage, the matrix
writer of otg_cohort_files, tools/otter_cohort --matrix).

1. building blocks: the device row list and GT numbers == the numpy restatement on cohort_collect(); usage / gc / hsd bit for bit what
   kmer_usage_batch gives for the same sequences uploaded from the host (the same kernels on the same bytes), exact against the numpy k-mer
   restatement (hsd 1e-9 relative, as tests/test_gpu_vcf2mat.py);
2. ranges, device tensors, refusals;
3. files: the matrix text == vcf2mat_files on the VCF of the same call == the restatement driver; the VCF bytes unchanged;
4. the committed golden matrix (written without the product's device code, scripts/make_golden_cohort_matrix.py) and the CLI."""
import os
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, bamwrite
import cohort_helpers as H
import cohort_matrix_helpers as M
import vcf2mat_fixtures as F

pytestmark = pytest.mark.gpu
CLI = os.path.join(F.ROOT, "tools", "otter_cohort")


@pytest.fixture(scope="module")
def other():
    ctx = otter_amd.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return F.build_driver(tmp_path_factory.mktemp("matrix_driver"))


# ---------------------------------------------------------------------------------------------- 1: building blocks
_VALUES = {}


def _kmer_values(seq, k):
    """numpy restatement of one row, computed once per (sequence, k)"""
    key = (seq, k)
    if key not in _VALUES:
        _VALUES[key] = F.kmer_values(seq, k)
    return _VALUES[key]


@pytest.mark.parametrize("S", [1, 3])
def test_rows_and_usage_against_numpy(gpu, other, S):
    M.stage(gpu, other, S)
    got = gpu.cohort_collect()
    exp = M.numpy_rows(got["first_allele"], got["gt"], got["n_gt"], got["reps"], got["sample"], S)
    rows = gpu.cohort_kmer_rows()
    assert rows["n_rows"] == exp["n_rows"] > 8
    for key in ("row_first", "row_allele", "sample_gt"):
        assert rows[key].dtype == exp[key].dtype and np.array_equal(rows[key], exp[key]), key
    assert rows["sample_gt"].shape == (M.N_REGIONS, S, 2)
    # the cases the reference alleles were chosen for (cohort_matrix_helpers.choose_refs) occurred
    regions = [r for r in range(M.N_REGIONS) if got["n_alleles"][r] > 0]
    assert regions == list(range(1, M.N_REGIONS)) and (rows["sample_gt"][0] == -1).all()
    ref_gt = {r: int(got["gt"][int(got["first_allele"][r + 1]) - 1]) for r in regions}
    n_gt = {r: int(got["n_gt"][r]) for r in regions}
    assert any(ref_gt[r] == 0 and n_gt[r] > 1 for r in regions)                                   # reference first
    assert any(ref_gt[r] == n_gt[r] - 1 and n_gt[r] > 1 for r in regions)                         # reference last
    assert n_gt[1] == 1 and rows["row_first"][2] - rows["row_first"][1] == 1                      # a single row: ALT '.'
    if S == 3:
        assert any(0 < ref_gt[r] < n_gt[r] - 1 for r in regions)                                  # reference in the middle
        assert (rows["sample_gt"][1, 1:] == -1).all() and (rows["sample_gt"][1, 0] >= 0).all()   # ./. next to a call
    seqs = M.row_seqs(rows, got)
    assert max(len(s) for s in seqs) == M.LONG_REF                                                # one row of two tier-L workgroups
    arena, off, ln = abi.pack_seqs(seqs)
    for k in (1, 3, 4, 5, 7, 8):
        usage, gc, hsd = gpu.cohort_kmer_usage(k)
        assert usage.shape == (rows["n_rows"], 4 ** k + 1)
        hu, hg, hh = gpu.kmer_usage_batch(arena, off, ln, k=k)
        assert np.array_equal(usage.view(np.uint64), hu.view(np.uint64)), k
        assert np.array_equal(gc.view(np.uint64), hg.view(np.uint64)) and np.array_equal(hsd.view(np.uint64), hh.view(np.uint64)), k
        for a, s in enumerate(seqs):
            counts, u, g, h = _kmer_values(s, k)
            total = max(len(s) - k + 1, 0)
            assert np.array_equal(usage[a], u, equal_nan=True), (k, a)
            if total:
                assert np.array_equal(np.rint(usage[a] * total).astype(np.int64), counts), (k, a)
            assert np.array_equal(gc[a], g, equal_nan=True), (k, a)
            assert abs(hsd[a] - h) <= 1e-9 * h, (k, a, hsd[a], h)
    gpu.cohort_end()


# ---------------------------------------------------------------------------------------------- 2: ranges, device tensors, refusals
@pytest.fixture
def staged(gpu, other):
    M.stage(gpu, other, 3)
    yield gpu
    gpu.cohort_end()


def test_ranges(staged):
    gpu = staged
    n = gpu.cohort_kmer_rows()["n_rows"]
    whole = gpu.cohort_kmer_usage(3, 0, n)
    head = gpu.cohort_kmer_usage(3, 0, 5)
    rest = gpu.cohort_kmer_usage(3, 5)
    assert rest[0].shape == (n - 5, 65)
    for w, h, r in zip(whole, head, rest):
        assert np.array_equal(np.concatenate([h, r]).view(np.uint64), w.view(np.uint64))
    for w, d in zip(whole, gpu.cohort_kmer_usage(3)):
        assert np.array_equal(w.view(np.uint64), d.view(np.uint64))
    for begin in (0, 7, n):
        u, g, h = gpu.cohort_kmer_usage(3, begin, 0)                                              # an empty range is fine
        assert u.shape == (0, 65) and g.shape == (0,) and h.shape == (0,)
    # tier L in ranges: the prefix of the workgroups is scanned on the device for whichever rows the range holds
    whole8 = gpu.cohort_kmer_usage(8)
    lo = int(gpu.cohort_kmer_rows()["row_first"][5])                                              # the 70 000-base row opens this range
    part8 = gpu.cohort_kmer_usage(8, lo, 3)
    for w, p in zip(whole8, part8):
        assert np.array_equal(w[lo:lo + 3].view(np.uint64), p.view(np.uint64))


def test_device_tensors(staged):
    import torch
    gpu = staged
    dev = torch.device("cuda", gpu.device)
    rows = gpu.cohort_kmer_rows()
    drows = gpu.cohort_kmer_rows(device_tensor=True)
    n = rows["n_rows"]
    assert drows["n_rows"] == n
    assert drows["row_first"].shape == (M.N_REGIONS + 1,) and drows["row_allele"].shape == (n,) and drows["sample_gt"].shape == (M.N_REGIONS, 3, 2)
    for key in ("row_first", "row_allele", "sample_gt"):
        assert drows[key].dtype == torch.int32 and drows[key].device == dev, key
        assert np.array_equal(drows[key].cpu().numpy().astype(np.int64), rows[key].astype(np.int64)), key
    hu, hg, hh = gpu.cohort_kmer_usage(5, 2, 9)
    du, dg, dh = gpu.cohort_kmer_usage(5, 2, 9, device_tensor=True)
    assert du.shape == (9, 4 ** 5 + 1) and dg.shape == (9,) and dh.shape == (9,)
    for t in (du, dg, dh):
        assert t.dtype == torch.float64 and t.device == dev
    # valid until the next k-mer call: the row list is read in between, and the genotype calls index the matrix on the device
    again = gpu.cohort_kmer_rows(device_tensor=True)
    assert np.array_equal(du.cpu().numpy().view(np.uint64), hu.view(np.uint64))
    assert np.array_equal(dg.cpu().numpy(), hg, equal_nan=True) and np.array_equal(dh.cpu().numpy(), hh)
    full = gpu.cohort_kmer_usage(3, device_tensor=True)[0]
    r = 3
    first = again["row_first"][r].item()
    picked = full[first + again["sample_gt"][r].clamp(min=0).long()]                              # [S, 2, bins]: the usage of every called allele
    assert picked.shape == (3, 2, 65) and picked.device == dev
    c_ms, e_ms = gpu.kmer_usage_last_ms()
    assert c_ms > 0 and e_ms >= 0


def test_building_block_refusals(gpu, other):
    import torch
    gpu.cohort_end()
    with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
        gpu.cohort_kmer_rows()
    P = abi.default_params(max_alleles=4)
    batches = M.sample_batches(3)
    gpu.cohort_begin(M.N_REGIONS, 3)
    results = []
    for k, batch in enumerate(batches):
        gpu.assemble_submit(P, batch)
        gpu.assemble_run()
        results.append(gpu.assemble_collect())
        gpu.cohort_stage(k)
    ref_arena, ref_off, ref_len = abi.pack_seqs(M.choose_refs(results))
    gpu.cohort_regroup(ref_arena, ref_off, ref_len)
    for call in (gpu.cohort_kmer_rows, lambda: gpu.cohort_kmer_usage(3, 0, 1), lambda: gpu.cohort_kmer_rows(device_tensor=True)):
        with pytest.raises(otter_amd.OtterGpuError, match="has not been clustered") as e:
            call()
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
    gpu.cohort_genotype(P)
    n = gpu.cohort_kmer_rows()["n_rows"]
    assert n >= 22

    def refused(code, *a):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            gpu.cohort_kmer_usage(*a)
        assert "(%d)" % code in str(e.value), str(e.value)
    refused(abi.OTG_ERR_ARG, 0, 0, 1)
    refused(abi.OTG_ERR_ARG, 13, 0, 1)
    refused(abi.OTG_ERR_ARG, 3, n, 1)
    refused(abi.OTG_ERR_ARG, 3, 0, n + 1)
    refused(abi.OTG_ERR_ARG, 3, 2 ** 32 - 1, 2)
    gpu.cohort_kmer_usage(3, 0, 1)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(gpu.device)[0]
    refused(abi.OTG_ERR_CAPACITY, 12, 0, 22)                                                      # 22 rows of 4^12+1 doubles and u32 counts: above 4 GiB
    assert free0 - torch.cuda.mem_get_info(gpu.device)[0] < (1 << 30)                             # refused before the workspace was allocated
    gpu.cohort_end()
    for call in (gpu.cohort_kmer_rows, lambda: gpu.cohort_kmer_usage(3, 0, 1)):
        with pytest.raises(otter_amd.OtterGpuError, match="no cohort batch is open"):
            call()


# ---------------------------------------------------------------------------------------------- 3: files
@pytest.fixture(scope="module")
def cohort(tmp_path_factory, gpu):
    tmp = str(tmp_path_factory.mktemp("cohort_matrix"))
    fx = bamwrite.make_cohort_fixture(tmp, 44, 5, depth=10, len_range=(200, 600), seed=29)
    fx["tmp"] = tmp
    return fx


def test_files_matrix_equals_vcf2mat_of_the_same_vcf(cohort, driver):
    args = (cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"])
    plain, st0 = otter_amd.cohort_files(*args, threads=3)
    vcf = os.path.join(cohort["tmp"], "joint.vcf")
    open(vcf, "wb").write(plain)
    want = otter_amd.vcf2mat_files(vcf, cohort["bed"], k=3, threads=2)[0]
    assert want.count(b"\n") > 100
    assert F.driver_text(driver, 3, vcf) == want
    for batch in (0, 7):
        for devices in ([0], [0, 0]):
            text, st, mat = otter_amd.cohort_files(*args, batch_regions=batch, devices=devices, threads=3, matrix_k=3)
            assert text == plain, (batch, devices)
            assert mat == want, (batch, devices)
            assert st["output_bytes"] == st0["output_bytes"] == len(plain) and st["n_regions_ok"] == st0["n_regions_ok"]


def test_files_refuse_a_bad_k(cohort):
    for k in (0, 13):
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], matrix_k=k)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "invalid '--kmer-size' (%d). Needs to be 1 <= x <= 12." % k in str(e.value)
        with pytest.raises(otter_amd.OtterGpuError) as e2:
            otter_amd.vcf2mat_files(H.GOLDEN_VCF, cohort["bed"], k=k)
        assert str(e.value).split(": ", 1)[1] == str(e2.value).split(": ", 1)[1]                 # vcf2mat's message


def test_files_with_whole_locus_deletions(gpu, tmp_path, driver):
    """a zero-length allele is <DEL> in the VCF: alone in its ALT column vcf2mat reads it back as N, beside other ALT alleles as the five
    characters; the matrix of the same call says the same in both cases (k = 6: the text <DEL> has no window at all)"""
    fx = M.make_deletion_fixture(str(tmp_path))
    args = (fx["bams"], fx["names"], fx["bed"], fx["fasta"])
    plain, _ = otter_amd.cohort_files(*args, threads=2)
    alts = [l.split(b"\t")[4] for l in plain.split(b"\n") if l and not l.startswith(b"#")]
    assert len(alts) == 4 and alts[0] == b"<DEL>" and alts[1].startswith(b"<DEL>,") and len(alts[1].split(b",")) == 3 and b"<DEL>" not in alts[2]
    vcf = str(tmp_path / "joint.vcf")
    open(vcf, "wb").write(plain)
    for k, batch in ((3, 0), (3, 1), (6, 0)):
        text, _, mat = otter_amd.cohort_files(*args, threads=2, batch_regions=batch, matrix_k=k)
        want = otter_amd.vcf2mat_files(vcf, fx["bed"], k=k)[0]
        assert text == plain and mat == want, (k, batch)
        assert want == F.driver_text(driver, k, vcf), k
        rows = [l.split(b"\t") for l in want.splitlines()]
        assert rows[1][:5] == [b"chrC:%d-%d" % fx["regions"][0][1:], b"1", b"0", b"1", b"1"]                   # the lone <DEL>: N
        assert rows[3][:5] == [b"chrC:%d-%d" % fx["regions"][1][1:], b"1", b"0", b"5", b"1"]                   # beside other ALTs: the text
        assert rows[3][-1] == (b"1" if k <= 5 else b"-nan")


def test_matrix_writer_refusal(cohort, monkeypatch):
    from otter_amd import _lib
    run = _lib._run_files_job

    def refusing(fn_name, job, job_type, callbacks=None, sink=None):
        cbs = dict(callbacks or {})
        cbs["matrix_write"] = (cbs["matrix_write"][0], lambda _user, _data, _n: 1)
        return run(fn_name, job, job_type, cbs, sink)
    monkeypatch.setattr(_lib, "_run_files_job", refusing)
    with pytest.raises(otter_amd.OtterGpuError) as e:
        otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], batch_regions=7, matrix_k=3)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and "the matrix writer failed" in str(e.value)


# ---------------------------------------------------------------------------------------------- 4: the independent expectation
def test_golden_matrix_and_cli(gpu, tmp_path, driver):
    fx = H.golden_fixture(str(tmp_path))
    args = (fx["bams"], fx["names"], fx["bed"], fx["fasta"])
    text, _, mat = otter_amd.cohort_files(*args, threads=2, matrix_k=M.GOLDEN_MAT_K)
    assert text == open(H.GOLDEN_VCF, "rb").read()
    assert mat == open(M.GOLDEN_MAT, "rb").read()
    # tiers M and L end to end; with alleles=True the matrix is still the last element
    text5, _, sams, mat5 = otter_amd.cohort_files(*args, batch_regions=5, devices=[0, 0], alleles=True, matrix_k=5)
    assert text5 == text and len(sams) == len(fx["bams"]) and mat5 == F.driver_text(driver, 5, H.GOLDEN_VCF)
    assert otter_amd.cohort_files(*args, batch_regions=5, matrix_k=8)[2] == F.driver_text(driver, 8, H.GOLDEN_VCF)
    out = str(tmp_path / "cli.mat")
    r = subprocess.run([CLI, "-b", fx["bed"], "-r", fx["fasta"], "-t", "2", "--matrix", out, "-k", "5"] + ["%s=%s" % (n, b) for n, b in zip(fx["names"], fx["bams"])],
                       capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == text, r.stderr
    assert open(out, "rb").read() == mat5

"""`otter vcf2mat` on the device: otg_kmer_usage_batch against the numpy restatement across the three counting tiers and their edges,
otg_vcf2mat_files and tools/otter_vcf2mat against the golden rows, batching and threads, the chain from otg_genotype_files, and the
zero-copy device tensors."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import otter_amd
from otter_amd import abi
import vcf2mat_fixtures as F

GOLD_VCF = os.path.join(F.GOLDEN, "vcf2mat_small.vcf.gz")
CLI = os.path.join(F.ROOT, "tools", "otter_vcf2mat")


def _golden(k):
    return gzip.open(os.path.join(F.GOLDEN, "vcf2mat_small_k%d.txt.gz" % k)).read()


def _seq(rng, n):
    """ACGT in both cases with about 1 % of other bytes (N, IUPAC codes, a byte >= 0x80, NUL)"""
    alpha = np.frombuffer(b"ACGTACGTACGTACGTacgt", dtype=np.uint8)
    s = alpha[rng.integers(0, len(alpha), n)]
    if n:
        bad = rng.random(n) < 0.01
        s[bad] = np.frombuffer(b"NRY\x80\xff\x00n-", dtype=np.uint8)[rng.integers(0, 8, int(bad.sum()))]
    return s.tobytes()


def _check(gpu, seqs, k):
    arena, off, ln = abi.pack_seqs(seqs)
    usage, gc, hsd = gpu.kmer_usage_batch(arena, off, ln, k=k)
    assert usage.shape == (len(seqs), 4 ** k + 1)
    for a, s in enumerate(seqs):
        _, u, g, h = F.kmer_values(s, k)
        assert np.array_equal(usage[a], u, equal_nan=True), (k, len(s))
        assert np.array_equal(gc[a], g, equal_nan=True), (k, len(s))
        assert abs(hsd[a] - h) <= 1e-9 * h, (k, len(s), hsd[a], h)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 4, 5, 7, 8, 12])
def test_kmer_usage_tiers(gpu, k):
    rng = np.random.default_rng(30 + k)
    lens = [0, k - 1, k, 63, 64, 65, 20_000, 100_000] if k < 12 else [0, k - 1, k, 64, 100_000]
    if k in (1, 4):
        lens.append(4_300_000)                 # past 4095 tiles: the wave tier folds its 16-bit columns mid-sequence
    seqs = [_seq(rng, n) for n in lens]
    seqs.append(b"A" * 70_000)                 # one bin holds every window
    _check(gpu, seqs, k)


@pytest.mark.gpu
def test_kmer_usage_many_alleles_and_workspace(gpu):
    rng = np.random.default_rng(77)
    seqs = [_seq(rng, int(n)) for n in rng.integers(0, 3000, 700)]
    for k in (3, 6, 9):
        _check(gpu, seqs, k)
    arena, off, ln = abi.pack_seqs([b"ACGT"] * 22)
    with pytest.raises(otter_amd.OtterGpuError) as e:            # 22 rows of 4^12+1 doubles and u32 counts exceed the 4 GiB workspace
        gpu.kmer_usage_batch(arena, off, ln, k=12)
    assert "(%d)" % abi.OTG_ERR_CAPACITY in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError):
        gpu.kmer_usage_batch(arena, off, ln, k=13)


@pytest.mark.gpu
def test_device_tensor(gpu):
    import torch
    rng = np.random.default_rng(3)
    seqs = [_seq(rng, n) for n in (0, 2, 500, 9000)]
    arena, off, ln = abi.pack_seqs(seqs)
    hu, hg, hh = gpu.kmer_usage_batch(arena, off, ln, k=5)
    du, dg, dh = gpu.kmer_usage_batch(arena, off, ln, k=5, device_tensor=True)
    assert du.shape == (4, 4 ** 5 + 1) and dg.shape == (4,) and dh.shape == (4,)
    assert du.dtype == torch.float64 and du.device == torch.device("cuda", gpu.device)
    assert np.array_equal(du.cpu().numpy(), hu, equal_nan=True)
    assert np.array_equal(dg.cpu().numpy(), hg, equal_nan=True) and np.array_equal(dh.cpu().numpy(), hh)
    c_ms, e_ms = gpu.kmer_usage_last_ms()
    assert c_ms > 0 and e_ms >= 0


@pytest.fixture(scope="module")
def bed(tmp_path_factory):
    p = tmp_path_factory.mktemp("vcf2mat") / "t.bed"
    p.write_text("chr1\t100\t200\n")
    return str(p)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 6])
def test_files_and_cli_on_the_golden_vcf(gpu, bed, k):
    want = _golden(k)
    text, st = otter_amd.vcf2mat_files(GOLD_VCF, bed, k=k)
    assert text == want
    assert st["n_regions"] == 19 and st["n_alleles"] == want.count(b"\n") and st["output_bytes"] == len(want)
    for batch, threads in ((1, 1), (3, 4), (5, 2)):
        assert otter_amd.vcf2mat_files(GOLD_VCF, bed, k=k, threads=threads, batch_alleles=batch)[0] == want
    r = subprocess.run([CLI, "-b", bed, "-k", str(k), "-t", "3", GOLD_VCF], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr


@pytest.mark.gpu
def test_genotype_vcf_chain(gpu, tmp_path):
    """the VCF otg_genotype_files writes, turned into rows: the same bytes as the restatement's"""
    g = json.load(open(os.path.join(F.GOLDEN, "genotype_ref.json")))
    bedp = tmp_path / "g.bed"
    bedp.write_text("".join("%s\t%d\t%d\n" % tuple(r) for r in g["regions"]))
    vcf_text, _ = otter_amd.genotype_files(os.path.join(F.GOLDEN, "genotype_small.bam"), str(bedp),
                                           fasta=os.path.join(F.GOLDEN, "genotype_small.fa"), threads=2)
    vcf = tmp_path / "g.vcf"
    vcf.write_bytes(vcf_text)
    exe = F.build_driver(tmp_path)
    for k in (3, 4):
        want = F.driver_text(exe, k, str(vcf))
        assert want.count(b"\n") > 20
        assert otter_amd.vcf2mat_files(str(vcf), str(bedp), k=k, threads=2)[0] == want

"""GPU parity at the size thresholds of the clustering stage: deep loci for `assemble` (the LDS working copy up to 64 valid reads, the
on-chip scratch up to 256, the HBM slab of the wide kernel above that; max_cov edges; max_alleles 3 and 4) and large cohorts for
`genotype` (the LDS matrix up to 102 alleles, HBM matrices above, the wide kernel above 256; a 4.3 Mb homopolymer allele whose 3-mer
counts pass the 16-bit per-lane columns).  Same contracts as test_gpu_pipeline.py / test_gpu_genotype.py: integer fields and sequences
bit-exact, `se` within 1e-6, gt / gt_l / gt_k / reps bit-exact, hsd within 1e-9 relative.  The oracle runs in threads (one batch each)."""
import os
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
from otter_amd import abi
import oracle_lib
from helpers import deep_batch, tie_heavy_matrix, pack_cluster_cases, genotype_region_alleles, rand_seq
from test_gpu_pipeline import compare

pytestmark = pytest.mark.gpu

STATS = ("edit_tasks", "edit_cells", "edit_seq_bytes", "affine_tasks", "affine_cells", "affine_seq_bytes", "allele_bytes", "algorithmic_bytes")


def _oracle_threads(fn, jobs):
    with ThreadPoolExecutor(min(16, max(1, len(jobs)))) as ex:
        return list(ex.map(lambda j: fn(*j), jobs))


def _assemble_parity(gpu, oracle, jobs):
    """jobs: list of (params, batch).  Oracle in threads, then every batch on the GPU against it (stats included)."""
    oras = _oracle_threads(oracle.assemble_batch, jobs)
    out = []
    for (P, b), ora in zip(jobs, oras):
        res = gpu.assemble(P, b)
        compare(res, ora, b)
        st = gpu.assemble_stats()
        for f in STATS:
            assert int(st[f]) == int(ora["stats"][0][f]), f
        out.append(res)
    return out


def _hifi(rng, n_span, n_part=3, lens=None):
    L = int(rng.integers(200, 500))
    return (n_span, n_part, lens or (L, int(L * rng.uniform(1.1, 1.3))))


def test_assemble_valid_read_thresholds(gpu, oracle):
    """Valid-read counts on both sides of 64 (LDS working copy) and 128, up to the reference default max_cov; each region also has three
    one-sided reads for the reassignment stage.  max_cov 256 leaves room for them next to 200 valid reads."""
    rng = np.random.default_rng(601)
    counts = (63, 64, 65, 127, 128, 129, 199, 200)
    jobs = [(abi.default_params(max_cov=256), deep_batch(rng, [_hifi(rng, n)])) for n in counts]
    jobs.append((abi.default_params(max_cov=256), deep_batch(rng, [_hifi(rng, n) for n in counts])))    # all in one batch too
    res = _assemble_parity(gpu, oracle, jobs)
    assert list(res[-1]["regions"]["n_valid"]) == list(counts)
    assert (res[-1]["regions"]["status"] == abi.OTG_REGION_OK).all()
    assert all((r["regions"]["ic"] >= 2).all() for r in res)      # bimodal: the NN-chain and the tree cut ran on every region


def test_assemble_max_cov_edges(gpu, oracle):
    """200 reads are processed and 201 skipped under the defaults; 256 / 257 under max_cov 256."""
    rng = np.random.default_rng(602)
    b1 = deep_batch(rng, [_hifi(rng, 200, 0), _hifi(rng, 201, 0), _hifi(rng, 150, 51)])
    b2 = deep_batch(rng, [_hifi(rng, 256, 0), _hifi(rng, 257, 0), _hifi(rng, 250, 6)])
    r1, r2 = _assemble_parity(gpu, oracle, [(abi.default_params(), b1), (abi.default_params(max_cov=256), b2)])
    S = abi.OTG_REGION_SKIP_MAXCOV
    assert list(r1["regions"]["status"]) == [abi.OTG_REGION_OK, S, S]
    assert list(r2["regions"]["status"]) == [abi.OTG_REGION_OK, S, abi.OTG_REGION_OK]
    assert int(r2["regions"]["n_valid"][0]) == 256


def test_assemble_above_256_valid_reads(gpu, oracle):
    """The wide clustering kernel: 257 (+3 one-sided), 400 and 1000 valid reads under max_cov 1000, next to a narrow region in one batch."""
    rng = np.random.default_rng(603)
    P = abi.default_params(max_cov=1000)
    jobs = [(P, deep_batch(rng, [_hifi(rng, 257), _hifi(rng, 40)])),
            (P, deep_batch(rng, [_hifi(rng, 400, 5)])),
            (P, deep_batch(rng, [(1000, 0, (200, 236))]))]
    res = _assemble_parity(gpu, oracle, jobs)
    assert [int(x) for r in res for x in r["regions"]["n_valid"]] == [257, 40, 400, 1000]
    assert all((r["regions"]["status"] == abi.OTG_REGION_OK).all() for r in res)
    assert all((r["regions"]["ic"] >= 2).all() for r in res)


def test_assemble_max_alleles_3_and_4(gpu, oracle):
    """About 150 reads drawn from three / four allele lengths, max_alleles 3 and 4 (and the default 2 on the same regions)."""
    rng = np.random.default_rng(604)
    b = deep_batch(rng, [(150, 4, (260, 300, 350)), (148, 4, (220, 260, 310, 380)), (152, 0, (300, 345, 400, 460))])
    jobs = [(abi.default_params(max_alleles=ma, max_cov=256), b) for ma in (3, 4, 2)]
    res = _assemble_parity(gpu, oracle, jobs)
    assert int(res[1]["regions"]["fc"].max()) >= 3


def test_assemble_deep_haps(gpu, oracle):
    """ignore_haps = 0 at about 150 reads with the tags of a third of them dropped: those become invalid and are reassigned."""
    rng = np.random.default_rng(605)
    b = deep_batch(rng, [(150, 3, (300, 360)), (140, 6, (250, 280))], haps=True)
    drop = rng.random(len(b["reads"])) < 1 / 3
    b["reads"]["ps"][drop] = -1
    b["reads"]["hp"][drop] = -1
    _assemble_parity(gpu, oracle, [(abi.default_params(ignore_haps=0), b)])


def test_assemble_deep_ont_and_adaptive(gpu, oracle):
    """About 100 ONT-like reads of 1 kb in one region; a deep HiFi region with the wfadaptive heuristic on."""
    rng = np.random.default_rng(606)
    b_ont = deep_batch(rng, [(100, 4, (1000, 1150))], err="ont")
    b_ad = deep_batch(rng, [_hifi(rng, 180, 4), _hifi(rng, 70, 2)])
    _assemble_parity(gpu, oracle, [(abi.default_params(), b_ont),
                                   (abi.default_params(heuristic=abi.OTG_HEURISTIC_WFADAPTIVE), b_ad)])


@pytest.mark.skipif(oracle_lib.ref_io() is None, reason="oracle/_ref/libotter_ref_io.so not built")
def test_assemble_files_deep_regions(gpu, oracle, tmp_path):
    """otg_assemble_files (BED + BAM -> SAM text through the dispatcher) with regions of 201, 300 and 399 reads next to shallow ones: under
    the default -c 200 the three deep regions are skipped, under -c 250 the 300- and 399-read ones, under -c 400 none (the 399-read region
    has 266 spanning reads: the wide clustering kernel).  The text equals the reference's own ingest -> oracle -> oracle emit, as in
    test_end_to_end_bam.py."""
    import otter_amd
    import e2e_bam
    ds = e2e_bam.make_dataset(str(tmp_path), n_regions=5, seed=73, depth=[14, 240, 14, 358, 476])
    ref_batch = e2e_bam.ingest_with_reference(ds, str(tmp_path), offset_l=1, offset_r=1, mapq=10)      # also writes reads.bam
    assert list(ref_batch["regions"]["n_reads"]) == [11, 201, 11, 300, 399]
    bam, bed = os.path.join(str(tmp_path), "reads.bam"), os.path.join(str(tmp_path), "regions.bed")
    with open(bed, "w") as f:
        for c, s, e in ds["regions"]:
            f.write("%s\t%d\t%d\n" % (c, s, e))
    beds, carena = abi.make_beds(ds["regions"])
    hdr = oracle.emit_sam_header([(ds["chrom"], ds["ref_len"])], "s1", 1, 1)
    cases = [(200, 3), (250, 2), (400, 0)]
    oras = _oracle_threads(oracle.assemble_batch, [(abi.default_params(max_cov=c), ref_batch) for c, _ in cases])
    for (c, n_skip), ora in zip(cases, oras):
        expect = hdr + oracle.emit_alleles(beds, carena, ora, "s1", False)
        text, st = otter_amd.assemble_files(bam, bed, read_group="s1", params=abi.default_params(max_cov=c), batch_regions=0,
                                            offset_l=1, offset_r=1, mapq=10, threads=2)
        assert text == expect, c
        assert st["n_regions"] == 5 and st["n_regions_skipped"] == n_skip and st["n_alleles"] == len(ora["alleles"]), (c, st)
    assert int(oras[-1]["regions"]["n_valid"][4]) > 256 and (oras[-1]["regions"]["ic"] >= 2).all()
    otter_amd.assemble_files_release()


def test_assemble_region_above_the_slot_bound(gpu):
    """One region of 65 536 reads within max_cov needs 2^32 reassignment slots: otg_assemble_submit refuses it as a capacity error that
    names the region (splitting the batch would not help), before any device work."""
    from otter_amd._lib import OtterGpuError
    n = 65536
    reads = np.zeros(n + 2, dtype=abi.read_dt)
    reads["seq_len"] = 4; reads["spanning_l"] = 1; reads["spanning_r"] = 1; reads["ps"] = -1; reads["hp"] = -1; reads["ccoord_second"] = 4
    regions = np.zeros(2, dtype=abi.region_dt)
    regions[0]["first_read"], regions[0]["n_reads"] = 0, 2
    regions[1]["first_read"], regions[1]["n_reads"] = 2, n
    b = {"arena": np.frombuffer(b"ACGT" + bytes(64), dtype=np.uint8).copy(), "reads": reads, "regions": regions}
    with pytest.raises(OtterGpuError, match="region 1: 65536 reads"):
        gpu.assemble(abi.default_params(max_cov=n), b)


def _cluster_compare(gpu, oracle, cases, **kw):
    P = abi.default_params(**kw)
    packed = pack_cluster_cases(cases)
    rc, el, eic, efc, eb = oracle.cluster_batch(P, *packed)
    assert rc == 0
    gl, gic, gfc, gb = gpu.cluster_batch(P, *packed)
    assert np.array_equal(gic, eic) and np.array_equal(gfc, efc) and np.array_equal(gl, el)
    assert np.array_equal(np.nan_to_num(gb, nan=-7.0), np.nan_to_num(eb, nan=-7.0))
    return gic, gfc


def test_cluster_wide_v_ties(gpu, oracle):
    """otg_cluster_batch at V = 257, 400 and 1000 with tie-heavy matrices (quantised to 2 and 3 decimals, and not), next to narrow regions."""
    rng = np.random.default_rng(607)
    cases = []
    for i, n in enumerate((257, 400, 1000, 257, 400, 120, 300)):
        cases.append((tie_heavy_matrix(rng, n, (2, 3, None)[i % 3]), rng.integers(300, 3000, n).astype(np.uint32)))
    _cluster_compare(gpu, oracle, cases)
    _cluster_compare(gpu, oracle, cases[:3], max_alleles=3)


def _genotype_args(rng, counts, extra=None):
    seqs, first = [], []
    for i, A in enumerate(counts):
        first.append(len(seqs))
        seqs += extra[i] if extra and extra[i] is not None else genotype_region_alleles(rng, A)
    arena, off, ln = abi.pack_seqs(seqs)
    return arena, off, ln, np.asarray(first, dtype=np.uint32), np.asarray([len(extra[i]) if extra and extra[i] is not None else A
                                                                          for i, A in enumerate(counts)], dtype=np.uint32)


def _genotype_check(gpu, oracle, args):
    P = abi.default_params()
    e = oracle.genotype_cluster_batch(P, *args)
    g = gpu.genotype_cluster_batch(P, *args)
    for i in (0, 1, 2, 4, 5):
        assert np.array_equal(g[i], e[i]), i
    assert np.allclose(g[3], e[3], rtol=1e-9, atol=0, equal_nan=True)
    return g


def test_genotype_allele_thresholds(gpu, oracle):
    """A = 102 (last LDS matrix), 103 (HBM matrices), 200, 256 (last on-chip scratch), 257, 301, 600 and 1000 (wide kernel) in one batch."""
    rng = np.random.default_rng(608)
    counts = (102, 103, 200, 256, 257, 301, 600, 1000)
    g = _genotype_check(gpu, oracle, _genotype_args(rng, counts))
    assert (g[4] >= 2).all()


def test_genotype_many_genotypes(gpu, oracle):
    """700 alleles of 150 lengths 3 % apart (each its own length cluster) and two motifs: a few hundred genotypes whose first appearances
    lie all over the region, so the first-appearance numbering runs over several rounds of 256."""
    rng = np.random.default_rng(610)
    motifs = [b"CAG", b"AATG"]
    region = []
    for _ in range(700):
        k, m = int(rng.integers(0, 150)), motifs[int(rng.integers(0, 2))]
        L = int(100 * 1.03 ** k)
        region.append((m * (L // len(m) + 1))[:L])
    g = _genotype_check(gpu, oracle, _genotype_args(rng, (0,), extra=[region]))
    assert g[4][0] > 256


def test_genotype_homopolymer_4_3mb(gpu, oracle):
    """An allele of a 4.3 Mb homopolymer and 40 kb of other sequence (its AAA count passes 2^16 in every lane's column, the other bins do
    not: a wrapped count moves the frequencies, so hsd and the 3-mer cosine move), next to ordinary alleles of the same region."""
    rng = np.random.default_rng(609)
    region = genotype_region_alleles(rng, 12)
    region.insert(5, b"A" * 4_300_000 + rand_seq(rng, 40_000))
    region.append(b"A" * 300)
    g = _genotype_check(gpu, oracle, _genotype_args(rng, (0, 20), extra=[region, None]))
    assert (g[1][:14] == g[1][5]).sum() == 1


def test_genotype_files_cohort_of_150(gpu, oracle, tmp_path):
    """otg_genotype_files on a 150-sample merged allele BAM: 301 alleles per region (the wide kernel, and the dispatcher's allele buffers
    growing past their first size), the VCF text == product ingest -> ORACLE anallele_cluster -> oracle text."""
    import otter_amd
    from otter_amd import bamwrite
    fx = bamwrite.make_genotype_fixture(str(tmp_path), 6, n_samples=150, len_range=(200, 600))
    bam = otter_amd.Bam(fx["bam"])
    samples, ol, orr = bam.sample_index()
    beds, carena = abi.make_beds(fx["regions"])
    blk = bam.ingest_alleles((beds, carena), reference=otter_amd.Fasta(fx["fasta"]), threads=2)
    so, sl, fa_, na_ = otter_amd.genotype_blocks(blk)
    assert (na_ == 301).all()
    P = abi.default_params()
    ogt, ogl, ogk, ohsd, ongt, oreps = oracle.genotype_cluster_batch(P, blk["arena"], so, sl, fa_, na_)
    exp = oracle.emit_vcf_header(bam.targets(), samples) + oracle.emit_vcf_lines(beds, carena, blk, len(samples), ogt, ohsd, ongt, oreps, ol, orr)
    text, st = otter_amd.genotype_files(fx["bam"], fx["bed"], fasta=fx["fasta"], threads=3)
    assert text == exp and st["n_regions"] == 6 and st["n_alleles"] == 6 * 301
    assert (ongt > 1).all()

"""The edit metric of the genotype clustering through the file commands: otg_genotype_files (metric), otg_cohort_files (gt_metric, with and
without its k-mer matrix) and tools/otter_cohort --gt-metric, on a cohort of 3 samples x 8 regions in which two regions carry a motif-order
pair: (CAG)n(CCG)n in the reference and two samples, (CCG)n(CAG)n in the third — one genotype by length and 3-mer usage, two by edit distance."""
import os
import subprocess
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, bamwrite
import cohort_helpers as H
import genotype_edit_ref as ger

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "otter_cohort")
PLANTED = {2: 40, 5: 60}            # region -> n of its motif-order pair (240 and 360 bp)
FLANK = 1200


def _codes(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


def make_planted_cohort(dirname, n_regions=8, n_samples=3, depth=10, seed=77, rate=0.005):
    """The layout of bamwrite.make_cohort_fixture (one reference, a sorted BED, a reads BAM per sample) with chosen alleles: a planted region's
    samples carry one of the two orders of its motif pair on both haplotypes (sample 1 the swapped one); elsewhere a sample's two alleles are
    the reference tract and a copy-number variant at least 10 % longer or shorter, far from the 0.025 cut under either metric."""
    rng = np.random.default_rng(seed)
    ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
    names = ["s%02d" % i for i in range(n_samples)]
    ref_parts, regions, loci = [], [], []
    pos = 0
    for r in range(n_regions):
        if r in PLANTED:
            a, b = ger.motif_order_pair(PLANTED[r])
            variants = [_codes(a), _codes(b)]
        else:
            motif = ACGT[rng.integers(0, 4, int(rng.integers(2, 7)))]
            L = int(rng.integers(200, 600))
            tr = np.tile(motif, L // len(motif) + 1)[:L]
            k = max(1, int(0.1 * L) // len(motif) + 1)
            variants = [tr, np.concatenate([tr, np.tile(motif, k)]), tr[:L - k * len(motif)]]
        fl, fr = ACGT[rng.integers(0, 4, FLANK)], ACGT[rng.integers(0, 4, FLANK)]
        start = pos + FLANK
        L = len(variants[0])
        ref_parts += [fl, variants[0], fr]
        regions.append(("chrC", start, start + L))
        loci.append((variants, fl, fr, start, L))
        pos += FLANK + L + FLANK
    ref = np.concatenate(ref_parts)
    bams = []
    for s in range(n_samples):
        recs = []
        for r, (variants, fl, fr, start, L) in enumerate(loci):
            if r in PLANTED:
                pick = [1, 1] if s == 1 else [0, 0]
            else:
                pick = [int(rng.integers(0, 3)), int(rng.integers(0, 3))]
            for d in range(depth):
                v = variants[pick[d % 2]]
                lf, rf = int(rng.integers(200, 900)), int(rng.integers(200, 900))
                left, c_l = bamwrite._noisy(rng, fl[FLANK - lf:], rate)
                right, c_r = bamwrite._noisy(rng, fr[:rf], rate)
                if len(v) == L:                 # the reference tract, or the swapped order: aligned base for base
                    mid, c_m = bamwrite._noisy(rng, v, rate)
                elif len(v) > L:
                    mid, c_m = bamwrite._noisy(rng, v[:L], rate)
                    mid = np.concatenate([mid, v[L:]]); c_m = np.concatenate([c_m, np.full(len(v) - L, 1, dtype=np.uint8)])
                else:
                    mid, c_m = bamwrite._noisy(rng, v, rate)
                    c_m = np.concatenate([c_m, np.full(L - len(v), 2, dtype=np.uint8)])
                recs.append((0, start - lf, "%s_r%d_%d" % (names[s], r, d), 0, 60, bamwrite._rle(np.concatenate([c_l, c_m, c_r])), np.concatenate([left, mid, right]), b""))
        recs.sort(key=lambda x: x[1])
        path = os.path.join(dirname, names[s] + ".bam")
        bamwrite.write_bam(path, [("chrC", int(ref.size))], recs)
        bams.append(path)
    bed, fa = os.path.join(dirname, "regions.bed"), os.path.join(dirname, "ref.fa")
    with open(bed, "w") as f:
        for c, s_, e in regions:
            f.write("%s\t%d\t%d\n" % (c, s_, e))
    with open(fa, "w") as f:
        f.write(">chrC\n")
        rb = ref.tobytes().decode()
        for i in range(0, len(rb), 60):
            f.write(rb[i:i + 60] + "\n")
    return {"bams": bams, "names": names, "bed": bed, "fasta": fa, "regions": regions}


def _merged_allele_bam(fx, tmp, tag, P):
    sams = [otter_amd.assemble_files(b, fx["bed"], fasta=fx["fasta"], read_group=n, params=P, threads=2)[0] for b, n in zip(fx["bams"], fx["names"])]
    bam = os.path.join(tmp, "merged_%s.bam" % tag)
    assert H.sam_to_bam_python(H.merge_sams(sams), bam) > 0
    return bam


@pytest.fixture(scope="module")
def cohort(tmp_path_factory, gpu):
    tmp = str(tmp_path_factory.mktemp("gtedit"))
    fx = make_planted_cohort(tmp)
    fx["tmp"] = tmp
    fx["merged"] = _merged_allele_bam(fx, tmp, "exact", abi.default_params())
    fx["vcf_edit"] = otter_amd.genotype_files(fx["merged"], fx["bed"], fasta=fx["fasta"], threads=2, metric="edit")[0]
    fx["vcf_length"] = otter_amd.genotype_files(fx["merged"], fx["bed"], fasta=fx["fasta"], threads=2, metric="length")[0]
    return fx


def _lines(vcf):
    return {l.split(b"\t")[2]: l for l in vcf.split(b"\n") if l and not l.startswith(b"#")}


def test_genotype_files_edit_equals_the_reference_text(cohort, oracle):
    bam = otter_amd.Bam(cohort["merged"])
    samples, ol, orr = bam.sample_index()
    beds, carena = abi.make_beds(cohort["regions"])
    blk = bam.ingest_alleles((beds, carena), reference=otter_amd.Fasta(cohort["fasta"]), threads=2)
    so, sl, fa_, na_ = otter_amd.genotype_blocks(blk)
    P = abi.default_params()
    regions = ger.region_seqs(blk["arena"], so, sl, fa_, na_)
    for r, n in PLANTED.items():            # the assembled alleles are the planted ones (behind the base --offset adds): both orders, letter for letter
        a, b = ger.motif_order_pair(n)
        assert any(s[ol:] == a for s in regions[r]) and any(s[ol:] == b for s in regions[r]), r
    mats, _ = ger.edit_matrices(regions)
    gt, gl, gk, hsd, ngt, reps = ger.genotype_with_matrix(P, blk["arena"], so, sl, fa_, na_, mats)
    exp = oracle.emit_vcf_header(bam.targets(), samples) + oracle.emit_vcf_lines(beds, carena, blk, len(samples), gt, hsd, ngt, reps, ol, orr)
    assert cohort["vcf_edit"] == exp
    # the default is the length metric, and the two texts differ in the planted regions only
    assert otter_amd.genotype_files(cohort["merged"], cohort["bed"], fasta=cohort["fasta"], threads=2)[0] == cohort["vcf_length"]
    le, ll = _lines(cohort["vcf_edit"]), _lines(cohort["vcf_length"])
    assert set(le) == set(ll) and len(le) == len(cohort["regions"])
    ids = [("%s:%d-%d" % reg).encode() for reg in cohort["regions"]]
    assert sorted(ids.index(k) for k in le if le[k] != ll[k]) == sorted(PLANTED)


@pytest.mark.parametrize("heuristic", ["exact", "wfadaptive"])
def test_cohort_files_edit_equals_genotype_files(cohort, heuristic):
    if heuristic == "exact":
        P, want = abi.default_params(), cohort["vcf_edit"]
    else:
        P = abi.default_params(heuristic=abi.OTG_HEURISTIC_WFADAPTIVE, heur_min_wavefront_length=10, heur_max_distance_threshold=50, heur_steps_between_cutoffs=1)
        merged = _merged_allele_bam(cohort, cohort["tmp"], "adaptive", P)
        want = otter_amd.genotype_files(merged, cohort["bed"], fasta=cohort["fasta"], params=P, threads=2, metric="edit")[0]
    text, st = otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], params=P, threads=2, gt_metric="edit")
    assert text == want
    assert st["n_regions"] == len(cohort["regions"])
    if heuristic == "exact":
        assert otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], params=P, threads=2)[0] == cohort["vcf_length"]


def test_cohort_matrix_follows_the_edit_genotypes(cohort):
    text, _, matrix = otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], threads=2, gt_metric="edit", matrix_k=3)
    assert text == cohort["vcf_edit"]
    vcf = os.path.join(cohort["tmp"], "edit.vcf")
    open(vcf, "wb").write(text)
    assert matrix == otter_amd.vcf2mat_files(vcf, cohort["bed"], k=3, threads=2)[0]
    _, _, matrix_length = otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], threads=2, matrix_k=3)
    assert matrix_length.count(b"\n") == matrix.count(b"\n") - len(PLANTED)      # one more ALT row per planted region


def test_cli_gt_metric(cohort):
    samples = ["%s=%s" % (n, b) for n, b in zip(cohort["names"], cohort["bams"])]
    r = subprocess.run([CLI, "-b", cohort["bed"], "-r", cohort["fasta"], "-t", "2", "--gt-metric", "edit"] + samples, capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stdout == cohort["vcf_edit"], r.stderr
    r = subprocess.run([CLI, "-b", cohort["bed"], "-r", cohort["fasta"], "-t", "2", "--gt-metric", "length"] + samples, capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stdout == cohort["vcf_length"], r.stderr
    r = subprocess.run([CLI, "-b", cohort["bed"], "-r", cohort["fasta"], "--gt-metric", "foo"] + samples, capture_output=True, timeout=600)
    assert r.returncode == 1 and r.stdout == b"" and b"[ERROR] --gt-metric length | edit" in r.stderr

"""Host-side expectations of the cohort k-mer matrix (otg_kmer_cohort_rows / otg_kmer_cohort_usage): a numpy restatement of the row list and of
the per-sample GT numbers, the same two read back from a VCF text, and a staged cohort whose reference alleles put the reference genotype in
every position."""
import os
import numpy as np
from otter_amd import abi, synth

GOLDEN_MAT_K = 3
# the rows of tests/golden/cohort_small.vcf at that k (scripts/make_golden_cohort_matrix.py)
GOLDEN_MAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cohort_small_k3.mat")


def numpy_rows(first_allele, gt, n_gt, reps, sample, n_samples):
    """The rows of the matrix and the GT pairs of the samples, from what cohort_collect returns.  A region with alleles a0 .. a0+na-1 has its
    reference allele last (ref_i = na-1) and contributes n_gt rows, the alleles of its VCF line in column order (src/genotype.cpp:149-153):
    row 0 the reference allele, row i >= 1 the allele a0 + reps[a0+i-1] (i <= ref_gt) or a0 + reps[a0+i], with ref_gt = gt[a0+ref_i].  The GT
    numbers of a sample are the re-centred gt (ref_gt -> 0, below it +1) of its first and last allele in the region; -1 -1 without one.
    -> {"n_rows", "row_first" [B+1], "row_allele" [n_rows], "sample_gt" [B, S, 2]}"""
    B, S = len(first_allele) - 1, int(n_samples)
    row_first, row_allele = [0], []
    sample_gt = np.full((B, S, 2), -1, dtype=np.int32)
    for r in range(B):
        a0, a1 = int(first_allele[r]), int(first_allele[r + 1])
        na = a1 - a0
        if na > 0:
            ref_i = na - 1
            ref_gt = int(gt[a0 + ref_i])
            for i in range(int(n_gt[r])):
                row_allele.append(a0 + (ref_i if i == 0 else int(reps[a0 + i - 1]) if i <= ref_gt else int(reps[a0 + i])))
            for s in range(S):
                mine = [a for a in range(a0, a1) if int(sample[a]) == s]
                if mine:
                    for slot, a in enumerate((min(mine), max(mine))):
                        g = int(gt[a])
                        sample_gt[r, s, slot] = 0 if g == ref_gt else g + 1 if g < ref_gt else g
        row_first.append(len(row_allele))
    return {"n_rows": len(row_allele), "row_first": np.asarray(row_first, dtype=np.uint32), "row_allele": np.asarray(row_allele, dtype=np.uint32),
            "sample_gt": sample_gt}


def row_seqs(rows, grp):
    """the bytes of every row, from the arena of a regroup / cohort_collect dict"""
    return [grp["arena"][int(grp["seq_off"][a]):int(grp["seq_off"][a]) + int(grp["seq_len"][a])].tobytes() for a in rows["row_allele"]]


def vcf_rows(vcf_text):
    """what a VCF text says about the same two: per line (ID, [REF, ALT...] with <DEL> as N and no ALT for '.', [(g1, g2) per sample] with ./. as
    (-1, -1))"""
    out = []
    for l in vcf_text.split(b"\n"):
        if not l or l.startswith(b"#"):
            continue
        f = l.split(b"\t")
        alts = [] if f[4] == b"." else [b"N" if a == b"<DEL>" else a for a in f[4].split(b",")]
        gts = []
        for col in f[9:]:
            g = col.split(b":")[0]
            gts.append((-1, -1) if g == b"./." else tuple(int(x) for x in g.split(b"/")))
        out.append((f[2], [f[3]] + alts, gts))
    return out


# ---- a staged cohort for the building blocks
N_REGIONS = 9
LONG_REF = 70_000                    # one row above 65 536 window starts: two workgroups of the HBM-histogram tier


def sample_batches(S):
    """S assemble batches over the same 9 regions; region 0 is empty in every sample, region 1 in all but sample 0, which is homozygous there
    (the seed was chosen for that)"""
    out = []
    for k in range(S):
        b = synth.make_batch(N_REGIONS, len_range=(150, 400), reads_range=(8, 14), err="hifi", seed=903 + k % 3, frac_partial=0.1, frac_het=0.8)
        for r in ([0] if k == 0 else [0, 1]):
            b["regions"][r]["n_reads"] = 0
        out.append(b)
    return out


def allele_seq(res, r, j):
    rr = res["regions"][r]
    a = res["alleles"][int(rr["first_allele"]) + j]
    return res["seqs"][int(a["seq_off"]):int(a["seq_off"]) + int(a["seq_len"])].tobytes()


def choose_refs(results, seed=11):
    """Reference alleles, one per region, from the samples' assembled alleles (results: per sample assemble_collect's dict), so that the
    reference's cluster takes every position among the clusters of its region:
      region 1: the only allele of sample 0, the only sample there -> the reference is the only distinct sequence: n_gt == 1, ALT '.'
      region 2: the first allele of sample 0                       -> ref_gt = 0
      region 3: the first allele of the middle sample              -> with three samples a middle ref_gt
      region 4: the last allele of the last sample                 -> ref_gt last, shared with a sample
      region 5: random, 70 000 bases                               -> alone and last, and a row of two tier-L workgroups
      others  : random, 40 .. 300 bases                            -> alone and last
    (the GPU test asserts on the collected gt / n_gt that these cases occurred)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    refs = [acgt[rng.integers(0, 4, int(rng.integers(40, 300)))].tobytes() for _ in range(N_REGIONS)]
    refs[1] = allele_seq(results[0], 1, 0)
    refs[2] = allele_seq(results[0], 2, 0)
    refs[3] = allele_seq(results[len(results) // 2], 3, 0)
    refs[4] = allele_seq(results[-1], 4, int(results[-1]["regions"][4]["n_alleles"]) - 1)
    refs[5] = acgt[rng.integers(0, 4, LONG_REF)].tobytes()
    return refs


def stage(gpu, other, S, P=None):
    """stages S samples on `gpu` (runs alternate between it and `other`), regroups with choose_refs and clusters -> (params, refs)"""
    P = P if P is not None else abi.default_params(max_alleles=4)
    batches = sample_batches(S)
    gpu.cohort_begin(N_REGIONS, S)
    results = []
    for k, batch in enumerate(batches):
        ctx = other if (k % 2) else gpu
        ctx.assemble_submit(P, batch)
        ctx.assemble_run()
        results.append(ctx.assemble_collect())
        gpu.cohort_stage(k, src=ctx)
    refs = choose_refs(results)
    ref_arena, ref_off, ref_len = abi.pack_seqs(refs)
    gpu.cohort_genotype(P, ref_arena, ref_off, ref_len)
    return P, refs


def make_deletion_fixture(dirname, depth=8, flank=1200, seed=5):
    """A cohort of 3 samples x 4 tandem-repeat loci with clean reads, written like bamwrite.make_cohort_fixture, in which whole-locus deletions
    occur — a zero-length allele, which the VCF prints as <DEL>:
      locus 0: s00 homozygous for the deletion, s01 and s02 the reference           -> ALT is <DEL> alone
      locus 1: s00 deletion + expansion, s01 expansion + contraction, s02 reference -> <DEL> beside other ALT alleles
      locus 2: s00 reference + expansion, s01 contraction, s02 no reads             -> ordinary
      locus 3: s00 and s01 homozygous for the deletion, s02 deletion + reference    -> <DEL> alone, shared
    Returns dict(bams, names, bed, fasta, regions)."""
    from otter_amd import bamwrite
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    names = ["s00", "s01", "s02"]
    DEL = "del"
    plan = [[(DEL, DEL), (0, 0), (0, 0)], [(DEL, 6), (6, -4), (0, 0)], [(0, 5), (-3, -3), None], [(DEL, DEL), (DEL, DEL), (DEL, 0)]]
    loci, ref_parts, regions, pos = [], [], [], 0
    for r in range(len(plan)):
        motif = acgt[rng.integers(0, 4, 3 + r)]
        L = len(motif) * (40 + 7 * r)
        tr = np.tile(motif, L // len(motif))
        fl, fr = acgt[rng.integers(0, 4, flank)], acgt[rng.integers(0, 4, flank)]
        start = pos + flank
        ref_parts += [fl, tr, fr]
        regions.append(("chrC", start, start + L))
        loci.append((motif, tr, fl, fr, start, L))
        pos += flank + L + flank
    ref = np.concatenate(ref_parts)
    bams = []
    for s, name in enumerate(names):
        recs = []
        for r, (motif, tr, fl, fr, start, L) in enumerate(loci):
            if plan[r][s] is None:
                continue
            for d in range(depth):
                dl = plan[r][s][d % 2]
                dl = -L if dl == DEL else dl * len(motif)
                lf, rf = int(rng.integers(300, 900)), int(rng.integers(300, 900))
                body = tr if dl >= 0 else tr[:L + dl]
                extra = np.tile(motif, dl // len(motif)) if dl > 0 else np.zeros(0, np.uint8)
                codes = np.concatenate([np.zeros(lf + len(body), np.uint8), np.full(len(extra), 1, np.uint8), np.full(max(-dl, 0), 2, np.uint8), np.zeros(rf, np.uint8)])
                recs.append((0, start - lf, "%s_r%d_%d" % (name, r, d), 0, 60, bamwrite._rle(codes), np.concatenate([fl[flank - lf:], body, extra, fr[:rf]]), b""))
        recs.sort(key=lambda x: x[1])
        path = os.path.join(dirname, name + ".bam")
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

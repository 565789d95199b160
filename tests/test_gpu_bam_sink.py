"""GPU: the dispatchers writing indexed allele BAMs through otg_bam_sink, and otg_bam_merge closing the loop to `otter genotype` and
`otter compare` — the file round trip include/otter_gpu.h promises for otg_cohort_files, with no Python BAM writer in between.

1. per-sample assemble_files(bam_out=) -> merge_bams -> genotype_files gives the bytes of cohort_files' VCF;
2. cohort_files(alleles_bam=) writes per-sample BAMs whose inflated streams equal those of 1;
3. a shuffled BED: sort=True gives the inflated stream of the sorted BED, sort=False fails with the sink's line number;
4. compare_files on sink-written truth / query BAMs prints what it prints on the bamwrite-written ones;
5. the command-line hosts: otter_assemble --bam, otter_merge, then genotype_files."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import otter_amd
from otter_amd import bamwrite
from compare_fixtures import ROOT, aux, write_allele_bam
from helpers import rand_seq, mutate, tr_seq

pytestmark = pytest.mark.gpu


def _inflated(path):
    return gzip.decompress(open(path, "rb").read())


@pytest.fixture(scope="module")
def cohort(tmp_path_factory, gpu):
    tmp = str(tmp_path_factory.mktemp("bam_sink"))
    fx = bamwrite.make_cohort_fixture(tmp, 12, 3, depth=8, len_range=(200, 500))
    fx["tmp"] = tmp
    fx["vcf"], _ = otter_amd.cohort_files(fx["bams"], fx["names"], fx["bed"], fx["fasta"], threads=2)
    fx["allele_bams"] = []
    for b, n in zip(fx["bams"], fx["names"]):
        out = os.path.join(tmp, "alleles_%s.bam" % n)
        text, st = otter_amd.assemble_files(b, fx["bed"], fasta=fx["fasta"], read_group=n, threads=2, bam_out=out)
        assert text == b"" and st["n_alleles"] > 0 and os.path.exists(out + ".bai")
        fx["allele_bams"].append(out)
    return fx


def test_assemble_bam_merge_genotype_equals_cohort(cohort):
    merged = os.path.join(cohort["tmp"], "merged.bam")
    n = otter_amd.merge_bams(cohort["allele_bams"], merged, threads=2)
    assert n > 30
    vcf, _ = otter_amd.genotype_files(merged, cohort["bed"], fasta=cohort["fasta"], threads=2)
    assert vcf == cohort["vcf"]
    assert len([l for l in vcf.split(b"\n") if l and not l.startswith(b"#")]) >= 10


def test_cohort_alleles_bam_equals_assemble_bam(cohort):
    outs = [os.path.join(cohort["tmp"], "cohort_%s.bam" % n) for n in cohort["names"]]
    vcf, _, sams = otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], threads=2, alleles=True, alleles_bam=outs)
    assert vcf == cohort["vcf"]
    for o, a, sam in zip(outs, cohort["allele_bams"], sams):
        assert _inflated(o) == _inflated(a)
        assert open(o + ".bai", "rb").read() == open(a + ".bai", "rb").read()
        assert sam.count(b"\tta:Z:") > 5
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.cohort_files(cohort["bams"], cohort["names"], cohort["bed"], cohort["fasta"], alleles_bam=outs[:2])


def test_shuffled_bed_needs_the_sort(cohort):
    lines = open(cohort["bed"]).read().splitlines()
    order = np.random.default_rng(3).permutation(len(lines))
    assert list(order) != sorted(order)
    bed = os.path.join(cohort["tmp"], "shuffled.bed")
    open(bed, "w").write("".join(lines[int(i)] + "\n" for i in order))
    bam, name = cohort["bams"][0], cohort["names"][0]
    out = os.path.join(cohort["tmp"], "shuffled.bam")
    otter_amd.assemble_files(bam, bed, fasta=cohort["fasta"], read_group=name, threads=2, bam_out=out, sort=True)
    assert _inflated(out) == _inflated(cohort["allele_bams"][0])
    # the same job without the sort: the sink refuses the first record that goes back, and the error says which line that was
    text, _ = otter_amd.assemble_files(bam, bed, fasta=cohort["fasta"], read_group=name, threads=2)
    last, bad = -1, None
    for i, l in enumerate(text.split(b"\n")):
        if l and not l.startswith(b"@"):
            pos = int(l.split(b"\t")[3])
            if pos < last:
                bad = i + 1
                break
            last = pos
    assert bad is not None
    out2 = os.path.join(cohort["tmp"], "unsorted.bam")
    with pytest.raises(otter_amd.OtterGpuError) as e:
        otter_amd.assemble_files(bam, bed, fasta=cohort["fasta"], read_group=name, threads=2, bam_out=out2, sort=False)
    assert "otg_assemble_files failed" in str(e.value) and "line %d: out of order" % bad in str(e.value), str(e.value)
    assert not os.path.exists(out2) and not os.path.exists(out2 + ".bai")
    # and the dispatcher is as usable as before
    assert otter_amd.assemble_files(bam, bed, fasta=cohort["fasta"], read_group=name, threads=2)[0] == text


def _sam_tags(tags):
    return "".join("\t%s:%s:%s" % t for t in tags)


def test_compare_on_sink_written_bams(tmp_path):
    """the allele records of tests/compare_fixtures.py's shape, once through bamwrite and once as SAM text through the sink"""
    rng = np.random.default_rng(8)
    chrom, n_regions = "chrC", 24
    recs = {"truth": [], "asm": []}
    regions = []
    for r in range(n_regions):
        s, e = 1000 + 3000 * r, 1000 + 3000 * r + 200
        name = "%s:%d-%d" % (chrom, s, e)
        n_t = [2, 2, 2, 1, 3, 0, 2][r % 7]
        hap = [tr_seq(rng, int(rng.integers(50, 600))) if r % 3 else rand_seq(rng, int(rng.integers(50, 600))) for _ in range(max(n_t, 2))]
        for a in range(n_t):
            v = "ubl rn"[(r + a) % 6]
            recs["truth"].append((s + a, "%s_h%d_%d" % (chrom, a, r), hap[a], [("RG", "Z", "truth"), ("ta", "Z", name)] + ([("sp", "A", v)] if v != " " else [])))
        for a in range([2, 1, 4, 2, 2, 2, 0][r % 7]):
            q = b"N" if (r % 11 == 5 and a == 0) else mutate(rng, hap[a % 2], 0.02 * (a + 1))
            recs["asm"].append((s + a, "%s_%d" % (name, a), q, [("RG", "Z", "asm"), ("ta", "Z", name)]))
        regions.append((chrom, s, e))
    ref_len = 3000 * n_regions + 2000
    bed = str(tmp_path / "regions.bed")
    open(bed, "w").write("".join("%s\t%d\t%d\n" % r for r in regions))
    paths = {}
    for side, rgs in (("truth", ["truth"]), ("asm", ["asm", "other"])):
        paths[side, "bamwrite"] = write_allele_bam(str(tmp_path / (side + "_w.bam")), chrom, ref_len, rgs,
                                                   [(p, n, q, b"".join(aux(*t) for t in tags)) for p, n, q, tags in recs[side]])
        text = "@SQ\tSN:%s\tLN:%d\n" % (chrom, ref_len) + "".join("@RG\tID:%s\n" % g for g in rgs) + "@PG\tID:otter\tOF:1,0\n"
        for p, n, q, tags in recs[side]:
            text += "%s\t0\t%s\t%d\t60\t%dM\t*\t0\t0\t%s\t*%s\n" % (n, chrom, p + 1, len(q), q.decode(), _sam_tags(tags))
        paths[side, "sink"] = str(tmp_path / (side + "_s.bam"))
        with otter_amd.BamSink(paths[side, "sink"], sort=True, threads=2) as sk:
            sk.write(text.encode())
        assert sk.n_records == len(recs[side])
    want = otter_amd.compare_files(paths["truth", "bamwrite"], paths["asm", "bamwrite"], bed, threads=2)
    got = otter_amd.compare_files(paths["truth", "sink"], paths["asm", "sink"], bed, threads=2)
    assert got[0] == want[0] and got[1] == want[1]
    assert want[0].count(b"\n") >= 2 * 10 and want[1].count(b"WARNING") > 0


def test_command_line_hosts(cohort):
    tmp = cohort["tmp"]
    two = [0, 2]
    outs = []
    for s in two:
        out = os.path.join(tmp, "cli_%s.bam" % cohort["names"][s])
        r = subprocess.run([os.path.join(ROOT, "tools", "otter_assemble"), "-b", cohort["bed"], "-R", cohort["names"][s], "-r", cohort["fasta"], "-t", "2",
                            "--bam", out, cohort["bams"][s]], capture_output=True, timeout=600)
        assert r.returncode == 0 and r.stdout == b"", r.stderr
        assert _inflated(out) == _inflated(cohort["allele_bams"][s])
        outs.append(out)
    merged = os.path.join(tmp, "cli_merged.bam")
    r = subprocess.run([os.path.join(ROOT, "tools", "otter_merge"), "-t", "2", merged] + outs, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    vcf, _ = otter_amd.genotype_files(merged, cohort["bed"], fasta=cohort["fasta"], threads=2)
    want, _ = otter_amd.cohort_files([cohort["bams"][s] for s in two], [cohort["names"][s] for s in two], cohort["bed"], cohort["fasta"], threads=2)
    assert vcf == want
    # usage errors and refusals of the hosts
    r = subprocess.run([os.path.join(ROOT, "tools", "otter_assemble"), "-b", cohort["bed"], "-R", "x", "--fasta", "--bam", os.path.join(tmp, "no.bam"), cohort["bams"][0]],
                       capture_output=True, timeout=600)
    assert r.returncode == 1 and b"--fasta" in r.stderr and not os.path.exists(os.path.join(tmp, "no.bam"))
    r = subprocess.run([os.path.join(ROOT, "tools", "otter_merge"), os.path.join(tmp, "no.bam"), outs[0], outs[0]], capture_output=True, timeout=600)
    assert r.returncode == 1 and b"ID:" + cohort["names"][two[0]].encode() in r.stderr and not os.path.exists(os.path.join(tmp, "no.bam"))
    # otter_cohort --alleles-prefix P --alleles-bam: the per-sample files as BAM + BAI, same stem
    prefix = os.path.join(tmp, "co_")
    r = subprocess.run([os.path.join(ROOT, "tools", "otter_cohort"), "-b", cohort["bed"], "-r", cohort["fasta"], "-t", "2", "--alleles-prefix", prefix, "--alleles-bam"] +
                       ["%s=%s" % (cohort["names"][s], cohort["bams"][s]) for s in two], capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    for s in two:
        assert _inflated(prefix + cohort["names"][s] + ".bam") == _inflated(cohort["allele_bams"][s])
        assert os.path.exists(prefix + cohort["names"][s] + ".bam.bai") and not os.path.exists(prefix + cohort["names"][s] + ".sam")

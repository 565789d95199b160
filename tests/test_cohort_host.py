"""CPU: the cohort path's host side — the golden joint VCF re-derived from the oracle (guards scripts/make_golden_cohort.py), the C layout
of otg_cohort_job, the exported symbols, the command-line tool, the fixture generator and the helpers the GPU tests rely on."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import otter_amd
from otter_amd import abi, bamwrite
import cohort_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otter_gpu.h")
COHORT_SYMBOLS = ["otg_cohort_begin", "otg_cohort_stage", "otg_cohort_regroup", "otg_cohort_genotype", "otg_cohort_result_sizes", "otg_cohort_collect",
                  "otg_cohort_end", "otg_cohort_files"]


def test_golden_vcf_rederived_from_the_oracle(oracle, tmp_path):
    fx = H.golden_fixture(str(tmp_path))
    text, printed, grp = H.oracle_cohort(oracle, fx)
    assert text == open(H.GOLDEN_VCF, "rb").read()
    # the condition the generator puts on the fixture: no printed hsd near a boundary of the 6-digit rounding (device and oracle agree to 1e-9)
    assert H.hsd_boundary_margin(printed) > 1e-7
    lines = [l.split(b"\t") for l in text.split(b"\n") if l and not l.startswith(b"#")]
    assert len(lines) >= 10 and all(len(l) == 9 + len(fx["names"]) for l in lines)
    assert text.split(b"\n#CHROM")[1].split(b"\n")[0].split(b"\t")[9:] == [n.encode() for n in fx["names"]]
    assert sum(1 for l in lines if l[4] != b".") >= 6                          # polymorphic loci
    genotypes = [g.split(b":")[0] for l in lines for g in l[9:]]
    assert len(set(genotypes)) >= 4 and genotypes.count(b"0/0") >= 3            # samples share alleles with each other and the reference


def test_cohort_job_layout_matches_c(tmp_path):
    fields = [n for n, _ in abi.CohortJob._fields_]
    src = tmp_path / "cj.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "otter_gpu.h"\nint main(){printf("%zu", sizeof(otg_cohort_job));\n' +
                   "".join('printf(" %%zu", offsetof(otg_cohort_job, %s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "cj"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.CohortJob)] + [getattr(abi.CohortJob, f).offset for f in fields]
    assert C.sizeof(abi.ALLELE_WRITE_FN) == C.sizeof(C.c_void_p)


def test_cohort_symbols_are_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(otg_cohort_[a-z_0-9]+)\s*\(", txt))
    assert declared == set(COHORT_SYMBOLS)
    lib = otter_amd.load()
    for n in COHORT_SYMBOLS:
        assert n in otter_amd.EXPORTS and getattr(lib, n) is not None, n
    for m in ("cohort_begin", "cohort_stage", "cohort_regroup", "cohort_genotype", "cohort_collect", "cohort_end"):
        assert callable(getattr(otter_amd.Context, m)), m
    assert callable(otter_amd.cohort_files)


def test_cohort_calls_fail_loudly_without_a_context():
    lib = otter_amd.load()
    assert lib.otg_cohort_begin(None, C.c_uint32(4), C.c_uint32(2)) == abi.OTG_ERR_NO_DEVICE
    assert lib.otg_cohort_stage(None, None, C.c_uint32(0)) == abi.OTG_ERR_NO_DEVICE
    assert lib.otg_cohort_genotype(None, None) == abi.OTG_ERR_NO_DEVICE


def test_tool_builds_and_prints_usage():
    from otter_amd import build
    build.build_tool()
    exe = os.path.join(ROOT, "tools", "otter_cohort")
    assert os.path.exists(exe)
    p = subprocess.run([exe], capture_output=True)
    assert p.returncode == 1 and b"usage: otter_cohort -b <BED> -r <FASTA>" in p.stderr
    p = subprocess.run([exe, "-b", "x.bed", "-r", "x.fa", "nameless.bam"], capture_output=True)
    assert p.returncode == 1 and b"NAME=<BAM>" in p.stderr


def test_cohort_fixture_shape(tmp_path):
    fx = bamwrite.make_cohort_fixture(str(tmp_path), 9, 3, depth=6, len_range=(150, 300), seed=3)
    assert fx["names"] == ["s00", "s01", "s02"] and len(fx["bams"]) == 3
    starts = [s for _, s, _ in fx["regions"]]
    assert starts == sorted(set(starts))                                        # sorted, no two regions with the same start
    beds, carena, skipped = otter_amd.parse_bed_file(fx["bed"])
    assert otter_amd.bed_tuples(beds, carena) == fx["regions"] and skipped == 0
    tg = [otter_amd.Bam(b).targets() for b in fx["bams"]]
    assert tg[0] == tg[1] == tg[2] and tg[0][0][0] == "chrC"
    fa = otter_amd.Fasta(fx["fasta"])
    assert fa.seqs() == tg[0]
    n_reads = [len(otter_amd.Bam(b).ingest((beds, carena), offset_l=1, offset_r=0)["reads"]) for b in fx["bams"]]
    assert all(6 * 5 <= n <= 6 * 9 for n in n_reads)
    # deterministic in the seed
    os.makedirs(str(tmp_path / "again"))
    again = bamwrite.make_cohort_fixture(str(tmp_path / "again"), 9, 3, depth=6, len_range=(150, 300), seed=3)
    b0, b1 = otter_amd.Bam(fx["bams"][1]).ingest((beds, carena)), otter_amd.Bam(again["bams"][1]).ingest((beds, carena))
    assert b0["arena"].tobytes() == b1["arena"].tobytes() and open(again["fasta"]).read() == open(fx["fasta"]).read()


def test_numpy_regroup_and_sam_merge_helpers(tmp_path):
    """the expectations the GPU tests compare against, on a hand-made case"""
    def res(alleles_per_region, seqs):
        rr = np.zeros(len(alleles_per_region), dtype=abi.region_result_dt)
        al = np.zeros(sum(alleles_per_region), dtype=abi.allele_dt)
        arena, off, ln = abi.pack_seqs(seqs)
        k = 0
        for r, n in enumerate(alleles_per_region):
            rr[r]["first_allele"] = k; rr[r]["n_alleles"] = n
            for j in range(n):
                al[k]["seq_off"] = off[k]; al[k]["seq_len"] = ln[k]; al[k]["region"] = r; al[k]["label"] = j; al[k]["tcov"] = 10 + k; al[k]["ps"] = -1; al[k]["hp"] = -1
                k += 1
        return {"regions": rr, "alleles": al, "seqs": arena}
    g = H.numpy_regroup([res([2, 0, 1], [b"AAAA", b"CC", b""]), res([1, 0, 0], [b"GGG"])], [b"TTTTT", b"ACGT", b"AC"])
    assert list(g["first_allele"]) == [0, 4, 4, 6] and list(g["n_alleles"]) == [4, 0, 2]
    assert g["arena"][:g["seq_bytes"]].tobytes() == b"AAAACCGGGTTTTTNAC"
    assert list(g["sample"]) == [0, 0, 1, 2, 0, 2] and list(g["alleles"]["label"]) == [0, 0, 1, 2, 0, 2]
    assert list(g["seq_len"]) == [4, 2, 3, 5, 1, 2] and list(g["alleles"]["region"]) == [0, 0, 0, 0, 2, 2]
    assert list(g["alleles"]["tcov"]) == [10, 11, 10, 1, 12, 1]
    hdr = "@SQ\tSN:c\tLN:900\n@RG\tID:%s\n@PG\tID:otter\tOF:1,0\n"
    rec = "c:%d-%d_%d\t0\tc\t%d\t0\t4M\t*\t0\t0\tACGT\t!!!!\tRG:Z:%s\tta:Z:c:%d-%d\ttc:i:9\tac:i:4\tsc:i:4\tic:i:2\tse:f:0.00123457\n"
    a = (hdr % "x" + rec % (10, 20, 0, 10, "x", 10, 20) + rec % (50, 60, 0, 50, "x", 50, 60)).encode()
    b = (hdr % "y" + rec % (10, 20, 0, 10, "y", 10, 20) + rec % (10, 20, 1, 10, "y", 10, 20) + rec % (30, 40, 0, 30, "y", 30, 40)).encode()
    m = H.merge_sams([a, b]).decode().split("\n")
    assert m[:5] == ["@HD\tVN:1.4\tSO:coordinate", "@SQ\tSN:c\tLN:900", "@RG\tID:x", "@RG\tID:y", "@PG\tID:otter\tOF:1,0"]
    assert [(l.split("\t")[0], l.split("\t")[11]) for l in m[5:] if l] == [("c:10-20_0", "RG:Z:x"), ("c:10-20_0", "RG:Z:y"), ("c:10-20_1", "RG:Z:y"), ("c:30-40_0", "RG:Z:y"), ("c:50-60_0", "RG:Z:x")]
    bam = str(tmp_path / "m.bam")
    assert H.sam_to_bam_python(H.merge_sams([a, b]), bam) == 5
    h = otter_amd.Bam(bam)
    assert h.sample_index() == (["x", "y"], 1, 0)
    blk = h.ingest_alleles([("c", 10, 20), ("c", 30, 40), ("c", 50, 60)])
    assert list(blk["first_allele"]) == [0, 3, 4, 5] and list(blk["alleles"]["label"]) == [0, 1, 1, 1, 0]
    assert np.array_equal(blk["alleles"]["se"], np.full(5, np.float32(0.00123457))) and list(blk["alleles"]["acov"]) == [4] * 5
    assert H.hsd_boundary_margin([1.0, 2.5, 1.2345649999]) < 1e-9 and H.hsd_boundary_margin([1.0, 2.0341]) > 1e-7

"""`otter compare` end to end on the device: otg_compare_files on allele BAMs written with bamwrite equals the C++ restatement of compare()
(tests/edit_align_ref.cpp) for every batch size, the command-line host prints the same, and the adapter's WFAlignerEdit(Alignment) returns
the op strings of otg_edit_align_batch."""
import os
import subprocess

import numpy as np
import pytest

import otter_amd
from compare_fixtures import ROOT, build_ref, ref_align, ref_compare, oriented, aux, write_allele_bam
from helpers import rand_seq, mutate, tr_seq, pair_tasks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("edit_align_ref_cmp"))


def _fixture(tmp_path, n_regions=40):
    """truth BAM (records named after the chromosome, sp:A tags, 0-3 alleles per region) and query BAM (0-4 assembled alleles: near copies
    of the truth haplotypes, sometimes an "N" placeholder); returns (bed path, truth bam, query bam, restatement input)"""
    rng = np.random.default_rng(8)
    chrom = "chrC"
    trecs, qrecs, regions, lines = [], [], [], []
    for r in range(n_regions):
        s, e = 1000 + 3000 * r, 1000 + 3000 * r + 200
        name = "%s:%d-%d" % (chrom, s, e)
        ta = aux("ta", "Z", name)
        n_t = [2, 2, 2, 1, 3, 0, 2][r % 7]
        hap = [tr_seq(rng, int(rng.integers(50, 800))) if r % 3 else rand_seq(rng, int(rng.integers(50, 800))) for _ in range(max(n_t, 2))]
        truth, sp = [], []
        for a in range(n_t):
            v = "ubl rn"[(r + a) % 6]
            tags = aux("RG", "Z", "truth") + ta + (aux("sp", "A", v) if v != " " else b"")
            trecs.append((s + a, "%s_h%d_%d" % (chrom, a, r), hap[a], tags))
            truth.append(hap[a])
            sp.append({" ": -1, "u": -1, "b": 0, "l": 1, "r": 2, "n": 3}[v])        # no sp tag: 'u' (src/compare.cpp:34)
        n_q = [2, 1, 4, 2, 2, 2, 0][r % 7]
        query = []
        for a in range(n_q):
            q = b"N" if (r % 11 == 5 and a == 0) else mutate(rng, hap[a % 2], 0.02 * (a + 1))
            qrecs.append((s + a, "%s_%d" % (name, a), q, aux("RG", "Z", "asm") + ta))
            query.append(q)
        regions.append((chrom, s, e))
        lines.append((name, truth, sp, query))
    tb = write_allele_bam(str(tmp_path / "truth.bam"), chrom, 3000 * n_regions + 2000, ["truth"], trecs)
    qb = write_allele_bam(str(tmp_path / "query.bam"), chrom, 3000 * n_regions + 2000, ["asm", "other"], qrecs)
    bed = str(tmp_path / "regions.bed")
    with open(bed, "w") as f:
        for c, s, e in regions:
            f.write("%s\t%d\t%d\n" % (c, s, e))
    return bed, tb, qb, lines


def test_compare_files_matches_restatement(tmp_path, ref_exe):
    bed, tb, qb, lines = _fixture(tmp_path)
    want, want_w = ref_compare(ref_exe, lines)
    outs = []
    for br in (1, 7, 0):
        text, warn, st = otter_amd.compare_files(tb, qb, bed, threads=2, batch_regions=br)
        outs.append(text)
        assert sorted(warn.splitlines()) == sorted(want_w.splitlines())
        assert st["n_regions"] == len(lines)
    assert outs[0] == want
    assert outs[1] == want and outs[2] == want
    # the command-line host prints the same
    exe = os.path.join(ROOT, "tools", "otter_compare")
    r = subprocess.run([exe, "-b", bed, "-R", "ignored", "-t", "2", tb, qb], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want


def test_adapter_edit_alignment_scope(tmp_path, gpu):
    exe = str(tmp_path / "edit_align_driver")
    lib = os.path.join(ROOT, "otter_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include", "wfa_adapter"), "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "adapter_edit", "edit_align_driver.cpp"), "-L" + lib, "-lotter_gpu",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(4)
    pairs = [(b"AB", b"BA"), (b"ACGT", b"-"[:0])]
    for n in (10, 100, 1000, 3000):
        a = tr_seq(rng, n)
        pairs.append(oriented(a, mutate(rng, a, 0.05)))
    inp = "".join("%s %s\n" % (p.decode() or "-", t.decode() or "-") for p, t in pairs).encode()
    r = subprocess.run([exe], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    scores, cigs = gpu.edit_align_batch(*pair_tasks(pairs))
    got = [line.split(" ") for line in r.stdout.decode().splitlines()]
    assert len(got) == len(pairs)
    for (st, sc, cg), s, c in zip(got, scores, cigs):
        assert st == "0" and int(sc) == int(s)
        assert cg.encode() == (c if c else b"-")
        assert cg != "-" or len(c) == 0

"""`otter compare` host layers (no device): the ABI structs, the region logic otg_compare_emit against the C++ restatement of compare()
(tests/edit_align_ref.cpp; src/compare.cpp:106-146), and the two allele ingests against the reference's own build (query side) and
hand-derived expectations (truth side, src/compare.cpp:26-48)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import otter_amd
from otter_amd import abi
import oracle_lib
from compare_fixtures import ROOT, build_ref, ref_align, ref_compare, pair_plan, oriented, aux, write_allele_bam
from helpers import rand_seq, mutate, tr_seq


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("edit_align_ref"))


def test_abi_struct_sizes(tmp_path):
    src = tmp_path / "sz.cpp"
    src.write_text('#include "otter_gpu.h"\n#include <cstddef>\n#include <cstdio>\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(otg_compare_job), '
                   'offsetof(otg_compare_job, warn), offsetof(otg_compare_job, warn_user), sizeof(otg_compare_counts));}\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(abi.CompareJob), abi.CompareJob.warn.offset, abi.CompareJob.warn_user.offset, C.sizeof(abi.CompareCounts)]


def _block(seq_lists):
    """[[seq, ...] per region] -> an allele block as the ingest returns it"""
    seqs = [s for lst in seq_lists for s in lst]
    arena, offs, lens = abi.pack_seqs(seqs)
    al = np.zeros(len(seqs), dtype=abi.allele_dt)
    al["seq_off"] = offs; al["seq_len"] = lens
    first = np.zeros(len(seq_lists) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(x) for x in seq_lists])
    return {"alleles": al, "first_allele": first, "arena": arena}


def _crafted(rng):
    a, b = rand_seq(rng, 300), rand_seq(rng, 280)
    tr = tr_seq(rng, 240)
    regions = [
        ("chr1:100-200", [a, b], [0, 1], [mutate(rng, a, 0.03), mutate(rng, b, 0.05)]),                       # ordinary
        ("chr1:300-400", [a, b], [-1, 2], [mutate(rng, b, 0.02)]),                                            # one query allele: duplicated
        ("chr1:500-600", [a, b, tr], [0, 0, 0], [a]),                                                         # > 2 truth alleles
        ("chr1:700-800", [a], [3], [a]),                                                                      # one truth allele
        ("chr1:900-1000", [], [], [a]),                                                                       # none
        ("chr1:1100-1200", [a, b], [0, 1], []),                                                               # no query alleles
        ("chr1:1300-1400", [b"N", b"NDNNN"], [1, 2], [b"NDNNN", b"N", tr]),                                   # the placeholders
        ("chr1:1500-1600", [tr, mutate(rng, tr, 0.1)], [2, 0], [mutate(rng, tr, 0.05), tr[:200] + b"A" * 40]), # equal lengths: pattern = query
        ("chr1:1700-1800", [a, b], [1], [mutate(rng, a, 0.2) for _ in range(6)] + [mutate(rng, b, 0.2) for _ in range(4)]),  # 20 edges; spannings short
        ("chr1:1900-2000", [a, b], [0, 1, 2, 3], [a, b]),                                                     # more spannings than alleles
        ("chr1:2100-2200", [b"N", b"NDNNN"], [0, 1], [(b"ACGT" * 308642)[:1234567]]),                        # %g exponent form: 1.23457e+06
        ("chr1:2300-2400", [b"AB", b"CD"], [0, 0], [b"BA", b"DC", b"AB"]),                                    # swapped pairs: op-string ties
    ]
    return regions


def _emit_inputs(exe, regions):
    truth = _block([r[1] for r in regions])
    query = _block([r[3] for r in regions])
    sp = [v for r in regions for v in r[2]]
    truth["spannings"] = np.asarray(sp if sp else [0], dtype=np.int32)[:len(sp)]
    truth["first_spanning"] = np.concatenate([[0], np.cumsum([len(r[2]) for r in regions])]).astype(np.uint32)
    pairs, pfirst = [], [0]
    for _, t, _, q in regions:
        pairs += pair_plan(t, q)
        pfirst.append(len(pairs))
    # pairs the reference does not align (equal, "N" / "NDNNN") get junk values: otg_compare_emit must ignore them
    special = [t == q or t in (b"N", b"NDNNN") or q in (b"N", b"NDNNN") for t, q in pairs]
    todo = [oriented(t, q) for (t, q), sp in zip(pairs, special) if not sp]
    res = iter(ref_align(exe, todo) if todo else [])
    edit, ops = np.full(len(pairs), -7.0), np.full(len(pairs), -7.0)
    for i, sp in enumerate(special):
        if not sp:
            s, o = next(res)
            edit[i], ops[i] = s, len(o)
    beds = abi.make_beds([(n.split(":")[0], int(n.split(":")[1].split("-")[0]), int(n.split("-")[1])) for n, _, _, _ in regions])
    return beds, truth, query, np.asarray(pfirst, dtype=np.uint64), edit, ops


def test_compare_emit_matches_restatement(ref_exe):
    rng = np.random.default_rng(11)
    regions = _crafted(rng)
    beds, truth, query, pfirst, edit, ops = _emit_inputs(ref_exe, regions)
    text, warn, counts = otter_amd.compare_emit(beds, truth, query, pfirst, edit, ops)
    want, want_w = ref_compare(ref_exe, regions)
    assert text == want
    assert warn == want_w
    assert counts == {"n_compared": 8, "skip_many_truth": 1, "skip_one_truth": 1, "skip_no_truth": 1, "skip_no_query": 1}
    assert b"1.23457e+06" in text


def test_compare_emit_random_regions(ref_exe):
    rng = np.random.default_rng(5)
    regions = []
    for r in range(40):
        base = tr_seq(rng, int(rng.integers(20, 120))) if r % 2 else rand_seq(rng, int(rng.integers(20, 120)))
        t = [mutate(rng, base, 0.1) for _ in range(2)]
        q = [mutate(rng, x, 0.08) for x in (t * 5)[:int(rng.integers(1, 10))]]
        regions.append(("chrR:%d-%d" % (100 * r, 100 * r + 50), t, [int(v) for v in rng.integers(-1, 4, int(rng.integers(0, 4)))], q))
    beds, truth, query, pfirst, edit, ops = _emit_inputs(ref_exe, regions)
    text, warn, _ = otter_amd.compare_emit(beds, truth, query, pfirst, edit, ops)
    assert (text, warn) == ref_compare(ref_exe, regions)


def test_edit_align_restatement_diamond_equals_full(ref_exe):
    """the device kernel computes only the diamond |k - kend| <= s - t: on the restatement the op strings are the same"""
    rng = np.random.default_rng(3)
    pairs = [(b"AB", b"BA"), (b"ACGT", b""), (b"", b"ACG"), (b"AAAA", b"AAAA")]
    for _ in range(300):
        n = int(rng.integers(1, 90))
        a = tr_seq(rng, n) if rng.integers(0, 2) else rand_seq(rng, n)
        b = mutate(rng, a, float(rng.choice([0.05, 0.2, 0.5])))
        if rng.integers(0, 4) == 0:
            b = b[:int(rng.integers(0, len(b) + 1))]
        pairs.append(oriented(a, b))
    full = ref_align(ref_exe, pairs)
    assert ref_align(ref_exe, pairs, diamond=True) == full
    assert full[0] == (2, b"XX")                # mismatch beats deletion beats insertion
    for (p, t), (s, o) in zip(pairs, full):
        assert o.count(b"M") + o.count(b"X") + o.count(b"D") == len(p) and o.count(b"M") + o.count(b"X") + o.count(b"I") == len(t)
        assert len(o) - o.count(b"M") == s


def _truth_and_query_bams(tmp_path, same_names=False, unknown_rg=False):
    chrom = "chrT"
    rng = np.random.default_rng(2)
    regions = [(chrom, 1000 + 400 * r, 1100 + 400 * r) for r in range(6)]
    trecs, qrecs, expect_sp = [], [], []
    tname = "asm" if same_names else "truth"
    for r, (c, s, e) in enumerate(regions):
        ta = aux("ta", "Z", "%s:%d-%d" % (c, s, e))
        sps = []
        for a in range(r % 4):
            seq = rand_seq(rng, int(rng.integers(30, 90)))
            sp = ["u", "b", "l", "r", "n", "x", None, "int"][(r + a) % 8]
            tags = aux("RG", "Z", tname) + ta
            if sp == "int":
                tags += aux("sp", "i", 7)
            elif sp is not None:
                tags += aux("sp", "A", sp)
            trecs.append((s + a, "%s_%d_%d" % (c, r, a), seq, tags))
            sps.append({"u": -1, None: -1, "b": 0, "l": 1, "r": 2, "n": 3}.get(sp, "none"))
        # a record whose name does not start with the chromosome: ignored entirely; one whose ta names another region: only its sp counts
        trecs.append((s + 5, "other_%d" % r, b"ACGTACGT", aux("RG", "Z", tname) + ta + aux("sp", "A", "b")))
        trecs.append((s + 6, "%s_wrongta_%d" % (c, r), b"ACGT", aux("RG", "Z", tname) + aux("ta", "Z", "x:1-2") + aux("sp", "A", "l")))
        sps.append(1)
        expect_sp.append([v for v in sps if v != "none"])
        for a in range((r + 1) % 3):
            seq = rand_seq(rng, int(rng.integers(30, 90)))
            qrecs.append((s + a, "%s:%d-%d_%d" % (c, s, e, a), seq, aux("RG", "Z", "asm") + ta + aux("tc", "i", 5)))
    if unknown_rg:
        c, s, e = regions[1]
        qrecs.append((s + 9, "bad", b"ACGT", aux("RG", "Z", "nobody") + aux("ta", "Z", "%s:%d-%d" % (c, s, e))))
    tb = write_allele_bam(str(tmp_path / "truth.bam"), chrom, 10000, [tname, "second"], trecs)
    qb = write_allele_bam(str(tmp_path / "query.bam"), chrom, 10000, ["asm"], qrecs)
    return regions, tb, qb, expect_sp, tname


@pytest.mark.parametrize("same_names", [False, True])
def test_compare_ingest_truth_side(tmp_path, same_names):
    regions, tb, qb, expect_sp, tname = _truth_and_query_bams(tmp_path, same_names=same_names)
    bam = otter_amd.Bam(tb)
    blk = bam.ingest_compare(regions + [("nochr", 1, 2)], tname, "asm", truth=True, threads=2)
    n = [int(blk["first_allele"][r + 1] - blk["first_allele"][r]) for r in range(len(regions))]
    assert n == [r % 4 for r in range(len(regions))]
    got_sp = [blk["spannings"][blk["first_spanning"][r]:blk["first_spanning"][r + 1]].tolist() for r in range(len(regions))]
    assert got_sp == expect_sp
    # the map has one key (-> 1) when both first read groups are equal
    assert set(blk["alleles"]["label"].tolist()) <= ({1} if same_names else {0})
    assert blk["warn"] == b"WARNING: query failed at region nochr:1-2\n"


def test_compare_ingest_unknown_read_group(tmp_path):
    regions, tb, qb, _, tname = _truth_and_query_bams(tmp_path, unknown_rg=True)
    with pytest.raises(otter_amd.OtterGpuError) as e:
        otter_amd.Bam(qb).ingest_compare(regions, tname, "asm", truth=False)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)


@pytest.mark.skipif(oracle_lib.ref_io() is None, reason="oracle/_ref/libotter_ref_io.so not built")
def test_compare_ingest_query_side_matches_reference(tmp_path):
    from test_genotype_io import _ref_ingest_alleles
    regions, tb, qb, _, tname = _truth_and_query_bams(tmp_path)
    got = otter_amd.Bam(qb).ingest_compare(regions, tname, "asm", truth=False)
    ref = _ref_ingest_alleles(qb, None, regions)
    assert np.array_equal(got["first_allele"], ref["first_allele"])
    for f in ("seq_off", "seq_len", "scov", "acov", "tcov", "se", "ic", "ps", "hp", "region"):
        assert np.array_equal(got["alleles"][f], ref["alleles"][f]), f
    assert (got["alleles"]["label"] == 1).all()       # "asm" is index 1 of compare's map (0 in the BAM's own index)
    n = int(ref["alleles"]["seq_len"].astype(np.int64).sum())
    assert got["arena"][:n].tobytes() == ref["arena"][:n].tobytes()

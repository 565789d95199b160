"""`otter compare` under wfadaptive: otg_compare_files with a heuristic named in the job equals otg_compare_emit fed with the adaptive
restatement's (score, columns) per pair, for every batch size; tools/otter_compare --wfa-heuristic prints the same; the fixture separates the
two modes and the default stays exact.  The adapter's WFAlignerEdit(Alignment) after setHeuristicWFadaptive returns the op strings of
otg_edit_align_heur_batch, and the exact ones again after setHeuristicNone."""
import os
import subprocess

import numpy as np
import pytest

import otter_amd
from otter_amd import abi
import adaptive_align_fixtures as fx
from compare_fixtures import ROOT, pair_plan, aux, write_allele_bam
from helpers import pair_tasks

pytestmark = pytest.mark.gpu

N_REGIONS = 12


def _regions():
    """12 regions of two truth alleles = the patterns of two MID pairs, the query alleles = their texts; the first regions take the MID pairs
    whose adaptive op string differs from the exact one.  Region 3 has a single query allele, region 7 an "N" in place of its first."""
    mid = fx.input_set("MID")
    differ = [i for i, (a, e) in enumerate(zip(fx.adaptive_ref("MID"), fx.exact_ref("MID"))) if a[2] != e[1]]
    assert len(differ) == 7
    order = differ + [i for i in range(len(mid)) if i not in differ]
    out = []
    for r in range(N_REGIONS):
        x, y = order[2 * r], order[2 * r + 1]
        truth = [mid[x][0], mid[y][0]]
        query = [mid[x][1], mid[y][1]]
        if r == 3:
            query = query[:1]
        if r == 7:
            query[0] = b"N"
        out.append(("chrA:%d-%d" % (1000 + 5000 * r, 1200 + 5000 * r), truth, [0, 1], query))
    return out


def _special(t, q):
    return t == q or t in (b"N", b"NDNNN") or q in (b"N", b"NDNNN")


def _block(seq_lists):
    seqs = [s for lst in seq_lists for s in lst]
    arena, offs, lens = abi.pack_seqs(seqs)
    al = np.zeros(len(seqs), dtype=abi.allele_dt)
    al["seq_off"] = offs; al["seq_len"] = lens
    first = np.zeros(len(seq_lists) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(x) for x in seq_lists])
    return {"alleles": al, "first_allele": first, "arena": arena}


def _expected(regions, align):
    """the text of otg_compare_emit with per pair the (score, columns) `align` gives for the oriented pairs"""
    truth = _block([r[1] for r in regions])
    query = _block([r[3] for r in regions])
    sp = [v for r in regions for v in r[2]]
    truth["spannings"] = np.asarray(sp, dtype=np.int32)
    truth["first_spanning"] = np.concatenate([[0], np.cumsum([len(r[2]) for r in regions])]).astype(np.uint32)
    pairs, pfirst = [], [0]
    for _, t, _, q in regions:
        pairs += pair_plan(t, q)
        pfirst.append(len(pairs))
    todo = [fx.oriented(t, q) for t, q in pairs if not _special(t, q)]
    res = iter(align(todo))
    edit, ops = np.full(len(pairs), -7.0), np.full(len(pairs), -7.0)
    for i, (t, q) in enumerate(pairs):
        if not _special(t, q):
            s, n = next(res)
            edit[i], ops[i] = s, n
    beds = abi.make_beds([(n.split(":")[0], int(n.split(":")[1].split("-")[0]), int(n.split("-")[1])) for n, _, _, _ in regions])
    text, _, counts = otter_amd.compare_emit(beds, truth, query, np.asarray(pfirst, dtype=np.uint64), edit, ops)
    assert counts["n_compared"] == len(regions)
    return text


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("compare_adaptive")
    regions = _regions()
    chrom = "chrA"
    trecs, qrecs = [], []
    for r, (name, truth, sp, query) in enumerate(regions):
        s = int(name.split(":")[1].split("-")[0])
        ta = aux("ta", "Z", name)
        for a, seq in enumerate(truth):
            trecs.append((s + a, "%s_h%d_%d" % (chrom, a, r), seq, aux("RG", "Z", "truth") + ta + aux("sp", "A", "bl"[a])))
        for a, seq in enumerate(query):
            qrecs.append((s + a, "%s_%d" % (name, a), seq, aux("RG", "Z", "asm") + ta))
    ref_len = 5000 * N_REGIONS + 10000
    tb = write_allele_bam(str(tmp / "truth.bam"), chrom, ref_len, ["truth"], trecs)
    qb = write_allele_bam(str(tmp / "query.bam"), chrom, ref_len, ["asm"], qrecs)
    bed = str(tmp / "regions.bed")
    with open(bed, "w") as f:
        for name, _, _, _ in regions:
            f.write("%s\t%s\t%s\n" % (name.split(":")[0], name.split(":")[1].split("-")[0], name.split("-")[1]))
    want_adaptive = _expected(regions, lambda prs: [(s, len(o)) for s, _, o in fx.run_adaptive_ref(prs, fx.DEFAULT)])
    want_exact = _expected(regions, lambda prs: [(s, len(o)) for s, o in fx.run_exact_ref(prs)])
    # the fixture separates the modes (checked on the CPU, with the two restatements)
    assert sum(1 for a, e in zip(want_adaptive.splitlines(), want_exact.splitlines()) if a != e) >= 1
    return bed, tb, qb, want_adaptive, want_exact


def test_compare_files_adaptive_matches_restatement(fixture):
    bed, tb, qb, want, want_exact = fixture
    for br in (1, 5, 0):
        text, warn, st = otter_amd.compare_files(tb, qb, bed, threads=2, batch_regions=br, heuristic=fx.DEFAULT)
        assert text == want, br
        assert st["n_regions"] == N_REGIONS and st["n_regions_ok"] == N_REGIONS
    # the default is exact, as before, and differs on this fixture
    text, _, _ = otter_amd.compare_files(tb, qb, bed, threads=2)
    assert text == want_exact
    assert otter_amd.compare_files(tb, qb, bed, threads=2, heuristic=None)[0] == want_exact
    assert want != want_exact


def test_otter_compare_tool_option(fixture):
    bed, tb, qb, want, want_exact = fixture
    exe = os.path.join(ROOT, "tools", "otter_compare")
    r = subprocess.run([exe, "-b", bed, "-R", "ignored", "-t", "2", "--wfa-heuristic", "wfadaptive", tb, qb], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    r = subprocess.run([exe, "-b", bed, "--wfa-heuristic", "wfadaptive:10,50,1", tb, qb], capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    r = subprocess.run([exe, "-b", bed, "--wfa-heuristic", "none", tb, qb], capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stdout == want_exact, r.stderr
    r = subprocess.run([exe, "-b", bed, "--wfa-heuristic", "banded", tb, qb], capture_output=True, timeout=600)
    assert r.returncode == 1 and b"--wfa-heuristic" in r.stderr


def test_adapter_edit_alignment_under_wfadaptive(tmp_path, gpu):
    exe = str(tmp_path / "driver")
    lib = os.path.join(ROOT, "otter_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include", "wfa_adapter"), "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "adapter_edit_adaptive", "driver.cpp"), "-L" + lib, "-lotter_gpu",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    mid = fx.input_set("MID")
    differ = [i for i, (a, e) in enumerate(zip(fx.adaptive_ref("MID"), fx.exact_ref("MID"))) if a[2] != e[1]]
    pairs = fx.input_set("HAND") + [mid[i] for i in (differ + [0, 1, 2])[:6]]
    inp = "".join("%s %s\n" % (p.decode() or "-", t.decode() or "-") for p, t in pairs).encode()
    r = subprocess.run([exe] + [str(x) for x in fx.DEFAULT], input=inp, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    arena, tasks = pair_tasks(pairs)
    got = [line.split(" ") for line in r.stdout.decode().splitlines()]
    assert len(got) == 2 * len(pairs)
    adaptive = gpu.edit_align_heur_batch(arena, tasks, abi.OTG_HEURISTIC_WFADAPTIVE, *fx.DEFAULT)
    exact = gpu.edit_align_batch(arena, tasks)
    for half, (scores, cigs) in ((got[:len(pairs)], adaptive), (got[len(pairs):], exact)):
        for (st, sc, cg), s, c in zip(half, scores, cigs):
            assert st == "0" and int(sc) == int(s)
            assert cg.encode() == (c if c else b"-")
    assert adaptive[1] != exact[1]

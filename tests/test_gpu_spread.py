"""GPU: the spread operator (otg_assemble_spread) against tests/spread_ref.py, exactly.

The batches are planted (tests/spread_cases.py): every read is flank + unit-set repeat + flank.  The labels and the rows come from the
device's own otg_spread_read output; the records, the unit records and the offsets must equal the reference computed from them, and every
test asserts that the shapes it is about occurred.
1. the table: one, two and eight units, no set, no calls and no reference tract, a region over max_cov, non-spanning reads, identical reads;
2. member counts 1 .. 5, 63, 64, 65, 64 R, 64 R + 1 and a deep allele, on both tiers;  3. an expansion-biased allele;
4. realign = 1: the rows are the trimmed descriptors;  5. other scores, min_score at one read's score;  6. device_tensor;
7. the reads' locus records afterwards, by task;  8. the refusals;  9. the row text over the operator's results, and assemble_files unchanged."""
import hashlib
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from otter_amd import abi, synth
import spread_cases as Cs
import spread_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_COV = 400


def _run(gpu, batch, unit_sets, region_set, params=None, scores=(2, 7, 7, 24), **kw):
    """assemble + spread on the session context -> (res, (records, unit_off, units, reads))"""
    P = params if params is not None else abi.default_params(max_cov=MAX_COV)
    res = gpu.assemble(P, batch)
    out = gpu.assemble_spread(unit_sets, region_set, *scores, **kw)
    return res, out


def _check(batch, res, out, unit_sets, region_set, scores=(2, 7, 7, 24)):
    """the device's records against the reference on the device's own rows and labels; -> the reference's read records"""
    rec, unit_off, units, reads = out
    assert np.array_equal(reads["label"], res["labels"]) and len(reads) == len(batch["reads"])
    # counted and task are what the rule says of the labels, the flags of the descriptors and the region states
    t = 0
    for r, g in enumerate(batch["regions"]):
        for i in range(int(g["first_read"]), int(g["first_read"]) + int(g["n_reads"])):
            rd = batch["reads"][i]
            want = int(res["regions"]["status"][r] == 0 and region_set[r] is not None and reads["label"][i] >= 0 and bool(rd["spanning_l"]) and bool(rd["spanning_r"]))
            assert reads["counted"][i] == want, (r, i)
            assert reads["task"][i] == (t if want else abi.SPREAD_NONE)
            t += want
    ref = S.spread(batch["arena"], reads, res, batch["regions"], region_set, unit_sets, scores)
    assert np.array_equal(unit_off, ref[1])
    for a in range(len(rec)):
        assert rec[a].tobytes() == ref[0][a].tobytes(), (a, rec[a], ref[0][a])
    assert units.tobytes() == ref[2].tobytes() and rec.tobytes() == ref[0].tobytes()
    for r in rec:
        assert list(r["q"]) == sorted(r["q"]) and r["n_below"] + r["n_above"] <= r["n_called"] <= r["n_reads"] and r["reserved"] == 0
    return ref[3]


@pytest.fixture(scope="module")
def table(gpu):
    rng = np.random.default_rng(20260)
    batch, unit_sets, region_set, planted = Cs.planted_batch(rng, Cs.table_specs(MAX_COV))
    res, out = _run(gpu, batch, unit_sets, region_set)
    return batch, unit_sets, region_set, planted, res, out


def test_table_of_shapes(table):
    batch, unit_sets, region_set, planted, res, out = table
    _check(batch, res, out, unit_sets, region_set)
    rec, unit_off, units, reads = out
    al, rg = res["alleles"], res["regions"]
    of = lambda r: [a for a in range(len(al)) if al[a]["region"] == r]
    assert [len(of(r)) for r in range(8)] == [2, 2, 2, 1, 1, 0, 1, 1]                       # the planted grouping
    for r in (0, 1, 2):
        for a in of(r):
            assert rec[a]["flags"] == 0 and rec[a]["n_called"] >= 6 and unit_off[a + 1] - unit_off[a] == len(unit_sets[region_set[r]])
    a = of(0)[0]
    assert units[unit_off[a]]["ref_bases"] == rec[a]["ref_bases"] and list(units[unit_off[a]]["q"]) == list(rec[a]["q"])      # one unit: the total
    assert rec[of(0)[0]]["q"][0] < rec[of(0)[0]]["q"][4]                                    # the scatter is seen
    a = of(3)[0]
    assert rec[a]["flags"] == abi.SPREAD_NO_SET and rec[a]["n_reads"] == 0 and unit_off[a + 1] == unit_off[a]
    a = of(4)[0]
    assert rec[a]["flags"] == abi.SPREAD_NO_CALLS | abi.SPREAD_REF_NONE and rec[a]["n_reads"] == 6 and rec[a]["n_called"] == 0
    assert rg["status"][5] == 1 and rg["n_alleles"][5] == 0                                 # over max_cov: no alleles, no rows
    g = batch["regions"][5]
    assert not reads["counted"][int(g["first_read"]):int(g["first_read"]) + int(g["n_reads"])].any()
    g = batch["regions"][6]
    sl = slice(int(g["first_read"]), int(g["first_read"]) + int(g["n_reads"]))
    part = ~((batch["reads"]["spanning_l"][sl] == 1) & (batch["reads"]["spanning_r"][sl] == 1))
    assert part.sum() == 4 and (reads["label"][sl][part] >= 0).any() and not reads["counted"][sl][part].any()      # reassigned, not counted
    assert rec[of(6)[0]]["n_reads"] == 8
    a = of(7)[0]
    assert rec[a]["ref_bases"] >= 66 and list(rec[a]["q"]) == [rec[a]["ref_bases"]] * 5 and (rec[a]["n_below"], rec[a]["n_above"], rec[a]["n_called"]) == (0, 0, 9)


@pytest.fixture(scope="module")
def depths():
    rng = np.random.default_rng(20261)
    return Cs.planted_batch(rng, Cs.depth_specs(), err=0.003)


def test_member_counts_on_both_tiers(gpu, depths):
    batch, unit_sets, region_set, planted = depths
    res, out = _run(gpu, batch, unit_sets, region_set)
    _check(batch, res, out, unit_sets, region_set)
    rec = out[0]
    assert list(rec["n_called"]) == [1, 3, 4, 5, 63, 64, 65, Cs.R64, Cs.R64 + 1, 300, 6, 2] and list(rec["n_reads"]) == list(rec["n_called"])
    assert [int(g["n_reads"]) for g in batch["regions"]][7:10] == [Cs.R64, Cs.R64 + 1, 300]      # the last region of the register tier, the first beyond it
    # the same through the re-read tier alone, in a fresh process (the switch is read once)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import otter_amd, spread_cases as Cs\nfrom otter_amd import abi\n"
            "b, us, rs, _ = Cs.planted_batch(np.random.default_rng(20261), Cs.depth_specs(), err=0.003)\n"
            "with otter_amd.Context(0) as c:\n    c.assemble(abi.default_params(max_cov=%d), b)\n    o = c.assemble_spread(us, rs)\n"
            "sys.stdout.buffer.write(o[0].tobytes() + o[2].tobytes())\n") % (ROOT, os.path.join(ROOT, "tests"), MAX_COV)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300, env=dict(os.environ, OTG_SPREAD_REREAD="1"))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout == out[0].tobytes() + out[2].tobytes()


def test_expansion_biased_allele(gpu):
    rng = np.random.default_rng(20262)
    batch, unit_sets, region_set, planted = Cs.planted_batch(rng, Cs.expansion_specs(), err=0.002)
    res, out = _run(gpu, batch, unit_sets, region_set)
    _check(batch, res, out, unit_sets, region_set)
    rec = out[0]
    assert len(rec) == 1 and rec[0]["ref_bases"] == 90 and rec[0]["q"][2] == 90                # the consensus sits at the mode
    assert rec[0]["n_above"] >= 6 > rec[0]["n_below"] and rec[0]["sum_above"] > rec[0]["sum_below"] and rec[0]["q"][4] == 90 + 17 * 3


def _guess_unit(arena, rd):
    """a unit for a region of synth.make_batch: the best period 2..6 of the middle of one spanning read"""
    s = arena[int(rd["seq_off"]):int(rd["seq_off"]) + int(rd["seq_len"])].tobytes()
    mid = s[len(s) // 2 - 30:len(s) // 2 + 30]
    p = min(range(2, 7), key=lambda p: (sum(mid[i] != mid[i + p] for i in range(len(mid) - p)), p))
    return mid[:p]


def test_realigned_rows_are_the_trimmed_descriptors(gpu):
    batch = synth.make_batch(4, len_range=(150, 400), n_reads=12, err="hifi", seed=77, realign=True)
    unit_sets, region_set = [], []
    for g in batch["regions"]:
        rd = next(batch["reads"][i] for i in range(int(g["first_read"]), int(g["first_read"]) + int(g["n_reads"])) if batch["reads"][i]["spanning_l"] and batch["reads"][i]["spanning_r"])
        region_set.append(len(unit_sets)); unit_sets.append([_guess_unit(batch["arena"], rd)])
    P = abi.default_params(realign=1, max_cov=MAX_COV)
    res, out = _run(gpu, batch, unit_sets, region_set, params=P)
    rec, unit_off, units, reads = out
    after = np.zeros(len(batch["reads"]), dtype=abi.read_dt)
    gpu._check(gpu._L.otg_assemble_collect_reads(gpu._h, abi.ptr(after), len(after)), "otg_assemble_collect_reads")
    assert np.array_equal(reads["seq_off"], after["seq_off"]) and np.array_equal(reads["seq_len"], after["seq_len"])
    assert (reads["seq_len"] != batch["reads"]["seq_len"]).any()                               # a rescued read is the trimmed one
    rescued = (after["spanning_l"] == 1) & (after["spanning_r"] == 1) & ~((batch["reads"]["spanning_l"] == 1) & (batch["reads"]["spanning_r"] == 1))
    assert (reads["counted"][rescued] == 1).any()
    _check(dict(batch, reads=after), res, out, unit_sets, region_set)
    assert (rec["n_called"] > 0).any()


def test_other_scores_and_min_score_at_a_reads_score(gpu, table):
    batch, unit_sets, region_set, planted = table[:4]
    scores = (3, 5, 9, 30)
    res, out = _run(gpu, batch, unit_sets, region_set, scores=scores)
    recs = _check(batch, res, out, unit_sets, region_set, scores)
    assert out[0].tobytes() != table[5][0].tobytes()
    # min_score at the lowest score among the called reads of region 0 keeps that read, one above it drops it
    g = batch["regions"][0]
    low = min(recs[i][0][0] for i in range(int(g["first_read"]), int(g["first_read"]) + int(g["n_reads"])) if recs[i] is not None and recs[i][0][7] == 0)
    called = []
    for ms in (low, low + 1):
        sc = (3, 5, 9, ms)
        out2 = gpu.assemble_spread(unit_sets, region_set, *sc)
        _check(batch, res, out2, unit_sets, region_set, sc)
        called.append(int(out2[0]["n_called"][[a for a in range(len(out2[0])) if res["alleles"][a]["region"] == 0]].sum()))
    assert called[0] > called[1]


def test_device_tensors_and_the_reads_locus_records(gpu, table):
    batch, unit_sets, region_set, planted, res, _ = table
    gpu.assemble(abi.default_params(max_cov=MAX_COV), batch)
    host = gpu.assemble_spread(unit_sets, region_set)
    dev = gpu.assemble_spread(unit_sets, region_set, device_tensor=True)
    assert dev[0].is_cuda and dev[0].cpu().numpy().tobytes() == host[0].tobytes() and dev[1].cpu().numpy().astype(np.uint64).tobytes() == host[1].tobytes()
    assert dev[2].cpu().numpy().tobytes() == host[2].tobytes() and dev[3].cpu().numpy().tobytes() == host[3].tobytes()
    recs = _check(batch, res, host, unit_sets, region_set)
    # the locus results on the context are now the reads' records, by task
    loci, seg_off, segs = gpu.locus_last()
    reads = host[3]
    assert len(loci) == int(reads["counted"].sum()) > 40
    n = 0
    for i in range(len(reads)):
        if not reads["counted"][i]:
            assert recs[i] is None
            continue
        t = int(reads["task"][i])
        want, wsegs = recs[i]
        assert tuple(int(x) for x in loci[t]) == tuple(want), (i, t)
        assert [tuple(int(x) for x in s) for s in segs[int(seg_off[t]):int(seg_off[t + 1])]] == [tuple(s) for s in wsegs]
        n += 1
    assert n == len(loci)
    ms = gpu.spread_last_ms()
    assert len(ms) == 4 and ms[0] >= ms[1] + ms[2] + ms[3] > 0 and ms[3] > 0


def test_refusals(gpu, table):
    batch, unit_sets, region_set = table[:3]
    with otter_amd.Context(0) as fresh:
        with pytest.raises(otter_amd.OtterGpuError, match="no completed run"):
            fresh.assemble_spread(unit_sets, region_set)
    gpu.assemble(abi.default_params(max_cov=MAX_COV), batch)
    for bad, msg in ((dict(region_set=region_set[:-1]), "regions, the latest run has"), (dict(region_set=[99] + region_set[1:]), "names set 99"),
                     (dict(unit_sets=[[b""]] + unit_sets[1:]), "has 0 bytes"), (dict(unit_sets=[[b"A"] * 9] + unit_sets[1:]), "at most 8"),
                     (dict(match=0), "match"), (dict(indel=65), "indel"), (dict(min_score=2 ** 24 + 1), "min_score")):
        kw = dict(unit_sets=unit_sets, region_set=region_set)
        kw.update(bad)
        with pytest.raises(otter_amd.OtterGpuError, match=msg) as e:
            gpu.assemble_spread(**kw)
        assert "otg_assemble_spread failed (%d)" % abi.OTG_ERR_ARG in str(e.value)
    gpu.assemble_spread(unit_sets, region_set)                                                   # and the context still works


def test_spread_files_and_the_tool(gpu, tmp_path):
    """otg_spread_files and tools/otter_spread on a small BAM (tests/e2e_bam.py's dataset, the SAM turned into a BAM by the library's own
    sink) with a catalogue BED: the bytes of spread_emit over the operator-level chain on the same inputs, whatever the batch size."""
    import e2e_bam
    ds = e2e_bam.make_dataset(str(tmp_path), n_regions=6, seed=81, depth=10)
    bam = os.path.join(str(tmp_path), "reads.bam")
    with otter_amd.BamSink(bam, sort=False) as sink:
        sink.write(open(ds["sam"], "rb").read())
    with open(ds["fasta"]) as f:
        ref = "".join(line.strip() for line in f if not line.startswith(">"))
    unit_sets, region_set = [], []
    cat = os.path.join(str(tmp_path), "catalogue.bed")
    with open(cat, "w") as f:
        for r, (c, s, e) in enumerate(ds["regions"]):
            tr = ref[s:e]
            p = next(p for p in range(1, 7) if all(tr[i] == tr[i % p] for i in range(len(tr))))
            if r == 3:                                                                      # a catalogue record without units
                region_set.append(None)
                f.write("%s\t%d\t%d\t.\n" % (c, s, e))
            else:
                region_set.append(len(unit_sets)); unit_sets.append([tr[:p].encode()])
                f.write("%s\t%d\t%d\tID=L%d;MOTIFS=%s\n" % (c, s, e, r, tr[:p]))
    assert otter_amd.parse_bed_units(cat) == [[] if q is None else unit_sets[q] for q in region_set]
    kw = dict(offset_l=1, offset_r=1, mapq=10)
    b = otter_amd.Bam(bam)
    batch = b.ingest(ds["regions"], **kw)
    b.close()
    res = gpu.assemble(abi.default_params(), batch)
    out = gpu.assemble_spread(unit_sets, region_set, 2, 7, 7, 24)
    _check(batch, res, out, unit_sets, region_set)
    beds, carena = abi.make_beds(ds["regions"])
    want = otter_amd.spread_emit(beds, carena, res, region_set, unit_sets, out[0], out[1], out[2])
    assert want.count(b"\n") == len(res["alleles"]) >= 6 and (out[0]["n_called"] > 0).sum() >= 5 and b"\t.\t0\t0\t0\t" in want
    gpu.trim()
    for batch_regions in (0, 2):
        text, st = otter_amd.spread_files(bam, cat, batch_regions=batch_regions, threads=2, **kw)
        assert text == want, batch_regions
        assert st["n_regions"] == 6 and st["n_alleles"] == len(res["alleles"]) and st["output_bytes"] == len(text)
    # other scores reach the operator
    sc = (3, 5, 9, 30)
    out2 = gpu.assemble_spread(unit_sets, region_set, *sc)
    assert otter_amd.spread_files(bam, cat, threads=2, match=3, mismatch=5, indel=9, min_score=30, **kw)[0] == \
        otter_amd.spread_emit(beds, carena, res, region_set, unit_sets, out2[0], out2[1], out2[2])
    with pytest.raises(otter_amd.OtterGpuError, match="--scores"):
        otter_amd.spread_files(bam, cat, match=17, **kw)
    tool = os.path.join(ROOT, "tools", "otter_spread")
    assert os.path.exists(tool)
    p = subprocess.run([tool, "-b", cat, "-o", "1,1", "-m", "10", "-t", "2", "--batch", "4", bam], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    assert p.stdout == want
    p = subprocess.run([tool, "-b", cat, "--min-score", "99999999", bam], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"--min-score" in p.stderr


def test_row_text_and_assemble_files_unchanged(gpu, table, tmp_path):
    batch, unit_sets, region_set, planted, res, out = table
    regions = [("chrP", 1000 * r, 1000 * r + 60) for r in range(len(batch["regions"]))]
    beds, carena = abi.make_beds(regions)
    text = otter_amd.spread_emit(beds, carena, res, region_set, unit_sets, out[0], out[1], out[2])
    want = b""
    for a, A in enumerate(res["alleles"]):
        r = int(A["region"])
        us = None if region_set[r] is None else unit_sets[region_set[r]]
        want += S.row(b"chrP:%d-%d" % (regions[r][1], regions[r][2]), int(A["label"]), int(A["seq_len"]), us, out[0][a], out[2][int(out[1][a]):int(out[1][a + 1])])
    assert text == want and text.count(b"\n") == len(res["alleles"]) == 10
    # otg_assemble_files writes what it wrote before the operator existed
    import spread_files_fixture as F
    fx = F.make(str(tmp_path))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "spread_assemble_files.json")))
    gpu.trim()
    sam, st = otter_amd.assemble_files(fx["bam"], fx["bed"], **F.KW)
    assert (hashlib.sha256(sam).hexdigest(), len(sam), int(st["n_alleles"]), int(st["n_regions"])) == (gold["sha256"], gold["bytes"], gold["n_alleles"], gold["n_regions"])

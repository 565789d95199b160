"""Two builds of the library against each other on the file dispatchers (otg_*_files): the same seeded fixtures, at the sizes bench.py and
scripts/bench_{cohort,compare,vcf2mat}.py time, through the entry points of the source tree given by --tree (a checkout with its library
built).  One fresh process per call, so that two trees can be run in turn:
  fixture NAME DIR --tree T   build one fixture (e2e, vcf, cohort, compare, vcf2mat) under DIR/NAME; the generators are seeded
  digest DIR --tree T         "RESULT {case: SHA-256 of everything the command writes, integer fields of otg_job_stats}"
  time DIR --tree T           "RESULT {leg: wall_s, ms_ingest, ms_hot_path, ms_emit}": per leg one untimed warm-up, one timed run
  table LOGDIR OUT.json       digest_{parent,result}.log and time_{parent,result}_<round>.log (the output of the calls above) -> the table:
                              cases that differ; per leg the rounds, the medians, the parent's max - min, and whether the result's median
                              wall is within the parent's median + that spread
(vcf2mat at k = 3 only: at k = 6 the text of 50 000 records is several gigabytes.)"""
import hashlib
import json
import os
import sys
import time

tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "tests"))
sys.path.insert(0, os.path.join(tree, "scripts"))
import otter_amd                     # noqa: E402
from otter_amd import abi, bamwrite  # noqa: E402

assert os.path.dirname(os.path.abspath(otter_amd.__file__)) == os.path.join(os.path.abspath(tree), "otter_amd")
T = 16


def sha(b):
    return hashlib.sha256(b).hexdigest()


def ints(st):
    return {k: v for k, v in st.items() if isinstance(v, int)}


def fixture(name, d):
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    if name == "e2e":
        fx = bamwrite.make_tr_fixture(d, 10000, depth=30, len_range=(1000, 5000), seed=7)
        with open(fx["bed"]) as f:
            lines = f.readlines()
        fx["prefix"] = os.path.join(d, "prefix.bed")
        with open(fx["prefix"], "w") as f:
            f.writelines(lines[:300])
    elif name == "vcf":
        fx = bamwrite.make_genotype_fixture(d, 5000, n_samples=50, len_range=(1000, 5000), seed=11)
    elif name == "cohort":
        fx = bamwrite.make_cohort_fixture(d, 1000, 8, depth=20, len_range=(1000, 3000), seed=41)
    elif name == "compare":
        import bench_compare
        bench_compare.make_job(d, 10000)
        fx = dict(bed=os.path.join(d, "regions.bed"), tb=os.path.join(d, "truth.bam"), qb=os.path.join(d, "query.bam"))
    elif name == "vcf2mat":
        import bench_vcf2mat
        fx = dict(vcf=os.path.join(d, "bench.vcf"), bed=os.path.join(d, "bench.bed"))
        bench_vcf2mat.make_vcf(fx["vcf"], 50000)
        open(fx["bed"], "w").write("chr1\t0\t100\n")
    json.dump({k: v for k, v in fx.items() if k != "regions"}, open(os.path.join(d, "fx.json"), "w"))
    print("fixture %s: %.1f s" % (name, time.time() - t0), flush=True)


def paths(d):
    return {n: json.load(open(os.path.join(d, n, "fx.json"))) for n in ("e2e", "vcf", "cohort", "compare", "vcf2mat")}


def legs(p):
    e, v, c, m, k = p["e2e"], p["vcf"], p["cohort"], p["compare"], p["vcf2mat"]
    return {
        "e2e": lambda: otter_amd.assemble_files(e["bam"], e["bed"], read_group="s1", batch_regions=0, offset_l=1, offset_r=1, mapq=10, threads=T),
        "files_to_vcf": lambda: otter_amd.genotype_files(v["bam"], v["bed"], fasta=v["fasta"], threads=T),
        "cohort": lambda: otter_amd.cohort_files(c["bams"], c["names"], c["bed"], c["fasta"], threads=T),
        "compare": lambda: otter_amd.compare_files(m["tb"], m["qb"], m["bed"], threads=8),
        "vcf2mat_k3": lambda: otter_amd.vcf2mat_files(k["vcf"], k["bed"], k=3, threads=T),
    }


def digest(d):
    p = paths(d)
    e, v, c, m, k = p["e2e"], p["vcf"], p["cohort"], p["compare"], p["vcf2mat"]
    out = {}

    def rec(name, res):
        st = [x for x in res if isinstance(x, dict)][0]
        blobs = []
        for x in res:
            if isinstance(x, bytes):
                blobs.append(sha(x))
            elif isinstance(x, list):
                blobs.append([sha(y) for y in x])
        out[name] = {"sha256": blobs, "bytes": sum(len(x) for x in res if isinstance(x, bytes)), "stats": ints(st)}
        print("digest %-40s %s" % (name, blobs[0][:16]), flush=True)
    kw = dict(read_group="s1", offset_l=1, offset_r=1, mapq=10, threads=T)
    for devs in (None, [0, 0]):
        tag = "dev%s" % ("None" if devs is None else "00")
        rec("assemble/full/b0/" + tag, otter_amd.assemble_files(e["bam"], e["bed"], batch_regions=0, devices=devs, **kw))
        for b in (0, 7):
            variants = {
                "plain": {}, "fasta": dict(fasta=e["fasta"]), "reads_only": dict(reads_only=True), "reads_only_fasta": dict(reads_only=True, fasta=e["fasta"]),
                "is_fasta": dict(is_fasta=True), "adaptive": dict(params=abi.default_params(heuristic=abi.OTG_HEURISTIC_WFADAPTIVE)),
                "adaptive_fasta": dict(params=abi.default_params(heuristic=abi.OTG_HEURISTIC_WFADAPTIVE), fasta=e["fasta"]),
            }
            for name, extra in variants.items():
                rec("assemble/prefix/b%d/%s/%s" % (b, tag, name), otter_amd.assemble_files(e["bam"], e["prefix"], batch_regions=b, devices=devs, **dict(kw, **extra)))
    rec("genotype/fasta", otter_amd.genotype_files(v["bam"], v["bed"], fasta=v["fasta"], threads=T))
    rec("genotype/table", otter_amd.genotype_files(v["bam"], v["bed"], fasta=None, threads=T))
    rec("cohort/alleles", otter_amd.cohort_files(c["bams"], c["names"], c["bed"], c["fasta"], threads=T, alleles=True))
    rec("cohort/alleles/b0/dev00", otter_amd.cohort_files(c["bams"], c["names"], c["bed"], c["fasta"], threads=T, alleles=True, devices=[0, 0]))
    rec("compare", otter_amd.compare_files(m["tb"], m["qb"], m["bed"], threads=8))
    rec("vcf2mat/k3", otter_amd.vcf2mat_files(k["vcf"], k["bed"], k=3, threads=T))
    return out


def timed(d):
    out = {}
    for name, call in legs(paths(d)).items():
        call()                                       # untimed warm-up: contexts, workspaces, file cache
        t0 = time.perf_counter()
        res = call()
        wall = time.perf_counter() - t0
        st = [x for x in res if isinstance(x, dict)][0]
        out[name] = {"wall_s": round(wall, 4), "ms_ingest": round(st["ms_ingest"], 1), "ms_hot_path": round(st["ms_hot_path"], 1), "ms_emit": round(st["ms_emit"], 1)}
        print("time %-14s %s" % (name, out[name]), flush=True)
    return out


def table(d, out_path):
    import glob
    import statistics

    def result(path):
        for line in open(path):
            if line.startswith("RESULT "):
                return json.loads(line[7:])
        raise SystemExit("no RESULT in " + path)

    dp, dr = result(os.path.join(d, "digest_parent.log")), result(os.path.join(d, "digest_result.log"))
    diff = [k for k in sorted(set(dp) | set(dr)) if dp.get(k) != dr.get(k)]
    print("digests: %d cases, %d differ %s" % (len(dp), len(diff), diff))
    rounds = {t: [result(p) for p in sorted(glob.glob(os.path.join(d, "time_%s_*.log" % t)))] for t in ("parent", "result")}
    out = {"what": "parent against result, alternating fresh processes on one MI355X; per process and leg one untimed warm-up and one timed run",
           "same_bytes": {"cases": len(dp), "differing": diff, "sha256_first_output": {k: v["sha256"][0] for k, v in dr.items()}},
           "legs": {}}
    ok = not diff
    for leg in rounds["parent"][0]:
        e = {}
        for t in ("parent", "result"):
            for f in ("wall_s", "ms_ingest", "ms_hot_path", "ms_emit"):
                e.setdefault(f, {})[t] = [r[leg][f] for r in rounds[t]]
        w = e["wall_s"]
        mp, mr, spread = statistics.median(w["parent"]), statistics.median(w["result"]), max(w["parent"]) - min(w["parent"])
        e["median_wall_s"] = {"parent": mp, "result": mr}
        e["parent_spread_s"] = round(spread, 4)
        e["pass"] = mr <= mp + spread
        e["median_stage_ms"] = {f: {t: statistics.median(e[f][t]) for t in ("parent", "result")} for f in ("ms_ingest", "ms_hot_path", "ms_emit")}
        ok = ok and e["pass"]
        out["legs"][leg] = e
        print("%-14s wall median parent %.4f result %.4f (parent spread %.4f) %s | stages %s" % (leg, mp, mr, spread, "pass" if e["pass"] else "FAIL", e["median_stage_ms"]))
    json.dump(out, open(out_path, "w"), indent=1)
    print("ALL PASS" if ok else "NOT ALL PASS")


mode = sys.argv[1]
if mode == "fixture":
    fixture(sys.argv[2], sys.argv[3])
elif mode == "digest":
    print("RESULT " + json.dumps(digest(sys.argv[2])), flush=True)
elif mode == "table":
    table(sys.argv[2], sys.argv[3])
elif mode == "time":
    print("RESULT " + json.dumps(timed(sys.argv[2])), flush=True)

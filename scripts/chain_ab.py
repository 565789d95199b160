"""Two builds of the library against each other on bench.py: the parent's tree and the result's, each a checkout with its library built.
  run OUT PARENT RESULT A B [bench.py arguments]   rounds A .. B-1: `bench.py --gpus 1 --steps 3 --warmup 1 --full` plus the given arguments, the parent then
                                                   the result, a fresh process each; bench.py's line goes to OUT/bench_{parent,result}_<round>.json
  dump OUT PARENT RESULT [bench.py arguments]      `bench.py --gpus 1 --steps 1 --warmup 1 --dump-outputs DIR` plus the given arguments (`--config 4`) once
                                                   per tree, the dumped arrays compared byte for byte: OUT/same_bytes.json (the arrays themselves are not kept)
  table OUT OUT.json                               same_bytes.json; per leg the rounds, the medians, the parent's max - min and whether the result's
                                                   median is no worse than the parent's median by more than that spread
                                                   (legs that the rounds' bench.py arguments switched off are left out)
Stops at the first process that fails or outlives its limit."""
import glob
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

# leg -> (path into bench.py's line, higher is better)
LEGS = {
    "value": (("value",), True),
    "configs[1]_adaptive": (("config", "legs", "configs[1]_adaptive", "value"), True),
    "configs[2]": (("config", "legs", "configs[2]", "value"), True),
    "configs[4] shard": (("config", "legs", "configs[4]", "value"), True),
    "e2e": (("config", "e2e", "regions_per_s"), True),
    "edit stage ms": (("config", "stage_ms", "ms_edit"), False),
    "affine stage ms": (("config", "stage_ms", "ms_affine"), False),
}


def bench(tree, args, log):
    t0 = time.time()
    with open(log, "w") as f:
        subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1"] + args, stdout=f, stdin=subprocess.DEVNULL, cwd=tree, timeout=600, check=True)
    print("%s: %.0f s" % (os.path.basename(log), time.time() - t0), flush=True)


def pick(line, path):
    for k in path:
        line = line[k]
    return float(line)


mode, out = sys.argv[1], sys.argv[2]
if mode == "table":
    same = json.load(open(os.path.join(out, "same_bytes.json")))
    rounds = {t: [json.load(open(p)) for p in sorted(glob.glob(os.path.join(out, "bench_%s_*.json" % t)))] for t in ("parent", "result")}
    res = {"what": "bench.py --gpus 1 --steps 3 --warmup 1 --full, parent and result in turn on one MI355X, a fresh process each", "same_bytes": same, "legs": {}}
    print("dumped arrays: %d, differing: %s" % (same["arrays"], same["differing"]))
    ok = same["arrays"] > 0 and not same["differing"]
    for leg, (where, higher) in LEGS.items():
        try:
            v = {t: [pick(r, where) for r in rounds[t]] for t in rounds}
        except KeyError:          # a leg the rounds were run without (--no-legs, --e2e-regions 0, --config N)
            continue
        mp, mr, spread = statistics.median(v["parent"]), statistics.median(v["result"]), max(v["parent"]) - min(v["parent"])
        good = mr >= mp - spread if higher else mr <= mp + spread
        res["legs"][leg] = dict(v, unit="regions/s" if higher else "ms", median={"parent": mp, "result": mr}, parent_spread=round(spread, 3))
        res["legs"][leg]["pass"] = good
        ok = ok and good
        print("%-20s parent %10.2f  result %10.2f  parent spread %8.2f  %s" % (leg, mp, mr, spread, "pass" if good else "FAIL"))
    json.dump(res, open(sys.argv[3], "w"), indent=1)
    print("ALL PASS" if ok else "NOT ALL PASS")
    sys.exit(0)
trees = {"parent": os.path.abspath(sys.argv[3]), "result": os.path.abspath(sys.argv[4])}
os.makedirs(out, exist_ok=True)
if mode == "dump":
    sha = {}
    for t, tree in trees.items():
        d = os.path.abspath(os.path.join(out, "dump_" + t))
        bench(tree, ["--steps", "1", "--warmup", "1", "--dump-outputs", d] + sys.argv[5:], os.path.join(out, "dump_%s.json" % t))
        sha[t] = {os.path.basename(p): hashlib.sha256(open(p, "rb").read()).hexdigest() for p in sorted(glob.glob(os.path.join(d, "*.npy")))}
        shutil.rmtree(d)
    same = {"arrays": len(sha["parent"]), "differing": sorted(n for n in set(sha["parent"]) | set(sha["result"]) if sha["parent"].get(n) != sha["result"].get(n)),
            "sha256": sha["result"]}
    json.dump(same, open(os.path.join(out, "same_bytes.json"), "w"), indent=1)
    print("dumped arrays: %d, differing: %s" % (same["arrays"], same["differing"]), flush=True)
else:
    for r in range(int(sys.argv[5]), int(sys.argv[6])):
        for t, tree in trees.items():
            bench(tree, ["--steps", "3", "--warmup", "1", "--full"] + sys.argv[7:], os.path.join(out, "bench_%s_%d.json" % (t, r)))

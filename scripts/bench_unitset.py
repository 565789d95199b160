"""Times the unit-set discovery (otg_unitset_repeats) and the locus chain behind it (otg_unitset_locus) on one device: planted loci of four
alleles (tests/unitset_cases.planted_locus at 1 % errors), N alleles in N / 4 groups, and the same alleles as one group.  Medians of
five calls after two warm-ups, HIP events.  Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import unitset_cases as Uc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alleles", type=int, default=65536)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = random.Random(1)
    pool = [Uc.planted_locus(rng, 0.01)[0] for _ in range(512)]
    groups = [pool[i % len(pool)] for i in range(a.alleles // 4)]
    alleles, first = Uc.flat(groups)
    rows = abi.pack_seqs(alleles)
    res = {"alleles": len(alleles), "bases": int(sum(len(s) for s in alleles))}
    with otter_amd.Context(0) as ctx:
        for name, gf in (("groups_of_4", first), ("one_group", [0, len(alleles)])):
            rep, vote, sel, loc = [], [], [], []
            for it in range(7):
                ctx.repeat_batch(*rows, device_tensor=True)
                sets = ctx.unitset_repeats(gf, device_tensor=True)
                ms = ctx.unitset_last_ms()
                ctx.locus_unitsets(device_tensor=True)
                if it >= 2:
                    rep.append(sum(ctx.repeat_last_ms())); vote.append(ms[0]); sel.append(ms[1]); loc.append(ctx.locus_last_ms()[0])
            res[name] = {"groups": len(gf) - 1, "units": int(sets[2].shape[0]), "repeat_ms": statistics.median(rep), "vote_ms": statistics.median(vote),
                         "select_ms": statistics.median(sel), "locus_ms": statistics.median(loc)}
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

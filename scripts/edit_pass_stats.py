"""Per-step kernel times of the edit chain from a `rocprofv3 --kernel-trace --output-format csv` run of bench.py, the first pass and the
reassignment pass apart.
  python scripts/edit_pass_stats.py TRACE.csv [OUT.json]
A launch belongs to the pass whose task generator (K_pair_tasks / K_reassign_tasks) ran last before it; a step is one K_pair_tasks launch.
Prints, and writes to OUT.json, ms per step of every myers_edit_kernel instantiation per pass and of the kernels around them."""
import csv
import json
import re
import sys
from collections import defaultdict

WATCH = ("read_masks_kernel", "K_reverse_reads", "K_reassign_apply", "K_reassign_tasks", "K_pair_tasks", "edit_route_kernel", "wfa_edit_kernel_v2")

rows = []
with open(sys.argv[1], newline="") as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
steps = sum(1 for _, _, n in rows if "K_pair_tasks" in n)
ms = defaultdict(float)
phase = "first"
for s, e, name in rows:
    if "K_pair_tasks" in name:
        phase = "first"
    elif "K_reverse_reads" in name or "K_reassign_tasks" in name:
        phase = "reassign"
    m = re.search(r"myers_edit_kernel<(\d+), (\d+), \d+>", name)
    if m:
        ms["myers<%s,%s> %s" % (m.group(1), m.group(2), phase)] += (e - s) / 1e6
        ms["myers all %s" % phase] += (e - s) / 1e6
        continue
    for w in WATCH:
        if w in name:
            key = w if w in ("read_masks_kernel", "K_reverse_reads", "K_reassign_apply", "K_reassign_tasks", "K_pair_tasks") else "%s %s" % (w, phase)
            ms[key] += (e - s) / 1e6
            break
out = {"steps": steps, "ms_per_step": {k: round(v / max(1, steps), 3) for k, v in sorted(ms.items())}}
for k, v in out["ms_per_step"].items():
    print("%-36s %9.3f" % (k, v))
print("steps: %d" % steps)
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], "w"), indent=1)

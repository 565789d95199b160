#!/usr/bin/env python3
"""tests/golden/poa_weights.json: what the REFERENCE's own PPOA (oracle/_ref/libotter_ref.so) gives for the graphs of
tests/test_poa_weights_golden.py under every (c, t) setting of tests/poa_weights_cases.py.  Inputs and outputs only: backbone, members (run-length op
string, the bases of its X and I ops, spanning flags), per setting c and t (the float32 values, written exactly), the distinct consensus strings of the graph and
per setting the index of its own.  Build container, no GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import poa_weights_cases as W  # noqa: E402
import test_poa_weights_golden as T  # noqa: E402
from helpers import build_poa_batch, poa_specs_with_weights  # noqa: E402

O.lib()
assert O.ref() is not None, "oracle/_ref/libotter_ref.so not built"
base = T.golden_specs(O)
graphs = [{"backbone": bb.decode(), "members": [list(T.pack_member(bb, s, cg)) + [bool(l), bool(r)] for s, cg, l, r in mem], "c": [], "t": [], "consensus": [], "expected": []}
          for bb, mem, c, t in base]
for setting, fn in W.SETTINGS.items():
    specs = poa_specs_with_weights(base, fn)
    cons = O.poa_consensus_batch(*build_poa_batch(specs), which="ref")
    for g, spec, out in zip(graphs, specs, cons):
        if out.decode() not in g["consensus"]:
            g["consensus"].append(out.decode())
        g["c"].append(float(spec[2])); g["t"].append(float(spec[3])); g["expected"].append(g["consensus"].index(out.decode()))


def lines(g):          # one line per key, one per member and per consensus string
    d = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    return ("{" + '"backbone":%s,\n"members":[\n%s],\n"c":%s,\n"t":%s,\n"consensus":[\n%s],\n"expected":%s}'
            % (d(g["backbone"]), ",\n".join(d(m) for m in g["members"]), d(g["c"]), d(g["t"]), ",\n".join(d(c) for c in g["consensus"]), d(g["expected"])))


path = os.path.join(ROOT, "tests", "golden", "poa_weights.json")
with open(path, "w") as f:
    f.write('{"settings":%s,\n"graphs":[\n%s]}\n' % (json.dumps(list(W.SETTINGS), separators=(",", ":")), ",\n".join(lines(g) for g in graphs)))
json.load(open(path))
print("%s: %d graphs, %d settings, %d bytes" % (path, len(graphs), len(W.SETTINGS), os.path.getsize(path)))

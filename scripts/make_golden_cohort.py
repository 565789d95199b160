#!/usr/bin/env python3
"""Golden joint VCF of the cohort path (tests/golden/cohort_small.vcf + cohort_small.json), written WITHOUT the product's device code: host
ingest -> oracle.assemble_batch per sample -> numpy regroup -> oracle.genotype_cluster_batch -> oracle VCF text
(tests/cohort_helpers.oracle_cohort).  The inputs are regenerated from a seed (bamwrite.make_cohort_fixture), so only the VCF and the
fixture's parameters are committed.

The VCF prints HSD with 6 significant digits while device and oracle hsd agree to 1e-9 relative: a value on a rounding
boundary could print differently.  That is a condition on the fixture, not a tolerance: a seed whose golden prints an hsd within 1e-7
relative of such a boundary is passed over for the next one.  The comparison in the tests stays byte for byte."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import cohort_helpers as H  # noqa: E402
from otter_amd import bamwrite  # noqa: E402

O.lib()
kw = dict(H.GOLDEN_FIXTURE)
for seed in range(kw["seed"], kw["seed"] + 50):
    kw["seed"] = seed
    fx = bamwrite.make_cohort_fixture(tempfile.mkdtemp(), **dict(kw, len_range=tuple(kw["len_range"])))
    text, printed, grp = H.oracle_cohort(O, fx)
    margin = H.hsd_boundary_margin(printed)
    if margin > 1e-7:
        break
    print("seed %d: a printed hsd lies %.3g relative from a 6-digit rounding boundary; trying the next seed" % (seed, margin))
else:
    raise SystemExit("no seed found")
n_lines = sum(1 for l in text.split(b"\n") if l and not l.startswith(b"#"))
assert n_lines >= kw["n_regions"] - 3 and len(text) < (1 << 20)
open(H.GOLDEN_VCF, "wb").write(text)
json.dump(kw, open(H.GOLDEN_PARAMS, "w"))
print("%s: %d bytes, %d VCF lines, %d alleles regrouped, seed %d, hsd boundary margin %.3g" % (H.GOLDEN_VCF, len(text), n_lines, len(grp["alleles"]), seed, margin))

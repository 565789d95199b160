"""Child process of test_gpu_poa_weights.py::test_fixtures_reach_both_kernels_and_the_redo: runs fixture sets under OTG_POA_PROFILE (read once per
process, hence a process of its own), whose first stderr line per batch says how many graphs each launch list held and how many the LDS kernel
finished.  A marker line goes in front of each batch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import otter_amd  # noqa: E402
import oracle_lib as oracle  # noqa: E402
import poa_weights_cases as W  # noqa: E402
from helpers import build_poa_batch  # noqa: E402

oracle.lib()
with otter_amd.Context(0) as ctx:
    for label in sys.argv[1:]:
        specs = W.mixed_specs(oracle) if label == "mixed" else W.specs(oracle, label, "c=n+2,t=0.3")
        batch = build_poa_batch(specs)
        exp = oracle.poa_consensus_batch(*batch)
        sys.stderr.write("== %s\n" % label)
        sys.stderr.flush()
        assert ctx.poa_consensus_batch(*batch) == exp, label

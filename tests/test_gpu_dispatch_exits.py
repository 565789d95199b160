"""The early exits of the five otg_*_files entry points: a writer that refuses its first or a later call (the text writer of each, the
warning writer of compare, the allele writer of cohort) and an input file that does not exist.  Each must return OTG_ERR_ARG with the
text of its entry point, and the same job run again in the same process must then give the bytes of an untouched run (the contexts came
back to the pool, no thread or file handle leaked into the next job).  The cases are in tests/dispatch_exits_child.py.

A dispatcher that loses a wake-up hangs rather than fails, and the suite has no per-test time limit, so every entry point runs in a
fresh child process (which initialises the device itself) under a time limit.  A child that times out is a finding to diagnose from the
code and the OTG_DISPATCH_TRACE lines, not something to run again."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "dispatch_exits_child.py")
# A hang detector only: ten times what the slowest of these children needs when every writer accepts everything (`--good-writer`).
# Measured once on an MI355X, from process start to exit (interpreter start, fixture and device initialisation included): cohort 24 s,
# assemble_fasta_out 13 s, assemble 12 s, the others 1 - 3 s.
CHILD_GOOD_WRITER_S = 25
CHILD_TIMEOUT_S = 10 * CHILD_GOOD_WRITER_S

ENTRY_POINTS = ["assemble", "assemble_fasta_out", "genotype", "genotype_table", "cohort", "compare", "vcf2mat"]


@pytest.mark.parametrize("entry_point", ENTRY_POINTS)
def test_early_exits(gpu, tmp_path, entry_point):
    gpu.trim()          # the session context's aligner workspaces: the child's dispatcher needs the room for its own contexts
    r = subprocess.run([sys.executable, CHILD, entry_point, str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, (entry_point, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("ok")

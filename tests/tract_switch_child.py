"""Child of tests/test_gpu_tract.py: the edge set and the one-wave batches with every task forced through the 64-bit tier (OTG_TRACT_WIDE=1) or
given a whole wave (OTG_TRACT_SEG64=1).  Both switches are read once per process, so the parent starts this script fresh with one of them
set.  Prints "ok <tasks>" when every record equals tests/tract_ref.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import tract_cases as Tc  # noqa: E402
import tract_ref as R  # noqa: E402


def main():
    assert (os.environ.get("OTG_TRACT_WIDE") == "1") != (os.environ.get("OTG_TRACT_SEG64") == "1")
    pairs = Tc.edge_set()
    for p in (3, 7, 13, 29):
        pairs += Tc.one_wave_batch(p)
    seqs, units, ts, tu = Tc.pack(pairs)
    arena, off, ln = abi.pack_seqs(seqs)
    with otter_amd.Context(0) as ctx:
        rec = ctx.tract_batch(arena, off, ln, units, ts, tu)
    for t, (s, u) in enumerate(pairs):
        want = R.tract_np(s, u)
        if tuple(int(x) for x in rec[t]) != want:
            print("mismatch", t, s[:80], u[:80], rec[t], want)
            return 1
    print("ok %d" % len(pairs))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Child of tests/test_gpu_locus.py: the edge set and the one-wave batches with every task forced through the 64-bit tier (OTG_LOCUS_WIDE=1) or
given a whole wave (OTG_LOCUS_SEG64=1).  Both switches are read once per process, so the parent starts this script fresh with one of them
set.  Prints "ok <tasks>" when every record and every segment equals tests/locus_ref.py and the tiers the call reports are the forced ones."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import locus_cases as Lc  # noqa: E402
import locus_ref as R  # noqa: E402
import motif_cases as Cs  # noqa: E402


def main():
    wide = os.environ.get("OTG_LOCUS_WIDE") == "1"
    assert wide != (os.environ.get("OTG_LOCUS_SEG64") == "1")
    tasks = Lc.edge_set()
    rng = np.random.default_rng(97)
    for lens in ([3], [1, 3], [3, 5], [7, 13]):
        tasks += Lc.one_wave_batch([Cs.rs(rng, p) for p in lens])
    seqs, sets, ts, tq = Lc.pack(tasks)
    arena, off, ln = abi.pack_seqs(seqs)
    with otter_amd.Context(0) as ctx:
        recs, seg_off, segs = ctx.locus_batch(arena, off, ln, sets, ts, tq)
        tiers = ctx.locus_last_tiers()
    run = sum(1 for s, _ in tasks if len(s))
    if tiers != ((0, run) if wide else (run, 0)):
        print("tiers", tiers, run)
        return 1
    for t, (s, units) in enumerate(tasks):
        want = R.locus_np(s, units)
        try:
            Lc.check(recs[t], segs[int(seg_off[t]):int(seg_off[t + 1])], want)
        except AssertionError:
            print("mismatch", t, s[:80], [u[:40] for u in units], recs[t], want)
            return 1
    print("ok %d" % len(tasks))
    return 0


if __name__ == "__main__":
    sys.exit(main())

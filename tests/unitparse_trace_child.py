"""Child of tests/test_gpu_unitparse.py: one batch parsed under the traceback budget the parent sets (OTG_UNITPARSE_TRACE_MB, read once per
process, so the parent starts this script fresh).  The batch's store is about three megabytes, so a budget of 1 cuts it into chunks.  Prints
"ok <tasks> <sha256 of the summaries, offsets and segments>"; the parent compares the digests of two budgets."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import unitparse_cases as Uc  # noqa: E402
import unitparse_ref as R  # noqa: E402


def batch():
    """three classes, 60 + 60 + 12 waves of up to 900 rows: about 3 MB of store (twenty alleles per class, each cut at many lengths)"""
    rng = np.random.default_rng(77)
    tasks = []
    for units, n in (([b"CAG", b"CCG"], 960), (Uc.HTT, 480), ([Uc.rs(rng, 70), b"GAA"], 12)):
        pool = [Uc.tracts(rng, units, 8, 60, 0.03) for _ in range(20)]
        for i in range(n):
            tasks.append((pool[i % 20][:int(rng.integers(700, 900))], units))
    return tasks


def main():
    assert os.environ.get("OTG_UNITPARSE_TRACE_MB") in ("1", "64")
    tasks = batch()
    seqs, sets, ts, tq = Uc.pack(tasks)
    arena, off, ln = abi.pack_seqs(seqs)
    with otter_amd.Context(0) as ctx:
        sums, seg_off, segs = ctx.unitparse_batch(arena, off, ln, sets, ts, tq)
    for t in range(0, len(tasks), 37):                                     # a sample against the rule; the parent compares the whole bytes
        try:
            Uc.check(sums[t], segs[int(seg_off[t]):int(seg_off[t + 1])], R.unitparse_np(*tasks[t]))
        except AssertionError:
            print("mismatch", t, tasks[t][1], sums[t])
            return 1
    print("ok %d %s" % (len(tasks), hashlib.sha256(sums.tobytes() + seg_off.tobytes() + segs.tobytes()).hexdigest()))
    return 0


if __name__ == "__main__":
    sys.exit(main())

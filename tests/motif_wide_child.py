"""Child of tests/test_gpu_motif.py: the small motif set with every allele forced onto the tier that keeps the planes in HBM.  The switch
(OTG_MOTIF_WIDE) is read once per process, so the parent starts this script fresh with it set.  Prints "ok <alleles>" when every record and
unit equals tests/motif_ref.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import motif_cases as Cs  # noqa: E402
import motif_ref as R  # noqa: E402


def main():
    assert os.environ.get("OTG_MOTIF_WIDE") == "1"
    rng = np.random.default_rng(5)
    sets = [(Cs.edge_set(), 256, 50), (Cs.edge_set()[::3], 64, 0), (Cs.random_set(n=60), 256, 50),
            ([Cs.substitute(rng, Cs.rs(rng, 700) * 12 + b"ACG", 6), b"AC", Cs.rs(rng, 9000)], 4096, 50)]      # 16 workgroups of periods per allele
    n = 0
    with otter_amd.Context(0) as ctx:
        for seqs, mp, sl in sets:
            arena, off, ln = abi.pack_seqs(seqs)
            rec, units = ctx.motif_batch(arena, off, ln, max_period=mp, slack=sl)
            for i, s in enumerate(seqs):
                if not R.same(rec[i], units[i], R.motif(s, mp, sl)):
                    print("mismatch", mp, sl, i, s[:80], rec[i], bytes(units[i])[:80], R.motif(s, mp, sl))
                    return 1
            n += len(seqs)
    print("ok %d" % n)
    return 0


if __name__ == "__main__":
    sys.exit(main())

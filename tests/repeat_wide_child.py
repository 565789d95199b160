"""Child of tests/test_gpu_repeat.py: the small repeat sets with every allele forced onto the tier that keeps the planes in HBM.  The switch
(OTG_MOTIF_WIDE) is read once per process, so the parent starts this script fresh with it set.  Prints "ok <alleles>" when every summary
and segment equals tests/repeat_ref.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import motif_cases as Cs  # noqa: E402
import repeat_cases as Rc  # noqa: E402
import repeat_ref as R  # noqa: E402


def main():
    assert os.environ.get("OTG_MOTIF_WIDE") == "1"
    rng = np.random.default_rng(5)
    sets = [(Cs.edge_set() + [t[0] for t in Rc.TABLE] + [Rc.deep_stack()], (256, 2, 12)), (Rc.word_edge_set(), (64, 2, 2)), (Rc.word_edge_set()[::2], (65, 3, 20)),
            (Cs.random_set(n=60), (256, 2, 12)),
            ([Cs.substitute(rng, Cs.rs(rng, 700) * 12 + b"ACG", 6), b"AC", Cs.rs(rng, 9000)], (4096, 2, 12))]      # 16 workgroups of periods per allele
    n = 0
    with otter_amd.Context(0) as ctx:
        for seqs, par in sets:
            arena, off, ln = abi.pack_seqs(seqs)
            sums, seg_off, segs = ctx.repeat_batch(arena, off, ln, *par)
            for i, s in enumerate(seqs):
                r = R.structure(s, *par)
                if Rc.as_tuples(sums, seg_off, segs, i) != r["segs"] or tuple(int(x) for x in sums[i]) != (r["n_segments"], r["n_repeats"], r["covered"], r["flags"]):
                    print("mismatch", par, i, s[:80], sums[i], Rc.as_tuples(sums, seg_off, segs, i)[:8], r["segs"][:8])
                    return 1
            n += len(seqs)
    print("ok %d" % n)
    return 0


if __name__ == "__main__":
    sys.exit(main())

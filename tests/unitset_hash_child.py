"""Child of tests/test_gpu_unitset.py: the discovery with the class table's hash cut to OTG_UNITSET_HASH_BITS bits, so that classes of one
length share a hash and the compare on the rotated bases has to tell them apart.  The switch is read once per process, so the parent starts
this script fresh with it set.  Prints "ok <groups>" when every record and every unit equals tests/unitset_ref.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import otter_amd  # noqa: E402
from otter_amd import abi  # noqa: E402
import unitset_cases as Uc  # noqa: E402
import unitset_ref as S  # noqa: E402


def main():
    assert 1 <= int(os.environ["OTG_UNITSET_HASH_BITS"]) <= 3
    kw = dict(min_permille=0)
    groups = [alleles for _, alleles, k in Uc.budget_cases() if k == kw] + Uc.random_groups(7, [0, 1, 2, 5, 3, 8] * 4 + [150], lower=0.2)
    alleles, first = Uc.flat(groups)
    with otter_amd.Context(0) as ctx:
        ctx.repeat_batch(*abi.pack_seqs(alleles))
        sets, units = ctx.unitset_repeats(first, **kw)
    for g, grp in enumerate(groups):
        want = S.unitset_dict(grp, **kw)
        if tuple(int(x) for x in sets[g]) != want["record"] or units[g] != want["units"]:
            print("mismatch", g, sets[g], units[g], want["record"], want["units"])
            return 1
    print("ok %d" % len(groups))
    return 0


if __name__ == "__main__":
    sys.exit(main())

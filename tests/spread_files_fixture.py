"""The file-level fixture of the spread tests: a small BAM over tandem-repeat regions with a catalogue BED (column 4 = MOTIFS=<unit>, one
region "." = no units), built with otter_amd.bamwrite alone.  Test infrastructure."""
import hashlib
import os
from otter_amd import bamwrite

N_REGIONS = 6
NO_SET_REGION = 4          # its catalogue record has no units
KW = dict(read_group="s1", offset_l=1, offset_r=1, mapq=10, threads=2)


def make(dirname):
    """-> dict(bam, bed = the catalogue, fasta, regions, units: per region the unit bytes or None)"""
    fx = bamwrite.make_tr_fixture(dirname, N_REGIONS, depth=10, len_range=(100, 300), seed=31, rate=0.01, flank=300)
    with open(fx["fasta"]) as f:
        ref = "".join(line.strip() for line in f if not line.startswith(">"))
    units = []
    for r, (c, s, e) in enumerate(fx["regions"]):
        tr = ref[s:e]
        p = next(p for p in range(1, 7) if all(tr[i] == tr[i % p] for i in range(len(tr))))
        units.append(None if r == NO_SET_REGION else tr[:p].encode())
    cat = os.path.join(dirname, "catalogue.bed")
    with open(cat, "w") as f:
        for (c, s, e), u in zip(fx["regions"], units):
            f.write("%s\t%d\t%d\t%s\n" % (c, s, e, "MOTIFS=" + u.decode() if u else "."))
    return dict(fx, bed=cat, units=units)


def digest(text):
    return hashlib.sha256(text).hexdigest()

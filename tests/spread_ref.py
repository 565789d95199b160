"""The rule of the spread operator (include/otter_gpu.h) in plain Python: per consensus allele the order statistics of the repeat length among
the reads that voted for it.  Every read and every consensus goes through locus_ref.locus_np; the statistics are stated twice, once by
counting (`quantiles_count`: the smallest value with enough members at or below it) and once as sorted() with indexing
(`quantiles_sorted`), so that the rule has two independent forms.  Test infrastructure."""
import numpy as np
from otter_amd import abi
import locus_ref

NONE = abi.SPREAD_NONE
_cache = {}


def locus_cached(s, units, scores):
    """locus_ref.locus_np, remembered per (row, set, scores): the reads of a deep allele repeat"""
    key = (bytes(s), tuple(bytes(u) for u in units), tuple(scores))
    if key not in _cache:
        _cache[key] = locus_ref.locus_np(key[0], list(key[1]), *scores)
    return _cache[key]


def rank(j, m):
    return j * (m - 1) // 4


def quantiles_sorted(values):
    v = sorted(values)
    return [v[rank(j, len(v))] for j in range(5)] if v else [0] * 5


def quantiles_count(values):
    """q[j] = the smallest x with more than rank(j, m) members <= x"""
    m = len(values)
    if m == 0:
        return [0] * 5
    out = []
    for j in range(5):
        k = rank(j, m)
        out.append(min(x for x in set(values) if sum(1 for v in values if v <= x) > k))
    return out


def values_of(rec, segs, n_units):
    """(unit_bases, per-unit sums) of a locus record with a tract"""
    per = [0] * n_units
    for u, b, e, n, ed, ph in segs:
        per[u] += n
    return rec[5], per


def spread(arena, reads, res, regions, region_set, unit_sets, scores=(2, 7, 7, 24), quantiles=quantiles_sorted):
    """arena: the batch's bytes; reads: the otg_spread_read rows the operator reported (row, label, counted); res: assemble_collect's dict
    (regions, alleles, seqs); regions: the submitted otg_region array -> (records, unit_off, unit_records, read_records) with read_records =
    per read the (locus record, segments) or None for an uncounted read"""
    arena = np.asarray(arena, dtype=np.uint8)
    seqs = np.asarray(res["seqs"], dtype=np.uint8)
    alleles = res["alleles"]
    na = len(alleles)
    rec = np.zeros(na, dtype=abi.spread_dt)
    unit_off = np.zeros(na + 1, dtype=np.uint64)
    units_out = []
    read_rec = [None] * len(reads)
    for r, g in enumerate(regions):
        s = region_set[r]
        if s is None or s == NONE or res["regions"]["status"][r] != 0:
            continue
        for i in range(int(g["first_read"]), int(g["first_read"]) + int(g["n_reads"])):
            if reads["counted"][i]:
                o, n = int(reads["seq_off"][i]), int(reads["seq_len"][i])
                read_rec[i] = locus_cached(arena[o:o + n].tobytes(), unit_sets[s], scores)
    for a in range(na):
        A = alleles[a]
        r = int(A["region"])
        s = region_set[r]
        unit_off[a + 1] = unit_off[a]
        if s is None or s == NONE:
            rec[a]["flags"] = abi.SPREAD_NO_SET
            continue
        K = len(unit_sets[s])
        unit_off[a + 1] += K
        g = regions[r]
        mine = [i for i in range(int(g["first_read"]), int(g["first_read"]) + int(g["n_reads"])) if reads["counted"][i] and reads["label"][i] == A["label"]]
        called = [read_rec[i] for i in mine if read_rec[i][0][7] == 0]
        vals = [values_of(c[0], c[1], K) for c in called]
        o, n = int(A["seq_off"]), int(A["seq_len"])
        crec, csegs = locus_cached(seqs[o:o + n].tobytes(), unit_sets[s], scores)
        flags = 0
        if crec[7] != 0:
            flags |= abi.SPREAD_REF_NONE
            ref, ref_per = 0, [0] * K
        else:
            ref, ref_per = values_of(crec, csegs, K)
        if not vals:
            flags |= abi.SPREAD_NO_CALLS
        tot = [v[0] for v in vals]
        rec[a]["n_reads"] = len(mine)
        rec[a]["n_called"] = len(vals)
        rec[a]["ref_bases"] = ref
        rec[a]["q"] = quantiles(tot)
        if not flags & abi.SPREAD_REF_NONE:
            rec[a]["n_below"] = sum(1 for v in tot if v < ref)
            rec[a]["n_above"] = sum(1 for v in tot if v > ref)
            rec[a]["sum_below"] = sum(ref - v for v in tot if v < ref)
            rec[a]["sum_above"] = sum(v - ref for v in tot if v > ref)
        rec[a]["flags"] = flags
        for k in range(K):
            u = np.zeros(1, dtype=abi.spread_unit_dt)
            u[0]["ref_bases"] = ref_per[k]
            u[0]["q"] = quantiles([v[1][k] for v in vals])
            units_out.append(u)
    units = np.concatenate(units_out) if units_out else np.zeros(0, dtype=abi.spread_unit_dt)
    return rec, unit_off, units, read_rec


def row(region, label, seq_len, units, rec, unit_recs):
    """the row otg_spread_emit writes for one allele; units: the byte strings of its set, or None"""
    head = region + b"\t%d\t%d\t" % (label, seq_len)
    tot = b"\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t" % ((int(rec["n_reads"]), int(rec["n_called"]), int(rec["ref_bases"])) + tuple(int(x) for x in rec["q"]) +
                                                                   (int(rec["n_below"]), int(rec["n_above"]), int(rec["sum_below"]), int(rec["sum_above"])))
    if not units:
        return head + b"." + tot + b".\n"
    per = b",".join(u + b":%.2f:" % (int(ur["ref_bases"]) / len(u)) + b"/".join(b"%.2f" % (int(x) / len(u)) for x in ur["q"]) for u, ur in zip(units, unit_recs))
    return head + b",".join(units) + tot + per + b"\n"

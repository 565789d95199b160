"""The rule of the unit-set discovery (include/otter_gpu.h, "Unit sets from the alleles") restated in plain Python, in two independent forms
built on the repeat structure's and the unit alignment's own references: unitset_dict keeps a dictionary of classes and ranks by repeated
selection, unitset_sort sorts the candidates and cuts the sorted list into classes.  Both return
  dict(record=(n_units, n_classes, n_ranked, flags, weight_total), units=[(unit bytes, weight, segments, length)], classes=...).
min_rotation is Booth-free on purpose (a doubled string and one pass); rotation_witness sorts every rotation."""
import itertools
import repeat_ref as R
import unitalign_ref as U

MAX_UNIT = U.MAX_UNIT                      # OTG_UNITALIGN_MAX_UNIT
TOP = 16                                   # OTG_UNITSET_TOP
MAX_CLASSES = 2048                         # OTG_UNITSET_MAX_CLASSES
MAX_UNITS = 8                              # OTG_UNITPARSE_MAX_UNITS
MAX_LANES = 64                             # OTG_UNITPARSE_MAX_LANES
NONE, OVERFLOW = 1, 2
DEFAULT = (12, 50, 100)                    # min_bases, min_permille, redundant_permille
REPEAT_DEFAULT = (256, 2, 12)              # max_period, min_copies, min_span


def params_ok(min_bases, min_permille, redundant_permille, reserved=0):
    return 1 <= min_bases <= 1 << 24 and 0 <= min_permille <= 1000 and 0 <= redundant_permille <= 1000 and reserved == 0


def primitive(u):
    """a unit is not a repetition of a shorter one"""
    p = len(u)
    return not any(p % d == 0 and u == u[:d] * (p // d) for d in range(1, p))


def candidates(alleles, repeat=REPEAT_DEFAULT):
    """step 1: (allele, begin, p, length, unit as a code tuple) of every repeat segment with p <= MAX_UNIT"""
    out = []
    for a, s in enumerate(alleles):
        s = bytes(s)
        c = R.codes(s).tolist()
        for b, p, _, ln in R.structure_cached(s, *repeat)["segs"]:
            if p == 0 or p > MAX_UNIT:
                continue
            u = tuple(c[b:b + p])
            assert max(u) < 4, "a run is exact and code 4 matches nothing"
            assert primitive(u), ("the repeat parse gave a unit that repeats a shorter one", s, b, p)
            out.append((a, b, p, ln, u))
    return out


def min_rotation(u):
    """(r, rotation): the smallest rotation of u code by code and the smallest start that gives it, by one pass over the doubled unit"""
    p = len(u)
    d = tuple(u) + tuple(u)
    best = 0
    for r in range(1, p):
        k = 0
        while k < p and d[r + k] == d[best + k]:
            k += 1
        if k < p and d[r + k] < d[best + k]:
            best = r
    return best, d[best:best + p]


def rotation_witness(u):
    """the same by sorting every rotation"""
    u = tuple(u)
    rots = sorted((u[r:] + u[:r], r) for r in range(len(u)))
    return rots[0][1], rots[0][0]


def letters(u):
    return bytes(b"ACGT"[x] for x in u)


def _redundant(rep_c, rep_d, permille):
    p = len(rep_c)
    edits = U.unitalign_np(rep_c + rep_c, rep_d)[0]
    return edits * 1000 <= permille * 2 * p


def _finish(classes, n_classes, weight_total, min_bases, min_permille, redundant_permille, ranked):
    """steps 4 to 7 on the ranked classes (dicts with weight, segments, length, rep, rot)"""
    if n_classes > MAX_CLASSES:
        return dict(record=(0, MAX_CLASSES + 1, 0, NONE | OVERFLOW, weight_total), units=[], classes=classes, ranked=[], redundant=[])
    red = []
    for c, cl in enumerate(ranked):
        red.append(any(_redundant(cl["rep"], ranked[d]["rep"], redundant_permille) for d in range(c)))
    units, lanes = [], 0
    for cl, r in zip(ranked, red):
        need = (cl["length"] + 3) // 4
        if r or len(units) >= MAX_UNITS or lanes + need > MAX_LANES:
            continue
        lanes += need
        units.append((cl["rep"], cl["weight"], cl["segments"], cl["length"]))
    flags = 0 if units else NONE
    return dict(record=(len(units), n_classes, len(ranked), flags, weight_total), units=units, classes=classes, ranked=ranked, redundant=red)


def unitset_dict(alleles, min_bases=12, min_permille=50, redundant_permille=100, repeat=REPEAT_DEFAULT, order=None):
    """the dictionary form; order (a permutation of the candidates, optional) shows that the order of processing does not matter"""
    assert params_ok(min_bases, min_permille, redundant_permille)
    cand = candidates(alleles, repeat)
    if order is not None:
        cand = [cand[i] for i in order]
    table = {}
    total = 0
    for a, b, p, ln, u in cand:
        _, rot = min_rotation(u)
        cl = table.setdefault(rot, dict(weight=0, segments=0, length=p, rot=rot, key=None, rep=None))
        cl["weight"] += ln
        cl["segments"] += 1
        total += ln
        key = (ln, -a, -b)
        if cl["key"] is None or key > cl["key"]:
            cl["key"], cl["rep"] = key, letters(u)
    classes = list(table.values())
    ranked = []
    if classes and len(classes) <= MAX_CLASSES:
        top = max(c["weight"] for c in classes)
        left = [c for c in classes if c["weight"] >= min_bases and c["weight"] * 1000 >= min_permille * top]
        while left and len(ranked) < TOP:
            best = left[0]
            for c in left[1:]:
                if (c["weight"] > best["weight"] or (c["weight"] == best["weight"] and (c["length"] < best["length"] or
                                                     (c["length"] == best["length"] and c["rot"] < best["rot"])))):
                    best = c
            left.remove(best)
            ranked.append(best)
    return _finish(classes, len(classes), total, min_bases, min_permille, redundant_permille, ranked)


def unitset_sort(alleles, min_bases=12, min_permille=50, redundant_permille=100, repeat=REPEAT_DEFAULT):
    """the sort form: the candidates sorted by their smallest rotation, cut into classes, the classes sorted by rank"""
    assert params_ok(min_bases, min_permille, redundant_permille)
    keyed = sorted((rotation_witness(u)[1], -ln, a, b, u) for a, b, _, ln, u in candidates(alleles, repeat))
    classes = []
    for rot, grp in itertools.groupby(keyed, key=lambda x: x[0]):
        grp = list(grp)                        # within a class: the longest first, then the lower allele, then the lower begin
        classes.append(dict(weight=sum(-g[1] for g in grp), segments=len(grp), length=len(rot), rot=rot, rep=letters(grp[0][4])))
    total = sum(c["weight"] for c in classes)
    ranked = []
    if classes and len(classes) <= MAX_CLASSES:
        top = max(c["weight"] for c in classes)
        ranked = sorted((c for c in classes if c["weight"] >= min_bases and c["weight"] * 1000 >= min_permille * top),
                        key=lambda c: (-c["weight"], c["length"], c["rot"]))[:TOP]
    return _finish(classes, len(classes), total, min_bases, min_permille, redundant_permille, ranked)


def class_set(res, selected=True):
    """the classes of a result as a set of smallest rotations in letters (of the selected units, or of every class seen)"""
    if selected:
        return {letters(min_rotation(U.codes(u[0]))[1]) for u in res["units"]}
    return {letters(c["rot"]) for c in res["classes"]}


def row(chrom, start, end, res, n_alleles):
    """the catalogue line of otg_unitset_emit for one region"""
    if not res["units"]:
        col = b"."
    else:
        col = (b"MOTIFS=" + b",".join(u[0] for u in res["units"]) + b";BASES=" + b",".join(b"%d" % u[1] for u in res["units"]) + b";SEGMENTS=" +
               b",".join(b"%d" % u[2] for u in res["units"]) + b";ALLELES=%d" % n_alleles)
    return chrom + b"\t%d\t%d\t" % (start, end) + col + b"\n"

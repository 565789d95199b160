"""Shared pieces of the `otter compare` tests: the C++ restatement (tests/edit_align_ref.cpp) built with g++, and allele BAMs written
with otter_amd/bamwrite.py the way `otter assemble` writes them (truth side: records named after the chromosome, with sp:A tags)."""
import os
import struct
import subprocess

import numpy as np

from otter_amd import abi, bamwrite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.path.join(ROOT, "tests", "edit_align_ref.cpp")


def build_ref(tmp):
    exe = os.path.join(str(tmp), "edit_align_ref")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, REF_SRC])
    return exe


def ref_align(exe, pairs, diamond=False):
    """[(pattern, text)] -> [(score, op string)] from the restatement."""
    inp = "".join("%s %s\n" % (p.decode() or "-", t.decode() or "-") for p, t in pairs).encode()
    r = subprocess.run([exe, "align"] + (["diamond"] if diamond else []), input=inp, capture_output=True, timeout=600, check=True)
    out = []
    for line in r.stdout.decode().splitlines():
        s, o = line.split(" ")
        out.append((int(s), b"" if o == "-" else o.encode()))
    return out


def ref_compare(exe, regions):
    """regions: [(region string, [truth seqs], [spannings], [query seqs])] -> (stdout, stderr) of compare() restated."""
    lines = []
    for name, truth, sp, query in regions:
        lines.append("R %s %d %d %d" % (name, len(truth), len(sp), len(query)))
        lines += ["T " + t.decode() for t in truth] + ["S %d" % v for v in sp] + ["Q " + q.decode() for q in query]
    r = subprocess.run([exe, "compare"], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600, check=True)
    return r.stdout, r.stderr


def pair_plan(truth, query):
    """the pairs otg_compare_emit expects for one region: [(truth seq, query seq)] truth-major, the single query allele duplicated"""
    if len(truth) != 2 or not query:
        return []
    q = query * 2 if len(query) == 1 else query
    return [(t, x) for t in truth for x in q]


def oriented(t, q):
    """get_distances' orientation (src/compare.cpp:59): pattern = the longer sequence, ties -> the query"""
    return (t, q) if len(t) > len(q) else (q, t)


def aux(tag, typ, val):
    if typ == "Z":
        return tag.encode() + b"Z" + val.encode() + b"\0"
    if typ == "A":
        return tag.encode() + b"A" + val.encode()
    if typ == "i":
        return tag.encode() + b"i" + struct.pack("<i", val)
    if typ == "c":
        return tag.encode() + b"c" + struct.pack("<b", val)
    raise ValueError(typ)


def write_allele_bam(path, chrom, ref_len, rg_ids, recs):
    """recs: [(pos0, name, seq bytes, tags bytes)]; one @RG line per id in rg_ids"""
    recs = sorted(recs, key=lambda r: r[0])
    records = [(0, p, name, 0, 60, "%dM" % len(seq) if seq else [], seq, tags) for p, name, seq, tags in recs]
    extra = "".join("@RG\tID:%s\n" % r for r in rg_ids) + "@PG\tID:otter\tOF:1,0\n"
    bamwrite.write_bam(path, [(chrom, ref_len)], records, extra_header=extra)
    return path

"""otg_bam_sink / otg_bam_merge: the product's own SAM text written as coordinate-sorted BAM + BAI, and the merge of such
BAMs.  Host code: runs without a GPU.  Records are compared byte for byte with what the REFERENCE's vendored converter makes of the same
text (sam_parse1 via ref_sam_to_bam in oracle/_ref/libotter_ref_io.so; those parts skip when it is not built); framing, index, order,
refusals and the merge are checked against the SAM specification restated here (parsers of BGZF, BAM and BAI below)."""
import ctypes as C
import gzip
import os
import struct
import zlib

import numpy as np
import pytest
import otter_amd
from otter_amd import abi, bamwrite
import oracle_lib
import cohort_helpers as H

needs_ref = pytest.mark.skipif(oracle_lib.ref_io() is None, reason="oracle/_ref/libotter_ref_io.so not built")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HD = b"@HD\tVN:1.6\tSO:coordinate\n"
BLOCK = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---------------------------------------------------------------- the formats, restated
def parse_bam(raw):
    """inflated BAM stream -> (header text, [(name, length)], [record bytes incl. the length field], offset of the first record)"""
    assert raw[:4] == b"BAM\x01"
    lt = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + lt]
    p = 8 + lt
    n = struct.unpack_from("<i", raw, p)[0]
    p += 4
    refs = []
    for _ in range(n):
        ln = struct.unpack_from("<i", raw, p)[0]
        refs.append((raw[p + 4:p + 4 + ln - 1].decode(), struct.unpack_from("<i", raw, p + 4 + ln)[0]))
        p += 8 + ln
    first, recs = p, []
    while p < len(raw):
        bl = struct.unpack_from("<i", raw, p)[0]
        recs.append(raw[p:p + 4 + bl])
        p += 4 + bl
    assert p == len(raw)
    return text, refs, recs, first


def read_bam(path):
    return parse_bam(gzip.decompress(open(path, "rb").read()))


def blocks(path):
    """[(file offset, block bytes, inflated payload)] with the framing checked: BC subfield, BSIZE, CRC32, ISIZE"""
    raw = open(path, "rb").read()
    out, p = [], 0
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", raw, p + 10)[0]
        assert xlen == 6 and raw[p + 12:p + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        blk = raw[p:p + bsize]
        assert len(blk) == bsize
        data = zlib.decompress(blk[18:-8], -15)
        crc, isize = struct.unpack_from("<II", blk, bsize - 8)
        assert crc == zlib.crc32(data) & 0xffffffff and isize == len(data) and isize <= 65536
        out.append((p, blk, data))
        p += bsize
    assert out[-1][1] == EOF_BLOCK and all(len(b[2]) > 0 for b in out[:-1])
    return out


def record_voffsets(path):
    """virtual offset of every record start, from the block walk"""
    bl = blocks(path)
    raw = b"".join(b[2] for b in bl)
    _, _, recs, first = parse_bam(raw)
    starts, u = [], 0
    for fo, _, data in bl:
        starts.append((u, fo))
        u += len(data)
    vo, u, k = [], first, 0
    for r in recs:
        while k + 1 < len(starts) and starts[k + 1][0] <= u:
            k += 1
        vo.append(starts[k][1] << 16 | (u - starts[k][0]))
        u += len(r)
    return vo, recs


def parse_bai(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"BAI\x01"
    n = struct.unpack_from("<i", raw, 4)[0]
    p, out = 8, []
    for _ in range(n):
        nb = struct.unpack_from("<i", raw, p)[0]
        p += 4
        bins = {}
        for _ in range(nb):
            b, nc = struct.unpack_from("<Ii", raw, p)
            p += 8
            bins[b] = [struct.unpack_from("<QQ", raw, p + 16 * i) for i in range(nc)]
            p += 16 * nc
        nl = struct.unpack_from("<i", raw, p)[0]
        lin = list(struct.unpack_from("<%dQ" % nl, raw, p + 4))
        p += 4 + 8 * nl
        out.append((bins, lin))
    assert p == len(raw)
    return out


def header_of(text):
    return b"".join(l + b"\n" for l in text.split(b"\n") if l.startswith(b"@"))


def record_lines(text):
    return [l for l in text.split(b"\n") if l and not l.startswith(b"@")]


def sorted_text(text):
    """the header, then the records in the order a coordinate sort gives them: (target index, position), unmapped last, ties in input order"""
    tid = {}
    for l in header_of(text).split(b"\n"):
        if l.startswith(b"@SQ"):
            tid[[x[3:] for x in l.split(b"\t") if x.startswith(b"SN:")][0]] = len(tid)

    def key(l):
        f = l.split(b"\t")
        t, pos = tid.get(f[2], -1), int(f[3])
        if pos == 0:
            t = -1
        return (t if t >= 0 else 1 << 32, pos)
    return header_of(text) + b"".join(l + b"\n" for l in sorted(record_lines(text), key=key))


def sink_bam(text, path, sort=False, threads=1, level=-1, piece=None):
    with otter_amd.BamSink(path, sort=sort, threads=threads, level=level) as s:
        if piece is None:
            s.write(text)
        else:
            for i in range(0, len(text), piece):
                s.write(text[i:i + piece])
    return s.n_records


def ref_bam(text, path):
    open(path + ".sam", "wb").write(text)
    n = oracle_lib.ref_io().ref_sam_to_bam((path + ".sam").encode(), path.encode())
    assert n >= 0, n
    return n


def expected_header(text):
    return HD + b"".join(l + b"\n" for l in header_of(text).split(b"\n") if l and not l.startswith(b"@HD"))


def same_as_converter(text, tmp, name, sort=False):
    """the sink's BAM of `text` against the converter's BAM of the sorted text: header text, reference list, record bytes"""
    a, b = os.path.join(str(tmp), name + ".bam"), os.path.join(str(tmp), name + "_ref.bam")
    st = sorted_text(text)
    n = sink_bam(text if sort else st, a, sort=sort)
    assert ref_bam(st, b) == n == len(record_lines(text))
    ta, ra, ca, _ = read_bam(a)
    tb, rb, cb, _ = read_bam(b)
    assert ta == expected_header(text) and tb == header_of(text)
    assert ra == rb and len(ra) > 0
    assert ca == cb
    return a, b, ca


# ---------------------------------------------------------------- texts
def hand_made_alleles(seed, regions, counts=(0, 1, 200, 255, 256, 300, 65535, 65536, 100000, 70000), haps=True, max_len=400):
    """allele records whose tc / ac / sc / ic take every tag width, with and without ps / hp, se values that need all six printed digits"""
    rng = np.random.default_rng(seed)
    ses = [0.0, 0.333333343, 0.123456, 123456.789, 1e-7, 3.4e-5, 0.00999999, 12.75, 0.142857149]
    rr = np.zeros(len(regions), dtype=abi.region_result_dt)
    als, seqs = [], bytearray()
    for r in range(len(regions)):
        na = int(rng.integers(1, 4))
        rr[r]["first_allele"] = len(als); rr[r]["n_alleles"] = na; rr[r]["fc"] = na; rr[r]["ic"] = int(rng.choice(counts))
        for l in range(na):
            L = int(rng.choice([0, 1, 2, 17, max_len // 3, max_len]))
            a = np.zeros(1, dtype=abi.allele_dt)[0]
            a["seq_off"] = len(seqs); a["seq_len"] = L
            a["scov"], a["acov"], a["tcov"] = (int(x) for x in rng.choice(counts, 3))
            a["se"] = np.float32(ses[int(rng.integers(0, len(ses)))]); a["ic"] = rr[r]["ic"]
            a["ps"] = int(rng.choice([-1, 0, 5, 70000, 104729999])) if haps else -1
            a["hp"] = int(rng.choice([-1, 0, 1, 2])) if haps else -1
            a["region"] = r; a["label"] = l
            als.append(a); seqs += bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), L))
    res = {"regions": rr, "alleles": np.array(als, dtype=abi.allele_dt), "seqs": np.frombuffer(bytes(seqs) + b"\0", dtype=np.uint8).copy()}
    beds, carena = abi.make_beds(regions)
    return beds, carena, res


TARGETS = [("chr1", 5_000_000), ("chrX", 3_000_000), ("HLA-DRB1*15:01:01:01", 20_000)]


def some_regions(seed, n):
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        c, ln = TARGETS[int(rng.integers(0, len(TARGETS)))]
        s = int(rng.integers(1, ln - 6000))
        out.add((c, s, s + int(rng.integers(1, 5000))))
    order = {c: i for i, (c, _) in enumerate(TARGETS)}
    return sorted(out, key=lambda r: (order[r[0]], r[1], r[2]))


def allele_text(seed=3, n=40, rg="sampleA", haps=True):
    beds, carena, res = hand_made_alleles(seed, some_regions(seed, n), haps=haps)
    return otter_amd.emit_sam_header(TARGETS, rg, 1, 0) + otter_amd.emit_alleles(beds, carena, res, rg, False)


def reads_text(seed=4, n=12):
    rng = np.random.default_rng(seed)
    regions = some_regions(seed, n)
    beds, carena = abi.make_beds(regions)
    regs = np.zeros(n, dtype=abi.region_dt)
    reads, meta, arena, names = [], [], bytearray(), bytearray()
    for r in range(n):
        k = int(rng.integers(0, 4))
        regs[r]["first_read"] = len(reads); regs[r]["n_reads"] = k
        for j in range(k):
            L = int(rng.integers(1, 300))
            rd = np.zeros(1, dtype=abi.read_dt)[0]
            rd["seq_off"] = len(arena); rd["seq_len"] = L
            rd["spanning_l"], rd["spanning_r"] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            rd["ps"] = int(rng.choice([-1, 7, 300, 70000, 104729999])); rd["hp"] = int(rng.choice([-1, 1, 2]))
            arena += bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L))
            nm = ("m64011_%d/%d/ccs" % (r, j)).encode()
            m = np.zeros(1, dtype=abi.read_meta_dt)[0]
            m["name_off"] = len(names); m["name_len"] = len(nm); m["rq"] = float(rng.choice([0.0, 0.998877, 0.999999, 1.0, 0.9]))
            names += nm
            reads.append(rd); meta.append(m)
    batch = {"regions": regs, "reads": np.array(reads, dtype=abi.read_dt), "arena": np.frombuffer(bytes(arena) + b"\0" * 64, dtype=np.uint8).copy(),
             "meta": np.array(meta, dtype=abi.read_meta_dt), "names": np.frombuffer(bytes(names) + b"\0", dtype=np.uint8).copy()}
    return otter_amd.emit_sam_header(TARGETS, "rds", 1, 0) + otter_amd.emit_reads(beds, carena, batch, "rds")


HAND = b"".join(l + b"\n" for l in [
    b"@HD\tVN:1.0\tSO:unsorted",
    b"@SQ\tSN:c1\tLN:100000",
    b"@SQ\tSN:c2\tLN:600000000",
    b"@RG\tID:x",
    b"@CO\tany text\twith tabs",
    b"plain\t0\tc1\t100\t60\t10M\t*\t0\t0\tACGTACGTAC\t*",
    b"ops\t0\tc1\t200\t7\t3S5M2I4D6M1H\t*\t0\t0\tACGTNACGTNACGTNA\t*\tNM:i:6",
    b"qual\t16\tc1\t300\t255\t8M\t=\t500\t-208\tacgtnRYK\tII5!~#AB\tXA:A:q\tXB:A:*",
    b"secondary\t256\tc1\t300\t0\t4=1X3N2P4M\tc2\t17\t0\tAAAACGGGG\t*",
    b"emptyseq\t0\tc1\t400\t0\t0M\t*\t0\t0\t\t\tta:Z:c1:400-400\ttc:i:1",
    b"nocigar\t0\tc1\t500\t30\t*\t*\t0\t0\tACGT\tIIII",
    b"noseq\t0\tc1\t600\t30\t12M\t*\t0\t0\t*\t*",
    b"ints\t0\tc2\t1\t0\t1M\t*\t0\t0\tA\t*\ta0:i:0\ta1:i:127\ta2:i:128\ta3:i:255\ta4:i:256\ta5:i:32767\ta6:i:32768\ta7:i:65535\ta8:i:65536\ta9:i:2147483647\tb0:i:2147483648\tb1:i:4294967295",
    b"negs\t0\tc2\t1\t0\t1M\t*\t0\t0\tC\t*\tn0:i:-1\tn1:i:-128\tn2:i:-129\tn3:i:-32768\tn4:i:-32769\tn5:i:-2147483648",
    b"floats\t0\tc2\t99\t0\t1M\t*\t0\t0\tG\t*\tf0:f:0\tf1:f:0.1\tf2:f:-1.5e-7\tf3:f:123456.789\tf4:f:1e39\tf5:f:0.333333343",
    b"far\t0\tc2\t536870000\t0\t900M\t*\t0\t0\t*\t*\tZZ:Z:a b:c",
    b"pos0\t0\tc1\t0\t9\t5M\t=\t0\t0\tACGTA\t*",
    b"star\t77\t*\t0\t0\t*\t*\t0\t0\tACG\t!!!",
    b"starpos\t4\t*\t1234\t0\t*\tc2\t5\t0\t*\t*",
])


def wgat_text():
    b = otter_amd.Bam(os.path.join(GOLD, "wgat_small.bam"))
    beds, carena, _ = otter_amd.parse_bed_file(os.path.join(GOLD, "wgat_small.bed"))
    text, n = otter_amd.wgat(b, (beds, carena), "asm")
    b.close()
    assert n > 100
    return text


# ---------------------------------------------------------------- 1. records equal the reference's
@needs_ref
@pytest.mark.parametrize("which", ["wgat", "alleles", "alleles_nohaps", "reads", "hand"])
def test_records_equal_the_converters(tmp_path, which):
    text = {"wgat": wgat_text, "alleles": allele_text, "alleles_nohaps": lambda: allele_text(seed=8, haps=False), "reads": reads_text,
            "hand": lambda: HAND}[which]()
    _, _, recs = same_as_converter(text, tmp_path, which, sort=(which == "wgat"))
    if which == "alleles":          # the fixture does cross the tag widths
        blob = b"".join(recs)
        for t in (b"tcC", b"tcS", b"tcI", b"PSI", b"HPC", b"sef"):
            assert t in blob, t
    if which == "hand":
        by_name = {r[36:36 + r[12]].rstrip(b"\0"): r for r in recs}
        tid, pos, _, flag = struct.unpack_from("<iiII", by_name[b"pos0"], 4)
        assert (tid, pos) == (-1, -1) and (flag >> 16) & 4
        assert struct.unpack_from("<i", by_name[b"emptyseq"], 20)[0] == 0
        tid, _, _, flag = struct.unpack_from("<iiII", by_name[b"nocigar"], 4)
        assert tid == 0 and (flag >> 16) & 4 and (flag & 0xffff) == 0


def test_hand_written_lines_without_the_converter(tmp_path):
    """the same properties from the specification alone: tag widths, unmapped rules, header"""
    p = str(tmp_path / "h.bam")
    assert sink_bam(HAND, p, sort=True) == len(record_lines(HAND))
    text, refs, recs, _ = read_bam(p)
    assert text == expected_header(HAND) and text.count(b"@HD") == 1
    assert refs == [("c1", 100000), ("c2", 600000000)]
    by_name = {r[36:36 + r[12]].rstrip(b"\0"): r for r in recs}
    assert [r[36:36 + r[12] - 1] for r in recs[-3:]] == [b"pos0", b"star", b"starpos"]          # unmapped last, in input order
    ints = by_name[b"ints"]
    for tag, typ, val in ((b"a0", "C", 0), (b"a1", "C", 127), (b"a2", "C", 128), (b"a3", "C", 255), (b"a4", "S", 256), (b"a5", "S", 32767), (b"a6", "S", 32768),
                          (b"a7", "S", 65535), (b"a8", "I", 65536), (b"a9", "I", 2147483647), (b"b0", "I", 2147483648), (b"b1", "I", 4294967295)):
        assert tag + typ.encode() + struct.pack("<" + {"C": "B", "S": "H", "I": "I"}[typ], val) in ints, tag
    negs = by_name[b"negs"]
    for tag, typ, val in ((b"n0", "c", -1), (b"n1", "c", -128), (b"n2", "s", -129), (b"n3", "s", -32768), (b"n4", "i", -32769), (b"n5", "i", -2147483648)):
        assert tag + typ.encode() + struct.pack("<" + {"c": "b", "s": "h", "i": "i"}[typ], val) in negs, tag
    assert b"f1f" + struct.pack("<f", 0.1) in by_name[b"floats"] and b"f4f" + struct.pack("<f", float("inf")) in by_name[b"floats"]
    ops = by_name[b"ops"]
    n_cigar = struct.unpack_from("<I", ops, 16)[0] & 0xffff
    cig = struct.unpack_from("<%dI" % n_cigar, ops, 36 + ops[12])
    assert [(c >> 4, "MIDNSHP=X"[c & 15]) for c in cig] == [(3, "S"), (5, "M"), (2, "I"), (4, "D"), (6, "M"), (1, "H")]
    assert struct.unpack_from("<I", ops, 12)[0] >> 16 == bamwrite.reg2bin(199, 199 + 15)
    q = by_name[b"qual"]
    assert struct.unpack_from("<iii", q, 24) == (0, 499, -208)                                    # RNEXT '=' is the record's own target
    assert q[-8 - 8:-8] == bytes(c - 33 for c in b"II5!~#AB") and q[-8:] == b"XAAqXBA*"


# ---------------------------------------------------------------- 2. framing and determinism
def test_framing_and_determinism(tmp_path):
    text = sorted_text(allele_text(seed=5, n=400))
    assert len(text) > 3 * BLOCK
    base = str(tmp_path / "t1.bam")
    sink_bam(text, base)
    bl = blocks(base)
    assert len(bl) >= 4 and all(len(b[2]) <= BLOCK for b in bl)
    want, want_bai = open(base, "rb").read(), open(base + ".bai", "rb").read()
    for tag, kw in (("t8", dict(threads=8)), ("p1", dict(piece=1)), ("p7", dict(piece=7, threads=3)), ("p64k", dict(piece=65536))):
        p = str(tmp_path / (tag + ".bam"))
        sink_bam(text, p, **kw)
        assert open(p, "rb").read() == want, tag
        assert open(p + ".bai", "rb").read() == want_bai, tag
    p = str(tmp_path / "l1.bam")
    sink_bam(text, p, level=1)
    assert open(p, "rb").read() != want and read_bam(p) == read_bam(base)                # the level changes the bytes, not the content


# ---------------------------------------------------------------- 3. block edges
def _line(name, pos, seq, extra=b""):
    return name + b"\t0\tc1\t%d\t0\t%dM\t*\t0\t0\t" % (pos, len(seq)) + seq + b"\t*" + extra + b"\n"


def _record_size(name, L):
    return 36 + len(name) + 1 + 4 + (L + 1) // 2 + L


def _line_of_size(size, pos, rng, tag):
    """a line whose BAM record (length field included) has exactly `size` bytes: the sequence takes most, the name the rest"""
    L = (size - 41 - len(tag) - 8) * 2 // 3
    name = tag + b"_" * (size - _record_size(tag, L))
    assert _record_size(name, L) == size and 0 < len(name) < 250
    return _line(name, pos, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L)))


def test_block_edges(tmp_path):
    rng = np.random.default_rng(6)
    hdr = b"@SQ\tSN:c1\tLN:10000000\n"
    lines, u = [], 0                                       # u: bytes of the record stream so far (it starts on a block boundary)

    def add(l):
        nonlocal u
        f = l.split(b"\t")
        lines.append(l)
        u += _record_size(f[0], len(f[9]))
    pos = 10
    for L in range(1, 1500, 7):                            # the sweep of allele lengths
        add(_line(b"sweep%d" % L, pos, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L))))
        pos += 3
    add(_line_of_size(BLOCK - u % BLOCK if BLOCK - u % BLOCK >= 300 else 2 * BLOCK - u % BLOCK, pos, rng, b"ends_on_last_byte"))
    assert u % BLOCK == 0
    add(_line(b"big", pos + 1, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 200_000))))
    add(_line_of_size(2 * BLOCK - 2 - u % BLOCK if BLOCK - 2 - u % BLOCK < 300 else BLOCK - 2 - u % BLOCK, pos + 2, rng, b"before_straddle"))
    assert u % BLOCK == BLOCK - 2
    add(_line(b"straddles", pos + 3, b"ACGTACGT"))
    for L in range(1, 300, 11):
        add(_line(b"tail%d" % L, pos + 4, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L))))
    text = hdr + b"".join(lines)
    p = str(tmp_path / "edges.bam")
    assert sink_bam(text, p, threads=4, piece=50_000) == len(lines)
    bl = blocks(p)
    _, _, recs, first = parse_bam(b"".join(b[2] for b in bl))
    edges, e = set(), 0
    for _, _, data in bl[:-1]:
        e += len(data)
        edges.add(e)
    assert first in edges                                  # the header was flushed: records start a block
    ended, straddled, spans, at = [], [], [], first
    for r in recs:
        if at + len(r) in edges:
            ended.append(r)
        if any(at < x < at + 4 for x in edges):
            straddled.append(r)
        spans.append(sum(1 for x in edges if at < x < at + len(r)))
        at += len(r)
    assert any(b"ends_on_last_byte" in r for r in ended)
    assert any(b"straddles" in r for r in straddled)
    assert max(spans) >= 4                                 # the 200 000-base record lies in several blocks
    # all of them read back intact
    assert len(recs) == len(lines)
    for r, l in zip(recs, lines):
        f = l.rstrip(b"\n").split(b"\t")
        lq, lseq = r[12], struct.unpack_from("<i", r, 20)[0]
        assert r[36:36 + lq - 1] == f[0] and lseq == len(f[9])
        packed = np.frombuffer(r[36 + lq + 4:36 + lq + 4 + (lseq + 1) // 2], dtype=np.uint8)
        codes = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:lseq]
        assert np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)[codes].tobytes() == f[9]
    if oracle_lib.ref_io() is not None:
        q = str(tmp_path / "edges_ref.bam")
        ref_bam(text, q)
        assert read_bam(q)[2] == recs
    # and through the product's reader: every record is found by its region
    names = [l.split(b"\t")[0] for l in lines]
    b = otter_amd.Bam(p)
    got = b.ingest([("c1", 1, 5000)], names=True)
    b.close()
    assert len(got["reads"]) == len(lines)
    assert sorted(got["names"].tobytes()) == sorted(b"".join(names))


# ---------------------------------------------------------------- 4. index
def _index_text(seed=12, n_windows=200):
    """alleles tagged with the window they belong to: overlapping it, touching its edges from inside and from outside"""
    rng = np.random.default_rng(seed)
    targets = [("tA", 400_000), ("tB", 90_000)]
    windows, recs = [], []
    for ti, (name, ln) in enumerate(targets):
        ws = [(name, 0, ln)]
        for _ in range(n_windows):
            s = int(rng.integers(1, ln - 6000))
            ws.append((name, s, s + int(rng.integers(1, 5000))))
        for (c, s, e) in ws:
            ta = b"%s:%d-%d" % (c.encode(), s, e)
            lo, hi = max(0, s - 1), e                    # the query is [s - 1, e) in 0-based coordinates
            for kind in range(int(rng.integers(2, 6))):
                L = int(rng.integers(1, 400))
                pos0 = int(rng.choice([lo - L, lo - L + 1, hi - 1, hi, rng.integers(max(0, lo - 300), hi + 300), rng.integers(lo, hi)]))
                pos0 = min(max(pos0, 0), ln - L - 1)
                recs.append((ti, pos0, L, ta))
        windows += ws
    recs.append((0, 16_000, 20_000, b"tA:16001-36000"))
    windows.append(("tA", 16001, 36000))
    recs.sort(key=lambda r: (r[0], r[1]))
    lines = []
    for i, (ti, pos0, L, ta) in enumerate(recs):
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L))
        lines.append(b"a%d\t0\t%s\t%d\t0\t%dM\t*\t0\t0\t%s\t%s\tRG:Z:s0\tta:Z:%s\ttc:i:%d\tac:i:3\tsc:i:2\tic:i:1\tse:f:0.25\n"
                     % (i, targets[ti][0].encode(), pos0 + 1, L, seq, b"!" * L, ta, i % 70000))
    text = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in targets) + b"@RG\tID:s0\n@PG\tID:otter\tOF:1,0\n" + b"".join(lines)
    return text, windows, recs, targets


def _brute_force(windows, recs, targets, lines):
    """per window the (tc, sequence) of the records that carry its tag and overlap it, in file order"""
    out = []
    for (c, s, e) in windows:
        ta = b"%s:%d-%d" % (c.encode(), s, e)
        lo, hi = max(0, s - 1), e
        hit = []
        for i, (ti, pos0, L, t) in enumerate(recs):
            if t == ta and targets[ti][0] == c and pos0 < hi and pos0 + L > lo:
                hit.append((i % 70000, lines[i].split(b"\t")[9]))
        out.append(hit)
    return out


def _alleles_of(blk, n_windows):
    out = []
    for r in range(n_windows):
        a0, a1 = int(blk["first_allele"][r]), int(blk["first_allele"][r + 1])
        out.append([(int(a["tcov"]), blk["arena"][int(a["seq_off"]):int(a["seq_off"]) + int(a["seq_len"])].tobytes()) for a in blk["alleles"][a0:a1]])
    return out


def test_index(tmp_path):
    text, windows, recs, targets = _index_text()
    p = str(tmp_path / "idx.bam")
    assert sink_bam(text, p, threads=2) == len(recs)
    vo, brecs = record_voffsets(p)
    starts = set(vo)
    bai = parse_bai(p + ".bai")
    assert len(bai) == len(targets)
    seen = 0
    for ti, (bins, lin) in enumerate(bai):
        assert all(a <= b for a, b in zip(lin, lin[1:]))                                   # the linear index never goes back
        assert all(x == 0 or x in starts for x in lin)
        for b, chunks in bins.items():
            assert chunks == sorted(chunks)
            for beg, end in chunks:
                assert beg in starts and beg < end
                seen += 1
        # every record lies inside a chunk of its own bin
        for v, r in zip(vo, brecs):
            tid, pos, x2, x3 = struct.unpack_from("<iiII", r, 4)
            if tid == ti:
                assert any(beg <= v < end for beg, end in bins[x2 >> 16]), (ti, pos)
    assert seen > 20
    # the 20 kb record that starts at 16 000 is the first record of both 16-kb windows it reaches into
    k = [i for i, r in enumerate(recs) if r[3] == b"tA:16001-36000"][0]
    lin = bai[0][1]
    assert lin[0] <= vo[k] and lin[0] != vo[k]
    later = [vo[i] for i, r in enumerate(recs) if r[0] == 0 and r[1] + r[2] > 16384]
    assert lin[1] == min(later) and lin[1] <= vo[k] and lin[2] <= vo[k]
    assert lin[2] == min(vo[i] for i, r in enumerate(recs) if r[0] == 0 and r[1] + r[2] > 32768)
    # queries: the product's reader on the sink's file against a brute-force filter of the text
    lines = record_lines(text)
    want = _brute_force(windows, recs, targets, lines)
    assert sum(1 for w in want if w) > 300 and sum(1 for w, h in zip(windows, want) if len(h) < sum(1 for r in recs if r[3] == b"%s:%d-%d" % (w[0].encode(), w[1], w[2]))) > 50
    b = otter_amd.Bam(p)
    b.sample_index()
    got = _alleles_of(b.ingest_alleles(windows, threads=2), len(windows))
    b.close()
    assert got == want
    if oracle_lib.ref_io() is not None:
        from test_genotype_io import _ref_ingest_alleles
        q = str(tmp_path / "idx_ref.bam")
        ref_bam(text, q)
        assert _alleles_of(_ref_ingest_alleles(p, None, windows), len(windows)) == want
        assert _alleles_of(_ref_ingest_alleles(q, None, windows), len(windows)) == want


# ---------------------------------------------------------------- 5. order
def test_order(tmp_path):
    text = allele_text(seed=9, n=60)
    hdr, lines = header_of(text), record_lines(text)
    by_region = {}
    for l in lines:
        by_region.setdefault(l.split(b"\t")[0].rsplit(b"_", 1)[0], []).append(l)
    keys = list(by_region)
    perm = np.random.default_rng(2).permutation(len(keys))
    shuffled = hdr + b"".join(l + b"\n" for k in perm for l in by_region[keys[int(k)]])
    assert shuffled != text
    a, b = str(tmp_path / "sorted.bam"), str(tmp_path / "shuffled.bam")
    sink_bam(sorted_text(text), a, sort=False)
    sink_bam(shuffled, b, sort=True, threads=3)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert open(a + ".bai", "rb").read() == open(b + ".bai", "rb").read()
    # two regions with the same start keep input order, either way round
    x = b"@SQ\tSN:c1\tLN:1000\n"
    r1, r2, r0 = _line(b"first", 50, b"AC"), _line(b"second", 50, b"ACGTA"), _line(b"early", 20, b"A")
    for first, second in ((r1, r2), (r2, r1)):
        p = str(tmp_path / "tie.bam")
        sink_bam(x + first + second + r0, p, sort=True)
        names = [r[36:36 + r[12] - 1] for r in read_bam(p)[2]]
        assert names == [b"early", first.split(b"\t")[0], second.split(b"\t")[0]]
    # sort = 0 on the shuffled text: refused, with the line
    first_bad = None
    last = (-1, -1)
    tid = {n.encode(): i for i, (n, _) in enumerate(TARGETS)}
    for i, l in enumerate(shuffled.split(b"\n")):
        if l and not l.startswith(b"@"):
            f = l.split(b"\t")
            k = (tid[f[2]], int(f[3]))
            if k < last:
                first_bad = i + 1
                break
            last = k
    p = str(tmp_path / "refused.bam")
    s = otter_amd.BamSink(p, sort=False)
    with pytest.raises(otter_amd.OtterGpuError) as e:
        s.write(shuffled)
    assert "line %d:" % first_bad in str(e.value) and "out of order" in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError):
        s.close()
    assert not os.path.exists(p) and not os.path.exists(p + ".bai")


# ---------------------------------------------------------------- 6. refusals and cleanup
SQ = b"@SQ\tSN:c1\tLN:600000000\n"
GOOD = b"ok\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\t*\n"
REFUSALS = [
    ("header after a record", SQ + GOOD + b"@CO\tlate\n", "line 3", "header line after the first record"),
    ("tag type B", SQ + GOOD + b"r\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\t*\tXB:B:c,1,2\n", "line 3", "type 'B'"),
    ("tag type H", SQ + b"r\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\t*\tXH:H:1AE301\n", "line 2", "type 'H'"),
    ("unknown RNAME", SQ + b"r\t0\tc9\t10\t0\t4M\t*\t0\t0\tACGT\t*\n", "line 2", "RNAME 'c9'"),
    ("SEQ / QUAL", SQ + b"r\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\tIII\n", "line 2", "QUAL 3"),
    ("SEQ / CIGAR", SQ + b"r\t0\tc1\t10\t0\t5M\t*\t0\t0\tACGT\t*\n", "line 2", "SEQ has 4"),
    ("65536 CIGAR operations", SQ + b"r\t0\tc1\t10\t0\t" + b"1M1I" * 32768 + b"\t*\t0\t0\t*\t*\n", "line 2", "65535 CIGAR operations"),
    ("end past 2^29", SQ + b"r\t0\tc1\t536870000\t0\t1000M\t*\t0\t0\t*\t*\n", "line 2", "past 2^29"),
    ("empty Z value", SQ + b"r\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\t*\tta:Z:\n", "line 2", "not XX:T:value"),
    ("ten fields", SQ + b"r\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\n", "line 2", "10 fields"),
    ("20-digit number", SQ + b"r\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\t*\ttc:i:12345678901234567890\n", "line 2", "32-bit integer"),
    ("out of order", SQ + GOOD + b"r\t0\tc1\t9\t0\t4M\t*\t0\t0\tACGT\t*\n", "line 3", "out of order"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_remove_the_files(tmp_path, case):
    _, text, line, why = case
    p = str(tmp_path / "r.bam")
    s = otter_amd.BamSink(p)
    with pytest.raises(otter_amd.OtterGpuError) as e:
        s.write(text)
    assert "(%d)" % abi.OTG_ERR_ARG in str(e.value) and line + ":" in str(e.value) and why in str(e.value), str(e.value)
    assert s.error and s.error in str(e.value)
    with pytest.raises(otter_amd.OtterGpuError):          # every later write fails
        s.write(GOOD)
    with pytest.raises(otter_amd.OtterGpuError) as e2:     # and close behaves like abort
        s.close()
    assert line + ":" in str(e2.value)
    assert not os.path.exists(p) and not os.path.exists(p + ".bai")


@needs_ref
def test_converter_refuses_an_empty_tag_value_too(tmp_path):
    """`XX:Z:` is five bytes; sam_parse1 calls a field under six an "incomplete aux field" and stops there (src/sam.c:611)"""
    text = SQ + GOOD + b"r\t0\tc1\t10\t0\t4M\t*\t0\t0\tACGT\t*\tta:Z:\n" + GOOD
    assert ref_bam(text, str(tmp_path / "z.bam")) == 1                       # the converter stops at the line it cannot parse


def test_65535_cigar_operations_are_written(tmp_path):
    p = str(tmp_path / "c.bam")
    sink_bam(SQ + b"r\t0\tc1\t10\t0\t" + b"1M1I" * 32767 + b"1M\t*\t0\t0\t*\t*\n", p)
    assert struct.unpack_from("<I", read_bam(p)[2][0], 16)[0] & 0xffff == 65535


def test_abort_and_context_manager_cleanup(tmp_path):
    p = str(tmp_path / "a.bam")
    s = otter_amd.BamSink(p)
    s.write(SQ + GOOD * 5000)
    assert os.path.exists(p)
    s.abort()
    assert not os.path.exists(p) and not os.path.exists(p + ".bai")
    with pytest.raises(ValueError):
        with otter_amd.BamSink(p) as s:
            s.write(SQ + GOOD)
            raise ValueError("the caller's own failure")
    assert not os.path.exists(p) and not os.path.exists(p + ".bai")
    with otter_amd.BamSink(p) as s:                        # a last line without its newline, and an empty job
        s.write(SQ + GOOD[:-1])
    assert s.n_records == 1 and len(read_bam(p)[2]) == 1
    with otter_amd.BamSink(p) as s:
        pass
    assert s.n_records == 0 and read_bam(p)[:3] == (HD, [], []) and parse_bai(p + ".bai") == []
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.BamSink(str(tmp_path / "no" / "such" / "dir.bam"))


# ---------------------------------------------------------------- 7. merge
def _sample_texts(n_samples=3, n_regions=12):
    regions = some_regions(21, n_regions)
    regions = [r for i, r in enumerate(regions) if i == 0 or r[:2] != regions[i - 1][:2]]       # no two regions with the same start (merge_sams)
    texts = []
    for s in range(n_samples):
        keep = [r for i, r in enumerate(regions) if (i + s) % 5 != 0]                           # every sample misses some regions
        beds, carena, res = hand_made_alleles(30 + s, keep, counts=(1, 8, 300))
        name = "s%02d" % s
        texts.append(otter_amd.emit_sam_header(TARGETS, name, 1, 0) + otter_amd.emit_alleles(beds, carena, res, name, False))
    return texts


def test_merge(tmp_path):
    texts = _sample_texts()
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("s%d.bam" % i)))
        sink_bam(t, paths[-1])
    out = str(tmp_path / "merged.bam")
    n = otter_amd.merge_bams(paths, out, threads=2)
    assert n == sum(len(record_lines(t)) for t in texts)
    one = str(tmp_path / "one.bam")
    sink_bam(sorted_text(H.merge_sams(texts)), one)          # merge_sams orders by position alone; the targets in header order here
    mt, mr, mrecs, _ = read_bam(out)
    ot, orefs, orecs, _ = read_bam(one)
    assert mrecs == orecs and mr == orefs == TARGETS
    sq = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (c.encode(), l) for c, l in TARGETS)
    assert mt == HD + sq + b"@RG\tID:s00\n@PG\tID:otter\tOF:1,0\n@RG\tID:s01\n@RG\tID:s02\n"
    # the index of the merged file answers like the one of the single sink
    vo, _ = record_voffsets(out)
    for bins, lin in parse_bai(out + ".bai"):
        assert all(beg in set(vo) for ch in bins.values() for beg, _ in ch)
    regions = sorted({tuple(l.split(b"\t")[11:13][1][5:].decode().rsplit(":", 1)) for t in texts for l in record_lines(t)})
    regions = [(c, int(se.split("-")[0]), int(se.split("-")[1])) for c, se in regions]
    a, b = otter_amd.Bam(out), otter_amd.Bam(one)
    assert a.sample_index() == b.sample_index() == (["s00", "s01", "s02"], 1, 0)
    ga, gb = a.ingest_alleles(regions), b.ingest_alleles(regions)
    n_query = sum(1 for t in texts for l in record_lines(t) if l.split(b"\t")[5] != b"0M")         # a 0M record covers no base: no query returns it
    assert ga["alleles"].tobytes() == gb["alleles"].tobytes() and len(ga["alleles"]) == n_query > 30
    # files do not depend on the threads
    out2 = str(tmp_path / "merged_t1.bam")
    otter_amd.merge_bams(paths, out2, threads=1)
    assert open(out, "rb").read() == open(out2, "rb").read() and open(out + ".bai", "rb").read() == open(out2 + ".bai", "rb").read()


def test_merge_refusals(tmp_path):
    texts = _sample_texts()
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("s%d.bam" % i)))
        sink_bam(t, paths[-1])
    out = str(tmp_path / "m.bam")

    def refused(inputs, *words):
        open(out, "wb").write(b"a merged BAM of an earlier run")               # a refusal leaves no output behind, stale ones included
        open(out + ".bai", "wb").write(b"and its index")
        with pytest.raises(otter_amd.OtterGpuError) as e:
            otter_amd.merge_bams(inputs, out)
        assert "(%d)" % abi.OTG_ERR_ARG in str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)
        assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    refused([paths[0], paths[1], paths[0]], "ID:s00", paths[0])                                 # a sample given twice
    p = str(tmp_path / "of.bam")
    sink_bam(texts[1].replace(b"OF:1,0", b"OF:2,0"), p)
    refused([paths[0], p], "OF:", p)
    p = str(tmp_path / "sq.bam")
    sink_bam(texts[2].replace(b"LN:3000000", b"LN:3000001"), p)
    refused([paths[0], p], "@SQ", p)
    p = str(tmp_path / "unsorted.bam")
    bamwrite.write_bam(p, TARGETS, [(0, 500, "a", 0, 0, "4M", b"ACGT", b""), (0, 100, "b", 0, 0, "4M", b"ACGT", b"")], extra_header="@RG\tID:zz\n")
    refused([paths[0], p], "not coordinate-sorted", p)
    raw = open(paths[1], "rb").read()
    assert raw.endswith(EOF_BLOCK)
    p = str(tmp_path / "no_eof.bam")
    open(p, "wb").write(raw[:-len(EOF_BLOCK)])                                                  # cut exactly at a block boundary
    refused([paths[0], p], "truncated", p)
    p = str(tmp_path / "cut.bam")
    open(p, "wb").write(raw[:len(raw) // 2])
    refused([paths[0], p], p)
    refused([paths[0], str(tmp_path / "missing.bam")], "missing.bam")
    # the output named among the inputs is refused before anything is touched
    keep = open(paths[1], "rb").read()
    with pytest.raises(otter_amd.OtterGpuError):
        otter_amd.merge_bams([paths[0], paths[1]], paths[1])
    assert open(paths[1], "rb").read() == keep and os.path.exists(paths[1] + ".bai")
    with pytest.raises(otter_amd.OtterGpuError) as e:                                           # a call that names no inputs touches nothing
        otter_amd.merge_bams([], out)
    assert "no inputs" in str(e.value)

"""ctypes mirror of include/otter_gpu.h (struct layouts + constants).  Pure data definitions."""
import ctypes as C
import numpy as np

OTG_OK = 0
OTG_ERR_NO_DEVICE = -1
OTG_ERR_ARG = -2
OTG_ERR_HIP = -3
OTG_ERR_CAPACITY = -4
OTG_ERR_FATAL = -5

OTG_REGION_OK = 0
OTG_REGION_SKIP_MAXCOV = 1
OTG_REGION_NO_SPANNING = 2
OTG_REGION_EMPTY = 3
OTG_REGION_HAP_CONFLICT = 4
OTG_REGION_ALIGN_CAPACITY = 5


class otg_params(C.Structure):
    _fields_ = [
        ("max_alleles", C.c_int32), ("ignore_haps", C.c_int32), ("max_cov", C.c_int32), ("flank", C.c_int32),
        ("bandwidth_length", C.c_int32), ("min_cov_fraction2_l", C.c_int32),
        ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_ext", C.c_int32), ("realign", C.c_int32),
        ("bandwidth_short", C.c_double), ("bandwidth_long", C.c_double), ("max_error", C.c_double),
        ("min_cov_fraction", C.c_double), ("min_cov_fraction2_f", C.c_double), ("min_sim", C.c_double),
        ("gt_max_error", C.c_double), ("gt_max_cosdis", C.c_double),
        ("heuristic", C.c_int32), ("heur_min_wavefront_length", C.c_int32), ("heur_max_distance_threshold", C.c_int32),
        ("heur_steps_between_cutoffs", C.c_int32),
    ]


OTG_HEURISTIC_NONE = 0
OTG_HEURISTIC_WFADAPTIVE = 1

# the metric of the genotype clustering's first matrix (otg_genotype_cluster_metric_batch)
OTG_GT_METRIC_LENGTH = 0
OTG_GT_METRIC_EDIT = 1


def gt_metric(metric):
    """"length" / "edit" -> the OTG_GT_METRIC_* number; an integer passes through (the library refuses unknown values)."""
    if isinstance(metric, str):
        try:
            return {"length": OTG_GT_METRIC_LENGTH, "edit": OTG_GT_METRIC_EDIT}[metric]
        except KeyError:
            raise ValueError("unknown genotype metric %r (length, edit)" % (metric,)) from None
    return int(metric)

# otg_affine_last_routing: routed 0..4 = a register tier, AFFINE_TIER_NONE = straight to tier A; finished 0..4, AFFINE_FIN_A / _B / _C,
# AFFINE_FIN_NOBODY = the generic kernel gave up too.  AFFINE_N_COUNTS = length of its counts_out.
AFFINE_REG_TIERS = 5
AFFINE_TIER_NONE = 5
AFFINE_FIN_A = 5
AFFINE_FIN_B = 6
AFFINE_FIN_C = 7
AFFINE_FIN_NOBODY = -2
AFFINE_N_COUNTS = 10


def default_params(**kw):
    """Reference CLI defaults (src/command_assemble.cpp:34-45, src/command_genotype.cpp:25-27)."""
    p = otg_params(max_alleles=2, ignore_haps=1, max_cov=200, flank=100, bandwidth_length=500,
                   min_cov_fraction2_l=500, mismatch=4, gap_open=6, gap_ext=2, realign=0,
                   bandwidth_short=0.01, bandwidth_long=0.015, max_error=0.01, min_cov_fraction=0.2,
                   min_cov_fraction2_f=0.1, min_sim=0.9, gt_max_error=0.025, gt_max_cosdis=0.025,
                   heuristic=OTG_HEURISTIC_NONE, heur_min_wavefront_length=10, heur_max_distance_threshold=50, heur_steps_between_cutoffs=1)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


# numpy structured dtypes with the exact C layout (align=True reproduces the C padding)
align_task_dt = np.dtype([
    ("pattern_off", "<u8"), ("text_off", "<u8"), ("pattern_len", "<u4"), ("text_len", "<u4"),
    ("pattern_begin_free", "<i4"), ("pattern_end_free", "<i4"), ("text_begin_free", "<i4"), ("text_end_free", "<i4"),
    ("endsfree", "<i4"), ("_pad", "<i4")], align=True)

read_dt = np.dtype([
    ("seq_off", "<u8"), ("seq_len", "<u4"), ("spanning_l", "u1"), ("spanning_r", "u1"), ("_pad", "<u2"),
    ("ps", "<i4"), ("hp", "<i4"), ("ccoord_first", "<i4"), ("ccoord_second", "<i4")], align=True)

region_dt = np.dtype([
    ("first_read", "<u4"), ("n_reads", "<u4"), ("flank_l_off", "<u8"), ("flank_r_off", "<u8"),
    ("flank_l_len", "<u4"), ("flank_r_len", "<u4")], align=True)

allele_dt = np.dtype([
    ("seq_off", "<u8"), ("seq_len", "<u4"), ("scov", "<i4"), ("acov", "<i4"), ("tcov", "<i4"), ("se", "<f4"),
    ("ic", "<i4"), ("ps", "<i4"), ("hp", "<i4"), ("region", "<u4"), ("label", "<i4")], align=True)

region_result_dt = np.dtype([
    ("first_allele", "<u4"), ("n_alleles", "<u4"), ("status", "<i4"), ("ic", "<i4"), ("fc", "<i4"), ("n_valid", "<i4")],
    align=True)

poa_member_dt = np.dtype([
    ("seq_off", "<u8"), ("seq_len", "<u4"), ("cigar_len", "<u4"), ("cigar_off", "<u8"),
    ("spanning_l", "u1"), ("spanning_r", "u1"), ("_pad", "u1", (6,))], align=True)

poa_graph_dt = np.dtype([
    ("backbone_off", "<u8"), ("backbone_len", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"),
    ("c", "<f4"), ("t", "<f4"), ("_pad", "<u4")], align=True)

run_stats_dt = np.dtype([
    ("n_regions", "<u8"), ("n_regions_ok", "<u8"),
    ("edit_tasks", "<u8"), ("edit_cells", "<u8"), ("edit_seq_bytes", "<u8"),
    ("affine_tasks", "<u8"), ("affine_cells", "<u8"), ("affine_seq_bytes", "<u8"),
    ("allele_bytes", "<u8"), ("algorithmic_bytes", "<u8"),
    ("ms_edit", "<f8"), ("ms_cluster", "<f8"), ("ms_reassign", "<f8"), ("ms_affine", "<f8"), ("ms_poa", "<f8"),
    ("ms_realign", "<f8"), ("ms_total", "<f8"), ("ms_edit_kernel", "<f8"), ("edit_kernel_launches", "<u8"),
    ("ms_affine_kernel", "<f8"), ("affine_kernel_launches", "<u8"), ("affine_visited_cells", "<u8")], align=True)

assert align_task_dt.itemsize == 48
assert read_dt.itemsize == 32
assert region_dt.itemsize == 32
assert allele_dt.itemsize == 48

bed_dt = np.dtype([("chr_off", "<u8"), ("chr_len", "<u4"), ("start", "<i4"), ("end", "<i4"), ("reserved", "<u4")], align=True)
assert bed_dt.itemsize == 24
read_meta_dt = np.dtype([("name_off", "<u8"), ("name_len", "<u4"), ("reserved", "<u4"), ("rq", "<f8")], align=True)
assert read_meta_dt.itemsize == 24


ingest_opts_dt = np.dtype([("offset_l", "<i4"), ("offset_r", "<i4"), ("mapq", "<i4"), ("nonprimary", "<i4"), ("omit_nonspanning", "<i4"),
                           ("threads", "<i4"), ("read_quality", "<f8")], align=True)
assert ingest_opts_dt.itemsize == 32


def make_beds(regions):
    """regions: list of (chr_str, start, end) -> (otg_bed array, chr byte arena)."""
    beds = np.zeros(len(regions), dtype=bed_dt)
    arena = bytearray()
    for i, (c, st, en) in enumerate(regions):
        cb = c.encode() if isinstance(c, str) else bytes(c)
        beds[i]["chr_off"] = len(arena); beds[i]["chr_len"] = len(cb); beds[i]["start"] = np.uint32(st & 0xffffffff).astype(np.int32); beds[i]["end"] = np.uint32(en & 0xffffffff).astype(np.int32)
        arena += cb
    return beds, np.frombuffer(bytes(arena) + b"\0", dtype=np.uint8).copy()
assert region_result_dt.itemsize == 24
assert poa_member_dt.itemsize == 32
assert poa_graph_dt.itemsize == 32


def ptr(a, ctype=C.c_void_p):
    """Pointer to a numpy array's buffer (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctype)


def make_tasks(pairs):
    """pairs: iterable of (pattern_off, pattern_len, text_off, text_len[, (pbf,pef,tbf,tef)])."""
    pairs = list(pairs)
    t = np.zeros(len(pairs), dtype=align_task_dt)
    for i, q in enumerate(pairs):
        t[i]["pattern_off"], t[i]["pattern_len"], t[i]["text_off"], t[i]["text_len"] = q[0], q[1], q[2], q[3]
        if len(q) > 4 and q[4] is not None:
            t[i]["endsfree"] = 1
            (t[i]["pattern_begin_free"], t[i]["pattern_end_free"], t[i]["text_begin_free"], t[i]["text_end_free"]) = q[4]
    return t


def pack_seqs(seqs, pad=64):
    """Concatenate byte strings into one arena; returns (arena u8 array with `pad` slack bytes, offsets, lens)."""
    offs, lens, total = [], [], 0
    for s in seqs:
        offs.append(total)
        lens.append(len(s))
        total += len(s)
    arena = np.zeros(total + pad, dtype=np.uint8)
    pos = 0
    for s in seqs:
        arena[pos:pos + len(s)] = np.frombuffer(s if isinstance(s, (bytes, bytearray)) else s.encode(), dtype=np.uint8)
        pos += len(s)
    return arena, np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint32)


class IngestOpts(C.Structure):
    _fields_ = [("offset_l", C.c_int32), ("offset_r", C.c_int32), ("mapq", C.c_int32), ("nonprimary", C.c_int32), ("omit_nonspanning", C.c_int32),
                ("threads", C.c_int32), ("read_quality", C.c_double)]


class AssembleJob(C.Structure):
    """otg_assemble_job (include/otter_gpu.h)."""
    _fields_ = [("bam_path", C.c_char_p), ("bed_path", C.c_char_p), ("fasta_path", C.c_char_p), ("read_group", C.c_char_p),
                ("is_fasta", C.c_int32), ("reads_only", C.c_int32), ("params", otg_params), ("ingest", IngestOpts),
                ("batch_regions", C.c_uint32), ("n_devices", C.c_int32), ("devices", C.POINTER(C.c_int32))]


class SpreadJob(C.Structure):
    """otg_spread_job (include/otter_gpu.h)."""
    _fields_ = [("assemble", AssembleJob), ("match", C.c_uint32), ("mismatch", C.c_uint32), ("indel", C.c_uint32), ("min_score", C.c_uint32)]


class GenotypeJob(C.Structure):
    """otg_genotype_job (include/otter_gpu.h)."""
    _fields_ = [("bam_path", C.c_char_p), ("bed_path", C.c_char_p), ("fasta_path", C.c_char_p), ("params", otg_params),
                ("threads", C.c_int32), ("device", C.c_int32), ("batch_regions", C.c_uint32), ("metric", C.c_uint32)]


class CompareJob(C.Structure):
    """otg_compare_job (include/otter_gpu.h)."""
    _fields_ = [("truth_bam_path", C.c_char_p), ("query_bam_path", C.c_char_p), ("bed_path", C.c_char_p), ("threads", C.c_int32),
                ("device", C.c_int32), ("batch_regions", C.c_uint32), ("reserved", C.c_uint32), ("warn", C.c_void_p), ("warn_user", C.c_void_p),
                ("heuristic", C.c_int32), ("heur_min_wavefront_length", C.c_int32), ("heur_max_distance_threshold", C.c_int32),
                ("heur_steps_between_cutoffs", C.c_int32)]


class CompareCounts(C.Structure):
    """otg_compare_counts (include/otter_gpu.h)."""
    _fields_ = [(k, C.c_uint64) for k in ("n_compared", "skip_many_truth", "skip_one_truth", "skip_no_truth", "skip_no_query")]


class Vcf2matJob(C.Structure):
    """otg_vcf2mat_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("k", C.c_int32), ("threads", C.c_int32), ("device", C.c_int32),
                ("batch_alleles", C.c_uint32)]


# otg_vcf_record (include/otter_gpu.h)
vcf_record_dt = np.dtype([("region_off", np.uint64), ("region_len", np.uint32), ("first_allele", np.uint32), ("n_alleles", np.uint32),
                          ("reserved", np.uint32)])
assert vcf_record_dt.itemsize == 24
KMER_MAX = 12

# otg_motif (include/otter_gpu.h) and the bounds of the motif annotation
motif_dt = np.dtype([("period", np.uint32), ("matches", np.uint32), ("compared", np.uint32), ("best_period", np.uint32), ("flags", np.uint32),
                     ("reserved", np.uint32)])
assert motif_dt.itemsize == 24
MOTIF_MAX_PERIOD = 4096
MOTIF_MAX_LEN = 1048575
MOTIF_LDS_LEN = 32768
MOTIF_TOO_LONG = 1


class MotifsJob(C.Structure):
    """otg_motifs_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("max_period", C.c_uint32), ("slack", C.c_uint32), ("threads", C.c_int32),
                ("device", C.c_int32), ("batch_alleles", C.c_uint32), ("reserved", C.c_uint32)]


# otg_repeat_seg / otg_repeat_sum (include/otter_gpu.h) and the bounds of the repeat structure
repeat_seg_dt = np.dtype([("begin", np.uint32), ("period", np.uint32), ("copies", np.uint32), ("length", np.uint32)])
repeat_sum_dt = np.dtype([("n_segments", np.uint32), ("n_repeats", np.uint32), ("covered", np.uint32), ("flags", np.uint32)])
assert repeat_seg_dt.itemsize == 16 and repeat_sum_dt.itemsize == 16
REPEAT_MAX_PERIOD = 4096
REPEAT_MAX_LEN = 1048575
REPEAT_TOO_LONG = 1
REPEAT_TEXT_LITERAL = 24


class RepeatsJob(C.Structure):
    """otg_repeats_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("max_period", C.c_uint32), ("min_copies", C.c_uint32), ("min_span", C.c_uint32),
                ("threads", C.c_int32), ("device", C.c_int32), ("batch_alleles", C.c_uint32)]


# otg_unitalign (include/otter_gpu.h) and the bounds of the unit alignment
unitalign_dt = np.dtype([("edits", np.uint32), ("unit_bases", np.uint32), ("end_phase", np.uint32), ("flags", np.uint32)])
assert unitalign_dt.itemsize == 16
UNITALIGN_MAX_UNIT = 256
UNITALIGN_MAX_LEN = 1048575
UNITALIGN_NARROW_LEN = (65535 - 2 * UNITALIGN_MAX_UNIT + 1) // 2
UNITALIGN_NO_UNIT = 1
UNITALIGN_TOO_LONG = 2
UNITALIGN_UNIT_TOO_LONG = 4
UNITALIGN_SOURCE_BED = 0
UNITALIGN_SOURCE_MOTIF = 1


# otg_unitparse_sum / otg_unitparse_seg (include/otter_gpu.h) and the bounds of the joint unit parse
unitparse_sum_dt = np.dtype([("edits", np.uint32), ("switches", np.uint32), ("unit_bases", np.uint32), ("n_segments", np.uint32), ("end_unit", np.uint32),
                             ("end_phase", np.uint32), ("flags", np.uint32), ("reserved", np.uint32)])
unitparse_seg_dt = np.dtype([("unit", np.uint32), ("begin", np.uint32), ("end", np.uint32), ("unit_bases", np.uint32), ("edits", np.uint32),
                             ("start_phase", np.uint32)])
assert unitparse_sum_dt.itemsize == 32 and unitparse_seg_dt.itemsize == 24
UNITPARSE_MAX_UNITS = 8
UNITPARSE_MAX_LANES = 64
UNITPARSE_MAX_LEN = (2097151 - 2 * UNITALIGN_MAX_UNIT + 1) // 2
UNITPARSE_TOO_LONG = 1
UNITPARSE_NO_SET = 0xffffffff


class UnitparseJob(C.Structure):
    """otg_unitparse_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("threads", C.c_int32), ("device", C.c_int32), ("batch_alleles", C.c_uint32),
                ("reserved", C.c_uint32)]


class CopiesJob(C.Structure):
    """otg_copies_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("max_period", C.c_uint32), ("slack", C.c_uint32), ("threads", C.c_int32),
                ("device", C.c_int32), ("batch_alleles", C.c_uint32), ("reserved", C.c_uint32)]


# otg_tract / otg_tract_params (include/otter_gpu.h) and the bounds of the tract mode
tract_dt = np.dtype([("score", np.uint32), ("begin", np.uint32), ("end", np.uint32), ("edits", np.uint32), ("unit_bases", np.uint32),
                     ("end_phase", np.uint32), ("start_phase", np.uint32), ("flags", np.uint32)])
assert tract_dt.itemsize == 32
TRACT_MAX_LEN = 1048575
TRACT_NO_UNIT = 1
TRACT_TOO_LONG = 2
TRACT_UNIT_TOO_LONG = 4
TRACT_NONE = 8


class TractParams(C.Structure):
    """otg_tract_params (include/otter_gpu.h)."""
    _fields_ = [("match", C.c_uint32), ("mismatch", C.c_uint32), ("indel", C.c_uint32), ("min_score", C.c_uint32)]


class TractsJob(C.Structure):
    """otg_tracts_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("max_period", C.c_uint32), ("slack", C.c_uint32), ("match", C.c_uint32),
                ("mismatch", C.c_uint32), ("indel", C.c_uint32), ("min_score", C.c_uint32), ("threads", C.c_int32), ("device", C.c_int32),
                ("batch_alleles", C.c_uint32), ("reserved", C.c_uint32)]


# otg_locus (include/otter_gpu.h) and the bounds of the locus mode
locus_dt = np.dtype([("score", np.uint32), ("begin", np.uint32), ("end", np.uint32), ("edits", np.uint32), ("switches", np.uint32), ("unit_bases", np.uint32),
                     ("n_segments", np.uint32), ("flags", np.uint32)])
assert locus_dt.itemsize == 32
LOCUS_MAX_LEN = UNITPARSE_MAX_LEN
LOCUS_TOO_LONG = 1
LOCUS_NONE = 2


class LociJob(C.Structure):
    """otg_loci_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("match", C.c_uint32), ("mismatch", C.c_uint32), ("indel", C.c_uint32),
                ("min_score", C.c_uint32), ("threads", C.c_int32), ("device", C.c_int32), ("batch_alleles", C.c_uint32), ("reserved", C.c_uint32)]


# otg_unitset / otg_unitset_unit / otg_unitset_params (include/otter_gpu.h) and the bounds of the unit-set discovery
unitset_dt = np.dtype([("n_units", np.uint32), ("n_classes", np.uint32), ("n_ranked", np.uint32), ("flags", np.uint32), ("weight_total", np.uint64)])
unitset_unit_dt = np.dtype([("weight", np.uint64), ("segments", np.uint32), ("length", np.uint32)])
assert unitset_dt.itemsize == 24 and unitset_unit_dt.itemsize == 16
UNITSET_TOP = 16
UNITSET_MAX_CLASSES = 2048
UNITSET_NONE = 1
UNITSET_OVERFLOW = 2
UNITSET_LOCUS_NO_SET = 4


class UnitsetParams(C.Structure):
    """otg_unitset_params (include/otter_gpu.h)."""
    _fields_ = [("min_bases", C.c_uint32), ("min_permille", C.c_uint32), ("redundant_permille", C.c_uint32), ("reserved", C.c_uint32)]


class UnitsJob(C.Structure):
    """otg_units_job (include/otter_gpu.h)."""
    _fields_ = [("vcf_path", C.c_char_p), ("bed_path", C.c_char_p), ("max_period", C.c_uint32), ("min_copies", C.c_uint32), ("min_span", C.c_uint32),
                ("min_bases", C.c_uint32), ("min_share", C.c_uint32), ("redundant", C.c_uint32), ("threads", C.c_int32), ("device", C.c_int32),
                ("batch_alleles", C.c_uint32), ("reserved", C.c_uint32)]


# otg_spread / otg_spread_unit / otg_spread_read (include/otter_gpu.h) and the flags of the spread operator
spread_dt = np.dtype([("n_reads", np.uint32), ("n_called", np.uint32), ("ref_bases", np.uint32), ("q", np.uint32, (5,)), ("n_below", np.uint32), ("n_above", np.uint32),
                      ("sum_below", np.uint64), ("sum_above", np.uint64), ("flags", np.uint32), ("reserved", np.uint32)])
spread_unit_dt = np.dtype([("ref_bases", np.uint32), ("q", np.uint32, (5,))])
spread_read_dt = np.dtype([("seq_off", np.uint64), ("seq_len", np.uint32), ("label", np.int32), ("counted", np.uint32), ("task", np.uint32)])
assert spread_dt.itemsize == 64 and spread_unit_dt.itemsize == 24 and spread_read_dt.itemsize == 24
SPREAD_NONE = 0xffffffff
SPREAD_NO_SET = 1
SPREAD_NO_CALLS = 2
SPREAD_REF_NONE = 4


class JobStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_regions", "n_regions_ok", "n_regions_skipped", "n_reads", "n_alleles", "input_bytes", "output_bytes")] + \
               [("n_devices", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_double) for k in ("ms_total", "ms_ingest", "ms_hot_path", "ms_emit")]


WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_uint64)
ALLELE_WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_char), C.c_uint64)


class CohortJob(C.Structure):
    """otg_cohort_job (include/otter_gpu.h)."""
    _fields_ = [("n_samples", C.c_uint32), ("batch_regions", C.c_uint32), ("bam_paths", C.POINTER(C.c_char_p)), ("sample_names", C.POINTER(C.c_char_p)),
                ("bed_path", C.c_char_p), ("fasta_path", C.c_char_p), ("params", otg_params), ("ingest", IngestOpts),
                ("n_devices", C.c_int32), ("gt_metric", C.c_int32), ("devices", C.POINTER(C.c_int32)),
                ("allele_write", C.c_void_p), ("allele_user", C.c_void_p),
                ("matrix_write", C.c_void_p), ("matrix_user", C.c_void_p), ("matrix_k", C.c_int32), ("reserved2", C.c_int32)]

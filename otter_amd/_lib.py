"""ctypes binding of libotter_gpu.so (the C-ABI of include/otter_gpu.h).  There is no CPU fallback:
if the HIP library is missing or no device is usable, every entry point raises."""
import ctypes as C
import os
import sys
import numpy as np
from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libotter_gpu.so")

EXPORTS = [
    "otg_params_default", "otg_create", "otg_destroy", "otg_trim", "otg_last_error", "otg_device_count", "otg_exp_variant", "otg_set_heuristic",
    "otg_edit_distance_batch", "otg_affine_align_batch", "otg_affine_last_routing", "otg_cluster_batch", "otg_poa_consensus_batch",
    "otg_genotype_cluster_batch", "otg_last_kernel_ms", "otg_assemble_submit", "otg_assemble_run", "otg_assemble_result_sizes",
    "otg_assemble_collect", "otg_assemble_device_results", "otg_assemble_stats", "otg_assemble_realign", "otg_assemble_collect_reads", "otg_assemble_collect_dist",
    "otg_emit_alleles", "otg_emit_sam_header",
    "otg_bam_open", "otg_bam_close", "otg_bam_n_targets", "otg_bam_target", "otg_ingest_regions",
    "otg_ingest_regions_named", "otg_emit_reads", "otg_parse_bed_file", "otg_fasta_open", "otg_fasta_close", "otg_fasta_n_seqs",
    "otg_fasta_seq", "otg_fasta_fetch", "otg_fasta_region_flanks",
    "otg_bam_sample_index", "otg_bam_sample", "otg_ingest_alleles", "otg_emit_vcf_header", "otg_emit_vcf_lines", "otg_emit_genotype_lengths", "otg_assemble_files", "otg_assemble_files_release", "otg_assemble_batch_plan", "otg_genotype_files", "otg_wgat",
    "otg_edit_align_batch", "otg_edit_align_heur_batch", "otg_edit_align_span_batch", "otg_edit_align_last_ms", "otg_edit_align_last_tiers", "otg_ingest_compare_alleles", "otg_compare_emit", "otg_compare_files",
    "otg_kmer_usage_batch", "otg_kmer_usage_device_results", "otg_kmer_usage_last_ms", "otg_vcf_open", "otg_vcf_close", "otg_vcf_read_alleles",
    "otg_vcf2mat_emit", "otg_vcf2mat_files",
    "otg_cohort_begin", "otg_cohort_stage", "otg_cohort_regroup", "otg_cohort_genotype", "otg_cohort_result_sizes", "otg_cohort_collect",
    "otg_cohort_end", "otg_cohort_files", "otg_kmer_cohort_rows", "otg_kmer_cohort_usage", "otg_kmer_cohort_device_rows",
    "otg_bam_sink_open", "otg_bam_sink_write", "otg_bam_sink_close", "otg_bam_sink_abort", "otg_bam_sink_error", "otg_bam_merge",
    "otg_comm_unique_id", "otg_comm_create", "otg_comm_destroy", "otg_gather_sizes", "otg_gather_records",
    "otg_exp_probe_mismatches", "otg_exp_probe", "otg_exp_host", "otg_exp_device", "otg_cluster_trace_batch", "otg_genotype_cluster_trace_batch",
    "otg_genotype_cluster_metric_batch", "otg_genotype_metric_last_ms", "otg_genotype_cohort_metric",
    "otg_motif_batch", "otg_motif_device_results", "otg_motif_last_ms", "otg_motif_cohort", "otg_motif_emit", "otg_motifs_files",
    "otg_repeat_batch", "otg_repeat_collect", "otg_repeat_device_results", "otg_repeat_last_ms", "otg_repeat_cohort", "otg_repeat_emit", "otg_repeats_files",
    "otg_unitalign_batch", "otg_unitalign_motifs", "otg_unitalign_cohort", "otg_unitalign_device_results", "otg_unitalign_last_ms", "otg_unitalign_emit",
    "otg_parse_bed_units", "otg_copies_files",
    "otg_unitparse_batch", "otg_unitparse_collect", "otg_unitparse_device_results", "otg_unitparse_last_ms", "otg_unitparse_cohort", "otg_unitparse_emit",
    "otg_unitparse_files",
    "otg_tract_params_default", "otg_tract_batch", "otg_tract_motifs", "otg_tract_cohort", "otg_tract_device_results", "otg_tract_last_ms", "otg_tract_emit",
    "otg_tracts_files",
    "otg_locus_batch", "otg_locus_collect", "otg_locus_device_results", "otg_locus_last_ms", "otg_locus_last_tiers", "otg_locus_cohort", "otg_locus_emit", "otg_loci_files",
    "otg_unitset_params_default", "otg_unitset_repeats", "otg_unitset_collect", "otg_unitset_device_results", "otg_unitset_last_ms", "otg_unitset_locus", "otg_unitset_emit", "otg_units_files", "otg_units_loci_files",
    "otg_assemble_spread", "otg_spread_collect", "otg_spread_collect_reads", "otg_spread_device_results", "otg_spread_last_ms", "otg_spread_emit", "otg_spread_files",
]

_lib = None


class OtterGpuError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OtterGpuError("%s is missing: build it with `python -m otter_amd.build` (hipcc, gfx950). "
                                "otter_amd has no CPU fallback." % LIB_PATH)
        # A process that also uses PyTorch must load PyTorch's HIP runtime FIRST: torch wheels bundle their own
        # libamdhip64 under the same soname, and whichever copy is mapped first serves both; with the system copy first
        # torch.cuda finds no device (and RCCL cannot start).  The library itself does not depend on torch.
        if "torch" not in sys.modules and os.environ.get("OTG_NO_TORCH_PRELOAD") is None:
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        _lib = C.CDLL(LIB_PATH)
        _lib.otg_last_error.restype = C.c_char_p
        _lib.otg_last_error.argtypes = [C.c_void_p]
        _lib.otg_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _lib.otg_destroy.argtypes = [C.c_void_p]
        _lib.otg_trim.argtypes = [C.c_void_p]
        _lib.otg_exp_probe_mismatches.restype = C.c_longlong
        _lib.otg_exp_probe_mismatches.argtypes = [C.c_void_p]
    return _lib


def exp_host(x, variant):
    """otg_exp_host: the host restatement of glibc's exp() in `variant` (1 = FMA build, 0 = non-FMA) over a float64 array; needs no device."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    rc = load().otg_exp_host(abi.ptr(x), C.c_uint64(x.size), C.c_int(int(variant)), abi.ptr(out))
    if rc != 0:
        raise OtterGpuError("otg_exp_host failed (%d): %s" % (rc, (load().otg_last_error(None) or b"").decode()))
    return out


def exp_probe():
    """otg_exp_probe: the libm probe of otg_create without a device -> dict(variant, n_args, n_differ, mismatches_fma, mismatches_nofma)."""
    v = [C.c_uint64(0) for _ in range(4)]
    variant = load().otg_exp_probe(*(C.byref(q) for q in v))
    return {"variant": int(variant), "n_args": v[0].value, "n_differ": v[1].value, "mismatches_fma": v[2].value, "mismatches_nofma": v[3].value}


class otg_cluster_trace(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dens_raw", "dens", "sums", "max_i", "max_v", "min_i", "min_v", "state", "scalars", "merge", "height", "labels_first")]


class otg_genotype_trace(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dl", "dk", "kvec", "vnorm", "height_l", "height_k")]


TRACE_GRID, TRACE_EXT = 512, 258
TRACE_STATE = ("evaluated", "n_grid", "n_max", "n_min", "do_hclust", "err", "cut_k", "recut")


class Context:
    """One otg_ctx = one GPU + one stream (single-threaded, like a reference worker thread's aligner pair,
    src/assemble.cpp:45-50)."""

    def __init__(self, device=0):
        L = load()
        h = C.c_void_p()
        rc = L.otg_create(int(device), C.byref(h))
        if rc != 0:
            raise OtterGpuError("otg_create(device=%d) failed (%d): %s" % (device, rc, (L.otg_last_error(None) or b"").decode()))
        self._h = h
        self._L = L
        self.device = int(device)
        self._cohort_regions = self._cohort_samples = 0          # of the open cohort batch (cohort_begin)

    def close(self):
        if getattr(self, "_h", None):
            self._L.otg_destroy(self._h)
            self._h = None

    def trim(self):
        """Release the aligners' scratch workspaces (otg_trim); they come back with the next call that needs them."""
        self._check(self._L.otg_trim(self._h), "otg_trim")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise OtterGpuError("%s failed (%d): %s" % (what, rc, (self._L.otg_last_error(self._h) or b"").decode()))

    @property
    def exp_variant(self):
        return self._L.otg_exp_variant(self._h)

    @property
    def exp_probe_mismatches(self):
        """on how many arguments of otg_create's probe set the chosen exp variant differed from the host libm (otg_exp_probe_mismatches)"""
        return int(self._L.otg_exp_probe_mismatches(self._h))

    def exp_device(self, x, variant):
        """otg_exp_device: the device exp() of the clustering kernel in `variant` over a float64 array"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        self._check(self._L.otg_exp_device(self._h, abi.ptr(x), C.c_uint64(x.size), C.c_int(int(variant)), abi.ptr(out)), "otg_exp_device")
        return out

    # ------------------------------------------------------------------ L1
    def set_heuristic(self, strategy=abi.OTG_HEURISTIC_NONE, min_wavefront_length=10, max_distance_threshold=50, steps_between_cutoffs=1):
        """Heuristic of the L1 aligner calls on this context: wfa::WFAligner::setHeuristicNone / setHeuristicWFadaptive."""
        self._check(self._L.otg_set_heuristic(self._h, int(strategy), int(min_wavefront_length), int(max_distance_threshold), int(steps_between_cutoffs)),
                    "otg_set_heuristic")

    def edit_distance_batch(self, arena, tasks, want_cells=False):
        n = len(tasks)
        scores = np.zeros(n, dtype=np.int32)
        cells = np.zeros(n, dtype=np.uint64)
        rc = self._L.otg_edit_distance_batch(self._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(tasks), C.c_uint32(n),
                                             abi.ptr(scores), abi.ptr(cells))
        self._check(rc, "otg_edit_distance_batch")
        return (scores, cells) if want_cells else scores

    def edit_align_batch(self, arena, tasks, want_cigars=True):
        """otg_edit_align_batch: end-to-end unit-cost alignments with op strings -> (scores, list of op strings); want_cigars=False
        asks for the column counts only -> (scores, lengths)."""
        n = len(tasks)
        scores = np.zeros(n, dtype=np.int32)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint32)
        used = C.c_uint64(0)
        if want_cigars:
            cap = int(tasks["pattern_len"].astype(np.int64).sum() + tasks["text_len"].astype(np.int64).sum()) + 64
            out = np.zeros(cap, dtype=np.uint8)
        else:
            cap, out = 0, None
        rc = self._L.otg_edit_align_batch(self._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(tasks), C.c_uint32(n), abi.ptr(scores),
                                          abi.ptr(off) if want_cigars else None, abi.ptr(ln), abi.ptr(out) if want_cigars else None,
                                          C.c_uint64(cap), C.byref(used))
        self._check(rc, "otg_edit_align_batch")
        if not want_cigars:
            return scores, ln
        return scores, [out[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(n)]

    def edit_align_heur_batch(self, arena, tasks, strategy, a=10, b=50, c=1, want_cigars=True, want_cells=False):
        """otg_edit_align_heur_batch: edit_align_batch under the heuristic named here (abi.OTG_HEURISTIC_NONE, or abi.OTG_HEURISTIC_WFADAPTIVE
        with min_wavefront_length a, max_distance_threshold b, steps_between_cutoffs c); the context's own heuristic is left alone.
        -> (scores, op strings or lengths) and, with want_cells, the score chain's cell counts as a third item."""
        return self._edit_align_named("otg_edit_align_heur_batch", arena, tasks, strategy, a, b, c, want_cigars, want_cells)

    def _edit_align_named(self, entry, arena, tasks, strategy, a, b, c, want_cigars, want_cells):
        n = len(tasks)
        scores = np.zeros(n, dtype=np.int32)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint32)
        cells = np.zeros(n, dtype=np.uint64)
        used = C.c_uint64(0)
        if want_cigars:
            cap = int(tasks["pattern_len"].astype(np.int64).sum() + tasks["text_len"].astype(np.int64).sum()) + 64
            out = np.zeros(cap, dtype=np.uint8)
        else:
            cap, out = 0, None
        rc = getattr(self._L, entry)(self._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(tasks), C.c_uint32(n),
                                     C.c_int(int(strategy)), C.c_int(int(a)), C.c_int(int(b)), C.c_int(int(c)), abi.ptr(scores),
                                     abi.ptr(off) if want_cigars else None, abi.ptr(ln), abi.ptr(out) if want_cigars else None,
                                     C.c_uint64(cap), C.byref(used), abi.ptr(cells) if want_cells else None)
        self._check(rc, entry)
        second = [out[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(n)] if want_cigars else ln
        return (scores, second, cells) if want_cells else (scores, second)

    def edit_align_span_batch(self, arena, tasks, strategy=abi.OTG_HEURISTIC_NONE, a=10, b=50, c=1, want_cigars=True, want_cells=False):
        """otg_edit_align_span_batch: edit_align_heur_batch that also takes tasks with free ends (alignEndsFree), mixed with end-to-end ones;
        their op strings carry the free end gaps.  Same arguments and results."""
        return self._edit_align_named("otg_edit_align_span_batch", arena, tasks, strategy, a, b, c, want_cigars, want_cells)

    def edit_align_last_ms(self):
        """(score chain ms, provenance pass ms) of the latest edit_align_batch / edit_align_heur_batch (HIP events)."""
        a, b = C.c_double(0), C.c_double(0)
        self._check(self._L.otg_edit_align_last_ms(self._h, C.byref(a), C.byref(b)), "otg_edit_align_last_ms")
        return a.value, b.value

    def edit_align_last_tiers(self):
        """(tasks finished by the LDS-window tier, by the global-row tier) of the latest edit alignment call (exact: given to each)."""
        f = (C.c_uint32 * 2)(0, 0)
        self._check(self._L.otg_edit_align_last_tiers(self._h, f), "otg_edit_align_last_tiers")
        return int(f[0]), int(f[1])

    def kmer_usage_batch(self, arena, seq_off, seq_len, k=3, device_tensor=False):
        """otg_kmer_usage_batch: per allele the 4^k+1 k-mer frequencies of vcf2mat, its GC fraction and Hill-Shannon diversity ->
        (usage [n, 4^k+1] float64, gc [n], hsd [n]) as numpy arrays, or with device_tensor=True as float64 torch tensors on this context's
        device that wrap the results in HBM without a copy (valid until the next kmer_usage_batch on this context)."""
        rows, ln = _rows(arena, seq_off, seq_len)
        n, bins = len(ln), 4 ** int(k) + 1
        if device_tensor:
            rc = self._L.otg_kmer_usage_batch(self._h, *rows, C.c_int32(k), None, None, None)
            self._check(rc, "otg_kmer_usage_batch")
            return self._kmer_device_results(n, k)
        usage = np.zeros((n, bins), dtype=np.float64)
        gc = np.zeros(n, dtype=np.float64)
        hsd = np.zeros(n, dtype=np.float64)
        rc = self._L.otg_kmer_usage_batch(self._h, *rows, C.c_int32(k), abi.ptr(usage), abi.ptr(gc), abi.ptr(hsd))
        self._check(rc, "otg_kmer_usage_batch")
        return usage, gc, hsd

    def _kmer_device_results(self, n, k):
        import torch
        pu, pg, ph = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.otg_kmer_usage_device_results(self._h, C.c_uint32(n), C.c_int32(k), C.byref(pu), C.byref(pg), C.byref(ph)),
                    "otg_kmer_usage_device_results")
        bins = 4 ** int(k) + 1
        return self._wrap_device(pu.value, (n, bins), "<f8"), self._wrap_device(pg.value, (n,), "<f8"), self._wrap_device(ph.value, (n,), "<f8")

    def _wrap_device(self, ptr, shape, typestr):
        """a torch tensor on this context's device over `shape` elements of `typestr` at the device address ptr, without a copy"""
        import torch
        dev = torch.device("cuda", self.device)

        class _Span:          # __cuda_array_interface__ carrier: torch.as_tensor wraps it without copying
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}

        if 0 in shape:
            return torch.zeros(shape, dtype={"<f8": torch.float64, "<i4": torch.int32, "<i8": torch.int64, "|u1": torch.uint8}[typestr], device=dev)
        return torch.as_tensor(_Span(ptr, shape), device=dev)

    def kmer_usage_last_ms(self):
        """(counting ms, epilogue ms) of the latest kmer_usage_batch (HIP events; k <= 7 counts and finishes in one kernel)."""
        return self._last_ms("otg_kmer_usage_last_ms", 2)

    def motif_batch(self, arena, seq_off, seq_len, max_period=256, slack=50, device_tensor=False):
        """otg_motif_batch: per allele the tandem-repeat period, match counts and unit (include/otter_gpu.h states the rule) ->
        (records [n] of abi.motif_dt, units [n, stride] uint8 with unit i in units[i, :records[i]["period"]], zero behind it) as numpy arrays,
        stride = max(1, min(max_period, longest allele // 2)); or with device_tensor=True as torch tensors on this context's device that wrap
        the results in HBM without a copy (records as int32 [n, 6] in the field order of abi.motif_dt, units as uint8 [n, stride]; valid
        until the next motif call on this context)."""
        rows, ln = _rows(arena, seq_off, seq_len)
        n = len(ln)
        stride = max(1, min(int(max_period), int(ln.max()) // 2 if n else 0))
        rec = np.zeros(n, dtype=abi.motif_dt)
        units = np.zeros((n, stride), dtype=np.uint8)
        rc = self._L.otg_motif_batch(self._h, *rows, C.c_uint32(max_period), C.c_uint32(slack), None if device_tensor else abi.ptr(rec),
                                     None if device_tensor else abi.ptr(units), C.c_uint32(stride))
        self._check(rc, "otg_motif_batch")
        return self._motif_device_results(n, stride) if device_tensor else (rec, units)

    def _motif_device_results(self, n, stride):
        import torch
        if n == 0:
            dev = torch.device("cuda", self.device)
            return torch.zeros((0, 6), dtype=torch.int32, device=dev), torch.zeros((0, stride), dtype=torch.uint8, device=dev)
        m, s, pr, pu = C.c_uint32(0), C.c_uint32(0), C.c_void_p(), C.c_void_p()
        self._check(self._L.otg_motif_device_results(self._h, C.byref(m), C.byref(pr), C.byref(pu), C.byref(s)), "otg_motif_device_results")
        assert (m.value, s.value) == (n, stride)
        return self._wrap_device(pr.value, (n, 6), "<i4"), self._wrap_device(pu.value, (n, stride), "|u1")

    def motif_last_ms(self):
        """(pack and match-count ms, reduce and unit ms) of the latest motif call on this context (HIP events)."""
        return self._last_ms("otg_motif_last_ms", 2)

    def repeat_batch(self, arena, seq_off, seq_len, max_period=256, min_copies=2, min_span=12, device_tensor=False):
        """otg_repeat_batch (and otg_repeat_collect): per allele its structure as exact tandem repeats and literals (include/otter_gpu.h states
        the rule) -> (sums [n] of abi.repeat_sum_dt, seg_off [n + 1] uint64, segs [total] of abi.repeat_seg_dt; the segments of allele i are
        segs[seg_off[i]:seg_off[i + 1]]) as numpy arrays; or with device_tensor=True as torch tensors on this context's device that wrap the
        results in HBM without a copy (int32 [n, 4], int64 [n + 1], int32 [total, 4]; valid until the next repeat call on this context)."""
        rows, ln = _rows(arena, seq_off, seq_len)
        return self._seg_results("repeat", len(ln), device_tensor, lambda sums, seg_off, total: self._L.otg_repeat_batch(
            self._h, *rows, C.c_uint32(max_period), C.c_uint32(min_copies), C.c_uint32(min_span), sums, seg_off, total), "otg_repeat_batch")

    def _seg_results(self, kind, n, device_tensor, call, who):
        """the results of an operator with segments ("repeat", "unitparse", "locus"): call(sums, seg_off, total) is its entry `who` on the C arguments of
        the three; -> (sums [n], seg_off [n + 1], segs [total]) as numpy arrays of its record types, or as int32 / int64 device tensors"""
        sum_dt, seg_dt = _SEG_TYPES[kind]
        sum_w, seg_w = sum_dt.itemsize // 4, seg_dt.itemsize // 4
        total = C.c_uint64(0)
        if device_tensor:
            self._check(call(None, None, C.byref(total)), who)
            if n == 0:
                import torch
                dev = torch.device("cuda", self.device)
                return (torch.zeros((0, sum_w), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                        torch.zeros((0, seg_w), dtype=torch.int32, device=dev))
            m, t, ps, po, pg = C.c_uint32(0), C.c_uint64(0), C.c_void_p(), C.c_void_p(), C.c_void_p()
            entry = "otg_%s_device_results" % kind
            self._check(getattr(self._L, entry)(self._h, C.byref(m), C.byref(ps), C.byref(po), C.byref(pg), C.byref(t)), entry)
            assert (m.value, t.value) == (n, total.value)
            return (self._wrap_device(ps.value, (n, sum_w), "<i4"), self._wrap_device(po.value, (n + 1,), "<i8"),
                    self._wrap_device(pg.value, (t.value, seg_w), "<i4"))
        sums = np.zeros(n, dtype=sum_dt)
        seg_off = np.zeros(n + 1, dtype=np.uint64)
        self._check(call(abi.ptr(sums), abi.ptr(seg_off), C.byref(total)), who)
        segs = np.zeros(total.value, dtype=seg_dt)
        if n and total.value:
            entry = "otg_%s_collect" % kind
            self._check(getattr(self._L, entry)(self._h, abi.ptr(segs), C.c_uint64(total.value)), entry)
        return sums, seg_off, segs

    def _last_ms(self, entry, n_values):
        """the n_values HIP-event times the entry reports of the latest call of its operator on this context"""
        ms = [C.c_double(0) for _ in range(n_values)]
        self._check(getattr(self._L, entry)(self._h, *[C.byref(x) for x in ms]), entry)
        return tuple(x.value for x in ms) if n_values > 1 else ms[0].value

    def repeat_last_ms(self):
        """(runs ms, select ms) of the latest repeat call on this context (HIP events)."""
        return self._last_ms("otg_repeat_last_ms", 2)

    def unitalign_batch(self, arena, seq_off, seq_len, units, task_seq, task_unit, device_tensor=False):
        """otg_unitalign_batch: allele task_seq[t] aligned to the cyclic repeat unit units[task_unit[t]] (a list of byte strings; include/otter_gpu.h
        states the rule) -> records [n_tasks] of abi.unitalign_dt as a numpy array; or with device_tensor=True an int32 [n_tasks, 4] torch tensor
        on this context's device that wraps the records in HBM without a copy (valid until the next unit alignment on this context)."""
        rows, ln = _rows(arena, seq_off, seq_len)
        uarena, uoff, ulen = _pack_units(units)
        ts = np.ascontiguousarray(task_seq, dtype=np.uint32)
        tu = np.ascontiguousarray(task_unit, dtype=np.uint32)
        if len(ts) != len(tu):
            raise ValueError("task_seq and task_unit differ in length")
        n = len(ts)
        out = np.zeros(n, dtype=abi.unitalign_dt)
        rc = self._L.otg_unitalign_batch(self._h, *rows, abi.ptr(uarena), C.c_uint64(int(ulen.sum())), abi.ptr(uoff), abi.ptr(ulen), C.c_uint32(len(ulen)), abi.ptr(ts), abi.ptr(tu), C.c_uint32(n),
                                         None if device_tensor else abi.ptr(out))
        self._check(rc, "otg_unitalign_batch")
        return self._unitalign_device_results(n) if device_tensor else out

    def unitalign_motifs(self, device_tensor=False):
        """otg_unitalign_motifs: every allele of the latest motif call on this context (motif_batch, cohort_motifs) aligned to the unit that call
        found for it, both read where they lie in HBM -> records as unitalign_batch returns them (period 0: flags UNITALIGN_NO_UNIT, a unit
        over UNITALIGN_MAX_UNIT bytes: UNITALIGN_UNIT_TOO_LONG)."""
        m = C.c_uint32(0)
        self._check(self._L.otg_motif_device_results(self._h, C.byref(m), None, None, None), "otg_unitalign_motifs")
        out = np.zeros(m.value, dtype=abi.unitalign_dt)
        self._check(self._L.otg_unitalign_motifs(self._h, None if device_tensor else abi.ptr(out)), "otg_unitalign_motifs")
        return self._unitalign_device_results(m.value) if device_tensor else out

    def _unitalign_device_results(self, n):
        if n == 0:
            import torch
            return torch.zeros((0, 4), dtype=torch.int32, device=torch.device("cuda", self.device))
        m, p = C.c_uint32(0), C.c_void_p()
        self._check(self._L.otg_unitalign_device_results(self._h, C.byref(m), C.byref(p)), "otg_unitalign_device_results")
        assert m.value == n
        return self._wrap_device(p.value, (n, 4), "<i4")

    def unitalign_last_ms(self):
        """binning and alignment ms of the latest unit alignment on this context (HIP events)."""
        return self._last_ms("otg_unitalign_last_ms", 1)

    def tract_batch(self, arena, seq_off, seq_len, units, task_seq, task_unit, match=2, mismatch=7, indel=7, min_score=24, device_tensor=False):
        """otg_tract_batch: the repeat tract of unit units[task_unit[t]] inside allele task_seq[t] (a local wraparound alignment; include/otter_gpu.h
        states the rule) and the unit alignment of exactly that tract -> records [n_tasks] of abi.tract_dt as a numpy array; or with
        device_tensor=True an int32 [n_tasks, 8] torch tensor on this context's device that wraps the records in HBM without a copy (valid until
        the next tract call on this context).  The call counts as a unit alignment on the context."""
        rows, ln = _rows(arena, seq_off, seq_len)
        uarena, uoff, ulen = _pack_units(units)
        ts = np.ascontiguousarray(task_seq, dtype=np.uint32)
        tu = np.ascontiguousarray(task_unit, dtype=np.uint32)
        if len(ts) != len(tu):
            raise ValueError("task_seq and task_unit differ in length")
        n = len(ts)
        out = np.zeros(n, dtype=abi.tract_dt)
        q = abi.TractParams(match, mismatch, indel, min_score)
        rc = self._L.otg_tract_batch(self._h, *rows, abi.ptr(uarena), C.c_uint64(int(ulen.sum())), abi.ptr(uoff), abi.ptr(ulen), C.c_uint32(len(ulen)), abi.ptr(ts), abi.ptr(tu), C.c_uint32(n),
                                     C.byref(q), None if device_tensor else abi.ptr(out))
        self._check(rc, "otg_tract_batch")
        return self._tract_device_results(n) if device_tensor else out

    def tract_motifs(self, match=2, mismatch=7, indel=7, min_score=24, device_tensor=False):
        """otg_tract_motifs: inside every allele of the latest motif call on this context (motif_batch, cohort_motifs) the tract of the unit that
        call found for it, both read where they lie in HBM -> records as tract_batch returns them (period 0: flags TRACT_NO_UNIT, a unit over
        UNITALIGN_MAX_UNIT bytes: TRACT_UNIT_TOO_LONG)."""
        m = C.c_uint32(0)
        self._check(self._L.otg_motif_device_results(self._h, C.byref(m), None, None, None), "otg_tract_motifs")
        out = np.zeros(m.value, dtype=abi.tract_dt)
        q = abi.TractParams(match, mismatch, indel, min_score)
        self._check(self._L.otg_tract_motifs(self._h, C.byref(q), None if device_tensor else abi.ptr(out)), "otg_tract_motifs")
        return self._tract_device_results(m.value) if device_tensor else out

    def _tract_device_results(self, n):
        if n == 0:
            import torch
            return torch.zeros((0, 8), dtype=torch.int32, device=torch.device("cuda", self.device))
        m, p = C.c_uint32(0), C.c_void_p()
        self._check(self._L.otg_tract_device_results(self._h, C.byref(m), C.byref(p)), "otg_tract_device_results")
        assert m.value == n
        return self._wrap_device(p.value, (n, 8), "<i4")

    def tract_last_ms(self):
        """(both passes ms, the local pass alone ms) of the latest tract call on this context (HIP events)."""
        return self._last_ms("otg_tract_last_ms", 2)

    def unitparse_batch(self, arena, seq_off, seq_len, unit_sets, task_seq, task_set, device_tensor=False):
        """otg_unitparse_batch (and otg_unitparse_collect): allele task_seq[t] parsed against the unit set unit_sets[task_set[t]] (a list of lists
        of byte strings; include/otter_gpu.h states the rule) -> (sums [n_tasks] of abi.unitparse_sum_dt, seg_off [n_tasks + 1] uint64, segs [total]
        of abi.unitparse_seg_dt; the segments of task t are segs[seg_off[t]:seg_off[t + 1]]) as numpy arrays; or with device_tensor=True as torch
        tensors on this context's device that wrap the results in HBM without a copy (int32 [n, 8], int64 [n + 1], int32 [total, 6]; valid until
        the next unit parse on this context)."""
        rows, ln = _rows(arena, seq_off, seq_len)
        sets, ts, tq = _pack_unit_sets(unit_sets, task_seq, task_set)
        return self._seg_results("unitparse", len(ts), device_tensor, lambda sums, seg_off, total: self._L.otg_unitparse_batch(
            self._h, *rows, *sets, abi.ptr(ts), abi.ptr(tq), C.c_uint32(len(ts)), sums, seg_off, total), "otg_unitparse_batch")

    def unitparse_last_ms(self):
        """(forward ms, traceback ms) of the latest unit parse on this context (HIP events)."""
        return self._last_ms("otg_unitparse_last_ms", 2)

    def locus_batch(self, arena, seq_off, seq_len, unit_sets, task_seq, task_set, match=2, mismatch=7, indel=7, min_score=24, device_tensor=False):
        """otg_locus_batch (and otg_locus_collect): the repeat of the unit set unit_sets[task_set[t]] inside allele task_seq[t] (a local wraparound
        alignment over the set; include/otter_gpu.h states the rule) and the joint parse of exactly that stretch -> (records [n_tasks] of
        abi.locus_dt, seg_off [n_tasks + 1] uint64, segs [total] of abi.unitparse_seg_dt in allele positions) as numpy arrays; or with
        device_tensor=True as torch tensors on this context's device that wrap the results in HBM without a copy (int32 [n, 8], int64 [n + 1],
        int32 [total, 6]; valid until the next locus call or unit parse on this context).  The call counts as a unit parse on the context."""
        rows, ln = _rows(arena, seq_off, seq_len)
        sets, ts, tq = _pack_unit_sets(unit_sets, task_seq, task_set)
        q = abi.TractParams(match, mismatch, indel, min_score)
        return self._seg_results("locus", len(ts), device_tensor, lambda recs, seg_off, total: self._L.otg_locus_batch(
            self._h, *rows, *sets, abi.ptr(ts), abi.ptr(tq), C.c_uint32(len(ts)), C.byref(q), recs, seg_off, total), "otg_locus_batch")

    def locus_last_ms(self):
        """(both passes ms, the local pass alone ms) of the latest locus call on this context (HIP events)."""
        return self._last_ms("otg_locus_last_ms", 2)

    def locus_last_tiers(self):
        """(tasks on the 32-bit key, tasks on the 64-bit key) of the local pass of the latest locus call on this context."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.otg_locus_last_tiers(self._h, C.byref(a), C.byref(b)), "otg_locus_last_tiers")
        return a.value, b.value

    def unitset_repeats(self, group_first, min_bases=12, min_permille=50, redundant_permille=100, device_tensor=False):
        """otg_unitset_repeats (and otg_unitset_collect): the unit set of every group of alleles of the latest repeat call on this context
        (repeat_batch, cohort_repeats); group g is alleles group_first[g] .. group_first[g + 1] (include/otter_gpu.h states the rule) ->
        (sets [n_groups] of abi.unitset_dt, units: per group the list of (unit bytes, weight, segments, length)); or with device_tensor=True
        the torch tensors (sets int32 [n_groups, 6], set_first int64 [n_groups + 1], units int32 [n_units, 4], unit_off int64 [n_units],
        unit_len int32 [n_units], unit_arena uint8 [bytes]) that wrap the results in HBM without a copy (valid until the next discovery on
        this context).  The call counts as a unit alignment on the context."""
        gf = np.ascontiguousarray(group_first, dtype=np.uint32)
        if gf.ndim != 1 or len(gf) < 1:
            raise ValueError("group_first needs n_groups + 1 entries")
        G = len(gf) - 1
        q = abi.UnitsetParams(min_bases, min_permille, redundant_permille, 0)
        sets = np.zeros(G, dtype=abi.unitset_dt)
        set_first = np.zeros(G + 1, dtype=np.uint64)
        nu, nb = C.c_uint64(0), C.c_uint64(0)
        rc = self._L.otg_unitset_repeats(self._h, abi.ptr(gf), C.c_uint32(G), C.byref(q), None if device_tensor else abi.ptr(sets),
                                         None if device_tensor else abi.ptr(set_first), C.byref(nu), C.byref(nb))
        self._check(rc, "otg_unitset_repeats")
        U, B = nu.value, nb.value
        if device_tensor:
            m, u2, b2 = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
            p = [C.c_void_p() for _ in range(6)]
            self._check(self._L.otg_unitset_device_results(self._h, C.byref(m), C.byref(p[0]), C.byref(p[1]), C.byref(u2), C.byref(p[2]), C.byref(p[3]), C.byref(p[4]),
                                                           C.byref(p[5]), C.byref(b2)), "otg_unitset_device_results")
            assert (m.value, u2.value, b2.value) == (G, U, B)
            return (self._wrap_device(p[0].value, (G, 6), "<i4"), self._wrap_device(p[1].value, (G + 1,), "<i8"), self._wrap_device(p[2].value, (U, 4), "<i4"),
                    self._wrap_device(p[3].value, (U,), "<i8"), self._wrap_device(p[4].value, (U,), "<i4"), self._wrap_device(p[5].value, (B,), "|u1"))
        rec = np.zeros(U, dtype=abi.unitset_unit_dt)
        uoff = np.zeros(U, dtype=np.uint64)
        ulen = np.zeros(U, dtype=np.uint32)
        arena = np.zeros(max(B, 1), dtype=np.uint8)
        self._check(self._L.otg_unitset_collect(self._h, abi.ptr(rec), abi.ptr(uoff), abi.ptr(ulen), C.c_uint64(U), abi.ptr(arena), C.c_uint64(B)), "otg_unitset_collect")
        raw = arena.tobytes()
        units = [[(raw[int(uoff[k]):int(uoff[k]) + int(ulen[k])], int(rec["weight"][k]), int(rec["segments"][k]), int(rec["length"][k]))
                  for k in range(int(set_first[g]), int(set_first[g + 1]))] for g in range(G)]
        return sets, units

    def unitset_last_ms(self):
        """(candidates and vote ms, pair alignments and select ms) of the latest discovery on this context (HIP events)."""
        return self._last_ms("otg_unitset_last_ms", 2)

    def locus_unitsets(self, match=2, mismatch=7, indel=7, min_score=24, device_tensor=False):
        """otg_unitset_locus: the locus mode of every allele of the latest repeat call against the unit set the latest discovery
        (unitset_repeats) gave its group, the alleles read where they lie in HBM -> (records, seg_off, segs) as locus_batch returns them, one
        record per allele; an allele whose group has no set has a zero record with flags = abi.UNITSET_LOCUS_NO_SET and no segments."""
        m = C.c_uint32(0)
        if self._L.otg_repeat_device_results(self._h, C.byref(m), None, None, None, None) != 0:
            m.value = 0                                                     # (no repeat results: the entry below says what is missing)
        q = abi.TractParams(match, mismatch, indel, min_score)
        return self._seg_results("locus", m.value, device_tensor, lambda recs, seg_off, total: self._L.otg_unitset_locus(
            self._h, C.byref(q), recs, seg_off, total), "otg_unitset_locus")

    def affine_align_batch(self, arena, tasks, x=4, o=6, e=2, want_cells=False):
        n = len(tasks)
        scores = np.zeros(n, dtype=np.int32)
        off = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint32)
        cap = int(tasks["pattern_len"].astype(np.int64).sum() + tasks["text_len"].astype(np.int64).sum()) + 64
        out = np.zeros(cap, dtype=np.uint8)
        used = C.c_uint64(0)
        cells = np.zeros(n, dtype=np.uint64)
        rc = self._L.otg_affine_align_batch(self._h, abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(tasks), C.c_uint32(n),
                                            int(x), int(o), int(e), abi.ptr(scores), abi.ptr(off), abi.ptr(ln), abi.ptr(out),
                                            C.c_uint64(cap), C.byref(used), abi.ptr(cells))
        self._check(rc, "otg_affine_align_batch")
        cigs = [out[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(n)]
        return (scores, cigs, cells) if want_cells else (scores, cigs)

    def affine_last_routing(self, n_tasks):
        """otg_affine_last_routing for the affine_align_batch just made on this context (same n_tasks): which tier the counting sort gave
        each alignment and which tier finished it.  Returns a dict: `bound`, `routed`, `finished` (one entry per task; abi.AFFINE_*),
        `mask` (the register tiers that ran), `seg` (the sort's 7 segment bounds), and the chain's lists cut to their lengths: `sorted`,
        `tier_a_input`, `tier_a_gave_up`, `tier_b_gave_up`."""
        n = int(n_tasks)
        bound = np.zeros(n, dtype=np.int32)
        routed = np.zeros(n, dtype=np.int8)
        finished = np.zeros(n, dtype=np.int8)
        counts = np.zeros(abi.AFFINE_N_COUNTS, dtype=np.uint32)
        lists = np.zeros((4, max(n, 1)), dtype=np.uint32)
        mask = self._L.otg_affine_last_routing(self._h, C.c_uint32(n), abi.ptr(bound), abi.ptr(routed), abi.ptr(finished), abi.ptr(counts), abi.ptr(lists))
        if mask < 0:
            self._check(mask, "otg_affine_last_routing")
        return {"bound": bound, "routed": routed, "finished": finished, "mask": int(mask), "seg": counts[:7].astype(np.int64),
                "tier_a_gave_up": lists[0, :int(counts[8])].copy(), "tier_b_gave_up": lists[1, :int(counts[9])].copy(),
                "sorted": lists[2, :int(counts[6])].copy(), "tier_a_input": lists[3, :int(counts[7])].copy()}

    # ------------------------------------------------------------------ L2
    def cluster_batch(self, params, dist, dist_off, read_len, len_off, n_valid):
        nreg = len(n_valid)
        labels = np.full(int(read_len.size), -1, dtype=np.int32)
        ic = np.zeros(nreg, dtype=np.int32)
        fc = np.zeros(nreg, dtype=np.int32)
        bounds = np.full(3 * nreg, np.nan)
        rc = self._L.otg_cluster_batch(self._h, C.byref(params), abi.ptr(dist), abi.ptr(dist_off), abi.ptr(read_len), abi.ptr(len_off),
                                       abi.ptr(n_valid), C.c_uint32(nreg), abi.ptr(labels), abi.ptr(ic), abi.ptr(fc), abi.ptr(bounds))
        self._check(rc, "otg_cluster_batch")
        return labels, ic, fc, bounds.reshape(-1, 3)

    def cluster_trace_batch(self, params, dist, dist_off, read_len, len_off, n_valid, exp_variant=-1):
        """otg_cluster_trace_batch: cluster_batch plus the kernel's intermediates -> (labels, ic, fc, bounds, trace); trace is a dict of
        arrays with one row per region (dens_raw / dens / sums [TRACE_GRID], max_i / max_v / min_i / min_v [TRACE_EXT], state [8, see
        TRACE_STATE], scalars [bandwidth, dist_final]) and merge / height / labels_first indexed through len_off.  Bytes the kernel did
        not write are 0xff."""
        nreg = len(n_valid)
        nlen = int(read_len.size)
        labels = np.full(nlen, -1, dtype=np.int32)
        ic = np.zeros(nreg, dtype=np.int32)
        fc = np.zeros(nreg, dtype=np.int32)
        bounds = np.full(3 * nreg, np.nan)
        tr = {"dens_raw": np.zeros((nreg, TRACE_GRID)), "dens": np.zeros((nreg, TRACE_GRID)), "sums": np.zeros((nreg, TRACE_GRID)),
              "max_i": np.zeros((nreg, TRACE_EXT), dtype=np.int32), "max_v": np.zeros((nreg, TRACE_EXT)),
              "min_i": np.zeros((nreg, TRACE_EXT), dtype=np.int32), "min_v": np.zeros((nreg, TRACE_EXT)),
              "state": np.zeros((nreg, 8), dtype=np.int32), "scalars": np.zeros((nreg, 2)),
              "merge": np.zeros(2 * nlen + 2, dtype=np.int32), "height": np.zeros(nlen + 1), "labels_first": np.zeros(nlen + 1, dtype=np.int32)}
        t = otg_cluster_trace(*(tr[n].ctypes.data for n, _ in otg_cluster_trace._fields_))
        rc = self._L.otg_cluster_trace_batch(self._h, C.byref(params), abi.ptr(dist), abi.ptr(dist_off), abi.ptr(read_len), abi.ptr(len_off),
                                             abi.ptr(n_valid), C.c_uint32(nreg), abi.ptr(labels), abi.ptr(ic), abi.ptr(fc), abi.ptr(bounds),
                                             C.c_int(int(exp_variant)), C.byref(t))
        self._check(rc, "otg_cluster_trace_batch")
        return labels, ic, fc, bounds.reshape(-1, 3), tr

    def poa_consensus_batch(self, seq_arena, cig_arena, members, graphs):
        ng = len(graphs)
        off = np.zeros(ng, dtype=np.uint64)
        ln = np.zeros(ng, dtype=np.uint32)
        cap = int(seq_arena.size) * 2 + 1024
        out = np.zeros(cap, dtype=np.uint8)
        used = C.c_uint64(0)
        rc = self._L.otg_poa_consensus_batch(self._h, abi.ptr(seq_arena), C.c_uint64(seq_arena.size), abi.ptr(cig_arena),
                                             C.c_uint64(cig_arena.size), abi.ptr(members), C.c_uint32(len(members)),
                                             abi.ptr(graphs), C.c_uint32(ng), abi.ptr(off), abi.ptr(ln), abi.ptr(out),
                                             C.c_uint64(cap), C.byref(used))
        self._check(rc, "otg_poa_consensus_batch")
        return [out[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(ng)]

    def genotype_cluster_batch(self, params, arena, seq_off, seq_len, first_allele, n_alleles, metric="length"):
        """otg_genotype_cluster_batch -> (gt, gt_l, gt_k, hsd, n_gt, reps); metric="edit": the same tuple from
        otg_genotype_cluster_metric_batch (the first matrix from exact alignments of the alleles)."""
        if abi.gt_metric(metric) != abi.OTG_GT_METRIC_LENGTH:
            return self.genotype_cluster_metric_batch(params, arena, seq_off, seq_len, first_allele, n_alleles, metric)[:6]
        nreg = len(n_alleles)
        na = len(seq_off)
        gt, gl, gk = (np.zeros(na, dtype=np.int32) for _ in range(3))
        hsd = np.zeros(na)
        ngt = np.zeros(nreg, dtype=np.int32)
        reps = np.zeros(na, dtype=np.int32)
        rc = self._L.otg_genotype_cluster_batch(self._h, C.byref(params), abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(seq_off),
                                                abi.ptr(seq_len), abi.ptr(first_allele), abi.ptr(n_alleles), C.c_uint32(nreg),
                                                abi.ptr(gt), abi.ptr(gl), abi.ptr(gk), abi.ptr(hsd), abi.ptr(ngt), abi.ptr(reps))
        self._check(rc, "otg_genotype_cluster_batch")
        return gt, gl, gk, hsd, ngt, reps

    def genotype_cluster_metric_batch(self, params, arena, seq_off, seq_len, first_allele, n_alleles, metric="length"):
        """otg_genotype_cluster_metric_batch -> (gt, gt_l, gt_k, hsd, n_gt, reps, dist, n_aligned): metric "length" (the reference's
        length-ratio matrix) or "edit" (edit distance / longer length, always exact); dist = the first matrix as clustered (condensed,
        region after region), n_aligned = pairs of distinct sequences scored (0 under "length")."""
        m = abi.gt_metric(metric)
        nreg = len(n_alleles)
        na = len(seq_off)
        gt, gl, gk = (np.zeros(na, dtype=np.int32) for _ in range(3))
        hsd = np.zeros(na)
        ngt = np.zeros(nreg, dtype=np.int32)
        reps = np.zeros(na, dtype=np.int32)
        A = np.asarray(n_alleles, dtype=np.int64)
        npairs = int((A * (A - 1) // 2).sum())
        dist = np.zeros(npairs + 1)
        n_aligned = C.c_uint64(0)
        rc = self._L.otg_genotype_cluster_metric_batch(self._h, C.byref(params), abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(seq_off),
                                                       abi.ptr(seq_len), abi.ptr(first_allele), abi.ptr(n_alleles), C.c_uint32(nreg),
                                                       abi.ptr(gt), abi.ptr(gl), abi.ptr(gk), abi.ptr(hsd), abi.ptr(ngt), abi.ptr(reps),
                                                       C.c_int32(m), abi.ptr(dist), C.byref(n_aligned))
        self._check(rc, "otg_genotype_cluster_metric_batch")
        return gt, gl, gk, hsd, ngt, reps, dist[:npairs], int(n_aligned.value)

    def genotype_metric_last_ms(self):
        """(align_ms, cluster_ms) of the latest genotype_cluster_metric_batch / cohort_genotype (otg_genotype_metric_last_ms)."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(self._L.otg_genotype_metric_last_ms(self._h, C.byref(a), C.byref(b)), "otg_genotype_metric_last_ms")
        return float(a.value), float(b.value)

    def genotype_cluster_trace_batch(self, params, arena, seq_off, seq_len, first_allele, n_alleles):
        """otg_genotype_cluster_trace_batch: genotype_cluster_batch's tuple plus a dict of the kernel's matrices: dl, dk (condensed, region
        after region), kvec [alleles, 65], vnorm, height_l, height_k [alleles; A - 1 used from a region's first allele on]."""
        nreg = len(n_alleles)
        na = len(seq_off)
        gt, gl, gk = (np.zeros(na, dtype=np.int32) for _ in range(3))
        hsd = np.zeros(na)
        ngt = np.zeros(nreg, dtype=np.int32)
        reps = np.zeros(na, dtype=np.int32)
        A = np.asarray(n_alleles, dtype=np.int64)
        npairs = int((A * (A - 1) // 2).sum())
        tr = {"dl": np.zeros(npairs + 1), "dk": np.zeros(npairs + 1), "kvec": np.zeros((na + 1, 65)), "vnorm": np.zeros(na + 1),
              "height_l": np.zeros(na + 1), "height_k": np.zeros(na + 1)}
        t = otg_genotype_trace(*(tr[n].ctypes.data for n, _ in otg_genotype_trace._fields_))
        rc = self._L.otg_genotype_cluster_trace_batch(self._h, C.byref(params), abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(seq_off),
                                                      abi.ptr(seq_len), abi.ptr(first_allele), abi.ptr(n_alleles), C.c_uint32(nreg),
                                                      abi.ptr(gt), abi.ptr(gl), abi.ptr(gk), abi.ptr(hsd), abi.ptr(ngt), abi.ptr(reps), C.byref(t))
        self._check(rc, "otg_genotype_cluster_trace_batch")
        tr = {"dl": tr["dl"][:npairs], "dk": tr["dk"][:npairs], "kvec": tr["kvec"][:na], "vnorm": tr["vnorm"][:na],
              "height_l": tr["height_l"][:na], "height_k": tr["height_k"][:na]}
        return (gt, gl, gk, hsd, ngt, reps), tr

    def last_kernel_ms(self):
        """HIP-event time of the kernels of the latest genotype_cluster_batch (otg_last_kernel_ms)."""
        ms = C.c_double(0.0)
        self._check(self._L.otg_last_kernel_ms(self._h, C.byref(ms)), "otg_last_kernel_ms")
        return float(ms.value)

    # ------------------------------------------------------------------ L3
    def assemble_submit(self, params, batch, region_range=None):
        arena, reads, regions = batch["arena"], batch["reads"], batch["regions"]
        if region_range is not None:
            a, b = region_range
            regions = np.ascontiguousarray(regions[a:b])
        self._n_regions = len(regions)
        self._n_reads = len(reads)
        self._first_read = int(regions["first_read"].min()) if len(regions) else 0
        rc = self._L.otg_assemble_submit(self._h, C.byref(params), abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(reads),
                                         C.c_uint32(len(reads)), abi.ptr(regions), C.c_uint32(len(regions)))
        self._check(rc, "otg_assemble_submit")

    def assemble_run(self):
        self._check(self._L.otg_assemble_run(self._h), "otg_assemble_run")

    def realign_reads(self, params, batch):
        """local_realignment alone (`--reads-only -r`): the read descriptors after the flank rescue (otg_assemble_realign)."""
        self.assemble_submit(params, batch)
        self._check(self._L.otg_assemble_realign(self._h), "otg_assemble_realign")
        out = np.zeros(len(batch["reads"]), dtype=abi.read_dt)
        self._check(self._L.otg_assemble_collect_reads(self._h, abi.ptr(out), C.c_uint32(len(out))), "otg_assemble_collect_reads")
        return out

    def assemble_collect(self):
        na = C.c_uint32(0)
        sb = C.c_uint64(0)
        self._check(self._L.otg_assemble_result_sizes(self._h, C.byref(na), C.byref(sb)), "otg_assemble_result_sizes")
        res = {
            "regions": np.zeros(self._n_regions, dtype=abi.region_result_dt),
            "alleles": np.zeros(na.value, dtype=abi.allele_dt),
            "seqs": np.zeros(max(1, sb.value), dtype=np.uint8),
            "labels": np.zeros(self._n_reads, dtype=np.int32),
        }
        rc = self._L.otg_assemble_collect(self._h, abi.ptr(res["regions"]), abi.ptr(res["alleles"]), C.c_uint32(na.value),
                                          abi.ptr(res["seqs"]), C.c_uint64(res["seqs"].size), abi.ptr(res["labels"]))
        self._check(rc, "otg_assemble_collect")
        return res

    def assemble_device_results(self):
        """Device-resident results of the last run as zero-copy torch uint8 tensors on this context's GPU
        (valid until the next submit / run): {"regions", "alleles", "seqs"} + counts.  Used by the multi-GPU
        gather so that allele records travel GPU -> GPU (RCCL) without a host round trip."""
        import torch
        na = C.c_uint32(0)
        sb = C.c_uint64(0)
        self._check(self._L.otg_assemble_result_sizes(self._h, C.byref(na), C.byref(sb)), "otg_assemble_result_sizes")
        pr, pa, ps = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.otg_assemble_device_results(self._h, C.byref(pr), C.byref(pa), C.byref(ps)), "otg_assemble_device_results")
        dev = torch.device("cuda", self.device)

        class _Span:          # minimal __cuda_array_interface__ carrier: torch.as_tensor wraps it without copying
            def __init__(self, ptr, nbytes):
                self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2, "strides": None}

        def wrap(ptr, nbytes):
            if not ptr or nbytes == 0:
                return torch.zeros(0, dtype=torch.uint8, device=dev)
            return torch.as_tensor(_Span(ptr, int(nbytes)), device=dev)

        return {"regions": wrap(pr.value, self._n_regions * abi.region_result_dt.itemsize),
                "alleles": wrap(pa.value, na.value * abi.allele_dt.itemsize),
                "seqs": wrap(ps.value, sb.value), "n_alleles": int(na.value), "n_regions": int(self._n_regions)}

    def assemble_collect_dist(self, n_slots):
        """The pair-distance matrices of the last run (otg_assemble_collect_dist): n_slots doubles, region r's condensed matrix at the sum of
        N (N - 1) / 2 over the regions before it."""
        out = np.zeros(max(1, int(n_slots)))
        self._check(self._L.otg_assemble_collect_dist(self._h, abi.ptr(out), C.c_uint64(int(n_slots))), "otg_assemble_collect_dist")
        return out[:int(n_slots)]

    def assemble_stats(self):
        st = np.zeros(1, dtype=abi.run_stats_dt)
        self._check(self._L.otg_assemble_stats(self._h, abi.ptr(st)), "otg_assemble_stats")
        return st[0]

    def assemble(self, params, batch, region_range=None):
        self.assemble_submit(params, batch, region_range)
        self.assemble_run()
        return self.assemble_collect()

    def assemble_spread(self, unit_sets, region_set, match=2, mismatch=7, indel=7, min_score=24, device_tensor=False):
        """otg_assemble_spread (and otg_spread_collect, otg_spread_collect_reads) after assemble_run on this context: per consensus allele the
        order statistics of the repeat length among the reads that voted for it, the reads parsed where the run left them in HBM
        (include/otter_gpu.h states the rule).  unit_sets: a list of lists of byte strings; region_set: per region an index into it, or None /
        abi.SPREAD_NONE for a region without a set -> (records [n_alleles] of abi.spread_dt, unit_off [n_alleles + 1] uint64, unit_records of
        abi.spread_unit_dt, reads [n_reads] of abi.spread_read_dt) as numpy arrays; or with device_tensor=True as torch tensors on this
        context's device that wrap the results in HBM without a copy (int32 [n, 16], int64 [n + 1], int32 [units, 6], int32 [reads, 6]; valid
        until the next spread call on this context).  Afterwards the locus results on the context are the reads' records, by reads["task"]."""
        sets, _, _ = _pack_unit_sets(unit_sets, [], [])
        rs = np.ascontiguousarray([abi.SPREAD_NONE if q is None else q for q in region_set], dtype=np.uint32)
        q = abi.TractParams(match, mismatch, indel, min_score)
        na, sb = C.c_uint32(0), C.c_uint64(0)
        if self._L.otg_assemble_result_sizes(self._h, C.byref(na), C.byref(sb)) != 0:
            na.value = 0                                                    # (no completed run: the entry below says what is missing)
        rec = np.zeros(na.value, dtype=abi.spread_dt)
        unit_off = np.zeros(na.value + 1, dtype=np.uint64)
        nu = C.c_uint64(0)
        rc = self._L.otg_assemble_spread(self._h, *sets, abi.ptr(rs) if len(rs) else None, C.c_uint32(len(rs)), C.byref(q), None if device_tensor else abi.ptr(rec),
                                         None if device_tensor else abi.ptr(unit_off), C.byref(nu))
        self._check(rc, "otg_assemble_spread")
        if device_tensor:
            m, u2, nr = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
            p = [C.c_void_p() for _ in range(4)]
            self._check(self._L.otg_spread_device_results(self._h, C.byref(m), C.byref(p[0]), C.byref(p[1]), C.byref(u2), C.byref(p[2]), C.byref(nr), C.byref(p[3])),
                        "otg_spread_device_results")
            assert (m.value, u2.value) == (na.value, nu.value)
            return (self._wrap_device(p[0].value, (m.value, 16), "<i4"), self._wrap_device(p[1].value, (m.value + 1,), "<i8"),
                    self._wrap_device(p[2].value, (u2.value, 6), "<i4"), self._wrap_device(p[3].value, (nr.value, 6), "<i4"))
        units = np.zeros(nu.value, dtype=abi.spread_unit_dt)
        self._check(self._L.otg_spread_collect(self._h, abi.ptr(units) if nu.value else None, C.c_uint64(nu.value)), "otg_spread_collect")
        nr = C.c_uint32(0)
        self._check(self._L.otg_spread_device_results(self._h, None, None, None, None, None, C.byref(nr), None), "otg_spread_device_results")
        reads = np.zeros(nr.value, dtype=abi.spread_read_dt)
        self._check(self._L.otg_spread_collect_reads(self._h, abi.ptr(reads) if nr.value else None, C.c_uint32(nr.value)), "otg_spread_collect_reads")
        return rec, unit_off, units, reads

    def spread_last_ms(self):
        """(the device work of the call summed, the reads' locus call, the consensus locus call, the stats kernel) ms of the latest assemble_spread (HIP events)."""
        return self._last_ms("otg_spread_last_ms", 4)

    def locus_last(self, device_tensor=False):
        """the locus results that lie on this context (otg_locus_device_results / otg_locus_collect) -> (records, seg_off, segs) as locus_batch
        returns them.  After assemble_spread they are the reads' records, indexed by the task of the read records."""
        m, t, ps, po, pg = C.c_uint32(0), C.c_uint64(0), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.otg_locus_device_results(self._h, C.byref(m), C.byref(ps), C.byref(po), C.byref(pg), C.byref(t)), "otg_locus_device_results")
        recs = self._wrap_device(ps.value, (m.value, 8), "<i4")
        off = self._wrap_device(po.value, (m.value + 1,), "<i8")
        segs = self._wrap_device(pg.value, (t.value, 6), "<i4")
        if device_tensor:
            return recs, off, segs
        return (recs.cpu().numpy().view(np.uint32).reshape(-1, 8).copy().view(abi.locus_dt).reshape(-1), off.cpu().numpy().astype(np.uint64),
                segs.cpu().numpy().view(np.uint32).reshape(-1, 6).copy().view(abi.unitparse_seg_dt).reshape(-1))


    # ------------------------------------------------------------------ cohort (assemble -> genotype without leaving the device)
    def cohort_begin(self, n_regions, n_samples):
        """otg_cohort_begin: opens the staging area of one batch of n_regions regions for n_samples samples."""
        self._check(self._L.otg_cohort_begin(self._h, C.c_uint32(n_regions), C.c_uint32(n_samples)), "otg_cohort_begin")
        self._cohort_regions, self._cohort_samples = int(n_regions), int(n_samples)

    def cohort_stage(self, sample, src=None):
        """otg_cohort_stage: the results of the latest assemble_run of `src` (default: this context) become sample `sample` of the batch."""
        self._check(self._L.otg_cohort_stage(self._h, (src or self)._h, C.c_uint32(sample)), "otg_cohort_stage")

    def cohort_regroup(self, ref_arena, ref_off, ref_len):
        """otg_cohort_regroup: uploads the reference allele of every region (bytes ref_arena[ref_off[r] : ref_off[r] + ref_len[r]]) and regroups
        the staged alleles on the device into the inputs of anallele_cluster."""
        ref_arena = np.ascontiguousarray(ref_arena, dtype=np.uint8)
        ref_off = np.ascontiguousarray(ref_off, dtype=np.uint64)
        ref_len = np.ascontiguousarray(ref_len, dtype=np.uint32)
        self._check(self._L.otg_cohort_regroup(self._h, abi.ptr(ref_arena), C.c_uint64(ref_arena.size), abi.ptr(ref_off), abi.ptr(ref_len)), "otg_cohort_regroup")

    def cohort_genotype(self, params, ref_arena=None, ref_off=None, ref_len=None, metric="length"):
        """otg_cohort_genotype (after cohort_regroup when the reference alleles are given): anallele_cluster on the regrouped buffers;
        metric="edit": otg_genotype_cohort_metric with OTG_GT_METRIC_EDIT."""
        m = abi.gt_metric(metric)
        if ref_off is not None:
            self.cohort_regroup(ref_arena, ref_off, ref_len)
        if m == abi.OTG_GT_METRIC_LENGTH:
            self._check(self._L.otg_cohort_genotype(self._h, C.byref(params)), "otg_cohort_genotype")
        else:
            self._check(self._L.otg_genotype_cohort_metric(self._h, C.byref(params), C.c_int32(m)), "otg_genotype_cohort_metric")

    def cohort_collect(self, clustered=True):
        """otg_cohort_collect -> {"first_allele" [n_regions + 1], "n_alleles", "alleles" (allele_dt, .label = sample index), "sample", "seq_off",
        "seq_len", "arena" (+ 64 slack bytes)} and, with clustered=True, "gt", "gt_l", "gt_k", "hsd", "n_gt", "reps"."""
        na, sb = C.c_uint32(0), C.c_uint64(0)
        self._check(self._L.otg_cohort_result_sizes(self._h, C.byref(na), C.byref(sb)), "otg_cohort_result_sizes")
        n, B = na.value, self._cohort_regions
        res = {"first_allele": np.zeros(B + 1, dtype=np.uint32), "alleles": np.zeros(n, dtype=abi.allele_dt), "sample": np.zeros(n, dtype=np.int32),
               "seq_off": np.zeros(n, dtype=np.uint64), "seq_len": np.zeros(n, dtype=np.uint32), "arena": np.zeros(sb.value + 64, dtype=np.uint8)}
        if clustered:
            res.update({"gt": np.zeros(n, dtype=np.int32), "gt_l": np.zeros(n, dtype=np.int32), "gt_k": np.zeros(n, dtype=np.int32), "hsd": np.zeros(n),
                        "n_gt": np.zeros(B, dtype=np.int32), "reps": np.zeros(n, dtype=np.int32)})
        g = lambda k: abi.ptr(res[k]) if k in res else None
        rc = self._L.otg_cohort_collect(self._h, g("first_allele"), g("alleles"), C.c_uint32(n), g("sample"), g("seq_off"), g("seq_len"), g("arena"),
                                        C.c_uint64(sb.value), g("gt"), g("gt_l"), g("gt_k"), g("hsd"), g("n_gt"), g("reps"))
        self._check(rc, "otg_cohort_collect")
        res["n_alleles"] = np.diff(res["first_allele"].astype(np.int64)).astype(np.uint32)
        res["seq_bytes"] = int(sb.value)
        return res

    def cohort_kmer_rows(self, device_tensor=False):
        """otg_kmer_cohort_rows (after cohort_genotype): the rows of the batch's k-mer usage matrix, the alleles of every VCF line in column
        order -> {"n_rows", "row_first" [n_regions + 1], "row_allele" [n_rows] (indices into cohort_collect's arrays), "sample_gt"
        [n_regions, n_samples, 2] (the GT numbers the VCF prints, -1 -1 for ./.)}: uint32 / uint32 / int32 numpy arrays, or with
        device_tensor=True int32 torch tensors that wrap the lists in HBM (valid until the next cohort_regroup)."""
        B, S = self._cohort_regions, self._cohort_samples
        n = C.c_uint32(0)
        if device_tensor:
            pf, pa, pg = C.c_void_p(), C.c_void_p(), C.c_void_p()
            self._check(self._L.otg_kmer_cohort_device_rows(self._h, C.byref(n), C.byref(pf), C.byref(pa), C.byref(pg)), "otg_kmer_cohort_device_rows")
            return {"n_rows": n.value, "row_first": self._wrap_device(pf.value, (B + 1,), "<i4"), "row_allele": self._wrap_device(pa.value, (n.value,), "<i4"),
                    "sample_gt": self._wrap_device(pg.value, (B, S, 2), "<i4")}
        self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(n), None, None, None), "otg_kmer_cohort_rows")
        res = {"n_rows": n.value, "row_first": np.zeros(B + 1, dtype=np.uint32), "row_allele": np.zeros(n.value, dtype=np.uint32),
               "sample_gt": np.zeros((B, S, 2), dtype=np.int32)}
        self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(n), abi.ptr(res["row_first"]), abi.ptr(res["row_allele"]), abi.ptr(res["sample_gt"])),
                    "otg_kmer_cohort_rows")
        return res

    def cohort_kmer_usage(self, k, row_begin=0, n=None, device_tensor=False):
        """otg_kmer_cohort_usage: rows [row_begin, row_begin + n) of the row list (n=None: to the end) through the k-mer tiers, read in the
        cohort arena in place -> (usage [n, 4^k+1], gc [n], hsd [n]) as numpy arrays, or with device_tensor=True as float64 torch tensors
        wrapping HBM (valid until the next k-mer call on this context), as kmer_usage_batch returns them."""
        if n is None:
            total = C.c_uint32(0)
            self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(total), None, None, None), "otg_kmer_cohort_rows")
            n = max(0, total.value - int(row_begin))
        n, k = int(n), int(k)
        if device_tensor:
            self._check(self._L.otg_kmer_cohort_usage(self._h, C.c_int32(k), C.c_uint32(row_begin), C.c_uint32(n), None, None, None), "otg_kmer_cohort_usage")
            return self._kmer_device_results(n, k)
        bins = 4 ** k + 1 if 1 <= k <= abi.KMER_MAX else 1
        usage, gc, hsd = np.zeros((n, bins), dtype=np.float64), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        self._check(self._L.otg_kmer_cohort_usage(self._h, C.c_int32(k), C.c_uint32(row_begin), C.c_uint32(n), abi.ptr(usage), abi.ptr(gc), abi.ptr(hsd)),
                    "otg_kmer_cohort_usage")
        return usage, gc, hsd

    def cohort_motifs(self, row_begin=0, n=None, max_period=256, slack=50, unit_stride=None, device_tensor=False):
        """otg_motif_cohort: the motif annotation of rows [row_begin, row_begin + n) of the row list (n=None: to the end), the alleles read in
        the cohort arena in place -> (records, units) as motif_batch returns them.  unit_stride=None: max_period (the row lengths are on the
        device only)."""
        if n is None:
            total = C.c_uint32(0)
            self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(total), None, None, None), "otg_kmer_cohort_rows")
            n = max(0, total.value - int(row_begin))
        n = int(n)
        stride = int(max_period) if unit_stride is None else int(unit_stride)
        rec = np.zeros(n, dtype=abi.motif_dt)
        units = np.zeros((n, max(stride, 1)), dtype=np.uint8)
        rc = self._L.otg_motif_cohort(self._h, C.c_uint32(row_begin), C.c_uint32(n), C.c_uint32(max_period), C.c_uint32(slack),
                                      None if device_tensor else abi.ptr(rec), None if device_tensor else abi.ptr(units), C.c_uint32(stride))
        self._check(rc, "otg_motif_cohort")
        return self._motif_device_results(n, stride) if device_tensor else (rec, units[:, :stride])

    def cohort_repeats(self, row_begin=0, n=None, max_period=256, min_copies=2, min_span=12, device_tensor=False):
        """otg_repeat_cohort: the repeat structure of rows [row_begin, row_begin + n) of the row list (n=None: to the end), the alleles read in
        the cohort arena in place -> (sums, seg_off, segs) as repeat_batch returns them."""
        if n is None:
            total = C.c_uint32(0)
            self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(total), None, None, None), "otg_kmer_cohort_rows")
            n = max(0, total.value - int(row_begin))
        n = int(n)
        return self._seg_results("repeat", n, device_tensor, lambda sums, seg_off, total: self._L.otg_repeat_cohort(
            self._h, C.c_uint32(row_begin), C.c_uint32(n), C.c_uint32(max_period), C.c_uint32(min_copies), C.c_uint32(min_span), sums, seg_off, total),
            "otg_repeat_cohort")

    def cohort_unitalign(self, row_begin=0, n=None, units=None, task_seq=None, task_unit=None, device_tensor=False):
        """otg_unitalign_cohort: rows [row_begin, row_begin + n) of the row list (n=None: to the end) aligned to cyclic repeat units, the alleles
        read in the cohort arena in place -> records as unitalign_batch returns them.  units=None: row i against the unit the latest
        cohort_motifs over the same rows found for it.  Otherwise a list of byte strings with task lists as in unitalign_batch, task_seq
        counted from row_begin."""
        if n is None:
            total = C.c_uint32(0)
            self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(total), None, None, None), "otg_kmer_cohort_rows")
            n = max(0, total.value - int(row_begin))
        n = int(n)
        if units is None:
            nt, args = n, (None, C.c_uint64(0), None, None, C.c_uint32(0), None, None, C.c_uint32(0))
        else:
            uarena, uoff, ulen = _pack_units(units)
            ts = np.ascontiguousarray(task_seq, dtype=np.uint32)
            tu = np.ascontiguousarray(task_unit, dtype=np.uint32)
            if len(ts) != len(tu):
                raise ValueError("task_seq and task_unit differ in length")
            nt, args = len(ts), (abi.ptr(uarena), C.c_uint64(int(ulen.sum())), abi.ptr(uoff), abi.ptr(ulen), C.c_uint32(len(ulen)), abi.ptr(ts), abi.ptr(tu),
                                 C.c_uint32(len(ts)))
        out = np.zeros(nt, dtype=abi.unitalign_dt)
        rc = self._L.otg_unitalign_cohort(self._h, C.c_uint32(row_begin), C.c_uint32(n), *args, None if device_tensor else abi.ptr(out))
        self._check(rc, "otg_unitalign_cohort")
        return self._unitalign_device_results(nt) if device_tensor else out

    def cohort_tracts(self, row_begin=0, n=None, units=None, task_seq=None, task_unit=None, match=2, mismatch=7, indel=7, min_score=24, device_tensor=False):
        """otg_tract_cohort: the tracts inside rows [row_begin, row_begin + n) of the row list (n=None: to the end), the alleles read in the cohort
        arena in place -> records as tract_batch returns them.  units=None: row i against the unit the latest cohort_motifs over the same rows
        found for it.  Otherwise a list of byte strings with task lists as in tract_batch, task_seq counted from row_begin."""
        if n is None:
            total = C.c_uint32(0)
            self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(total), None, None, None), "otg_kmer_cohort_rows")
            n = max(0, total.value - int(row_begin))
        n = int(n)
        if units is None:
            nt, args = n, (None, C.c_uint64(0), None, None, C.c_uint32(0), None, None, C.c_uint32(0))
        else:
            uarena, uoff, ulen = _pack_units(units)
            ts = np.ascontiguousarray(task_seq, dtype=np.uint32)
            tu = np.ascontiguousarray(task_unit, dtype=np.uint32)
            if len(ts) != len(tu):
                raise ValueError("task_seq and task_unit differ in length")
            nt, args = len(ts), (abi.ptr(uarena), C.c_uint64(int(ulen.sum())), abi.ptr(uoff), abi.ptr(ulen), C.c_uint32(len(ulen)), abi.ptr(ts), abi.ptr(tu),
                                 C.c_uint32(len(ts)))
        out = np.zeros(nt, dtype=abi.tract_dt)
        q = abi.TractParams(match, mismatch, indel, min_score)
        rc = self._L.otg_tract_cohort(self._h, C.c_uint32(row_begin), C.c_uint32(n), *args, C.byref(q), None if device_tensor else abi.ptr(out))
        self._check(rc, "otg_tract_cohort")
        return self._tract_device_results(nt) if device_tensor else out

    def cohort_unitparse(self, unit_sets, task_seq, task_set, row_begin=0, n=None, device_tensor=False):
        """otg_unitparse_cohort: rows [row_begin, row_begin + n) of the row list (n=None: to the end) parsed against unit sets, the alleles read
        in the cohort arena in place -> (sums, seg_off, segs) as unitparse_batch returns them; task_seq counts from row_begin."""
        if n is None:
            total = C.c_uint32(0)
            self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(total), None, None, None), "otg_kmer_cohort_rows")
            n = max(0, total.value - int(row_begin))
        n = int(n)
        sets, ts, tq = _pack_unit_sets(unit_sets, task_seq, task_set)
        return self._seg_results("unitparse", len(ts), device_tensor, lambda sums, seg_off, total: self._L.otg_unitparse_cohort(
            self._h, C.c_uint32(row_begin), C.c_uint32(n), *sets, abi.ptr(ts), abi.ptr(tq), C.c_uint32(len(ts)), sums, seg_off, total), "otg_unitparse_cohort")

    def cohort_loci(self, unit_sets, task_seq, task_set, row_begin=0, n=None, match=2, mismatch=7, indel=7, min_score=24, device_tensor=False):
        """otg_locus_cohort: the locus mode over rows [row_begin, row_begin + n) of the row list (n=None: to the end), the alleles read in the
        cohort arena in place -> (records, seg_off, segs) as locus_batch returns them; task_seq counts from row_begin."""
        if n is None:
            total = C.c_uint32(0)
            self._check(self._L.otg_kmer_cohort_rows(self._h, C.byref(total), None, None, None), "otg_kmer_cohort_rows")
            n = max(0, total.value - int(row_begin))
        n = int(n)
        sets, ts, tq = _pack_unit_sets(unit_sets, task_seq, task_set)
        q = abi.TractParams(match, mismatch, indel, min_score)
        return self._seg_results("locus", len(ts), device_tensor, lambda recs, seg_off, total: self._L.otg_locus_cohort(
            self._h, C.c_uint32(row_begin), C.c_uint32(n), *sets, abi.ptr(ts), abi.ptr(tq), C.c_uint32(len(ts)), C.byref(q), recs, seg_off, total), "otg_locus_cohort")

    def cohort_unitsets(self, max_period=256, min_copies=2, min_span=12, min_bases=12, min_permille=50, redundant_permille=100, device_tensor=False):
        """the unit set of every region of the open cohort batch: cohort_repeats over the whole row list, then the discovery with row_first as
        the groups (one group per VCF line), the alleles read in the cohort arena in place -> as unitset_repeats returns it."""
        self.cohort_repeats(0, None, max_period, min_copies, min_span, device_tensor=True)
        return self.unitset_repeats(self.cohort_kmer_rows()["row_first"], min_bases, min_permille, redundant_permille, device_tensor)

    def cohort_end(self):
        self._check(self._L.otg_cohort_end(self._h), "otg_cohort_end")


class Comm:
    """An RCCL communicator of the library (otg_comm_create): one per process and GPU, for Context.gather_records_rccl."""

    def __init__(self, device, rank, world, uid):
        L = load()
        h = C.c_void_p()
        L.otg_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
        rc = L.otg_comm_create(int(device), int(rank), int(world), uid, C.byref(h))
        if rc != 0:
            raise OtterGpuError("otg_comm_create failed (%d): %s" % (rc, (L.otg_last_error(None) or b"").decode()))
        self._h, self._L, self.rank, self.world = h, L, int(rank), int(world)
        L.otg_comm_destroy.argtypes = [C.c_void_p]

    @staticmethod
    def unique_id():
        L = load()
        buf = C.create_string_buffer(128)
        rc = L.otg_comm_unique_id(buf)
        if rc != 0:
            raise OtterGpuError("otg_comm_unique_id failed (%d): %s" % (rc, (L.otg_last_error(None) or b"").decode()))
        return buf.raw

    def close(self):
        if getattr(self, "_h", None):
            self._L.otg_comm_destroy(self._h)
            self._h = None

    def gather_records(self, ctx):
        """End-of-run gather of ctx's last results to rank 0 (otg_gather_sizes + otg_gather_records).  Rank 0 gets
        {"regions", "alleles", "seqs", "counts"} of the whole job in rank order; the other ranks get {"counts"}."""
        L = self._L
        counts = np.zeros(3 * self.world, dtype=np.uint64)
        L.otg_gather_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.otg_gather_records.argtypes = [C.c_void_p] * 6
        ctx._check(L.otg_gather_sizes(ctx._h, self._h, abi.ptr(counts)), "otg_gather_sizes")
        if self.rank != 0:
            ctx._check(L.otg_gather_records(ctx._h, self._h, abi.ptr(counts), None, None, None), "otg_gather_records")
            return {"counts": counts.reshape(-1, 3)}
        tot = counts.reshape(-1, 3).sum(axis=0)
        res = {"regions": np.zeros(int(tot[0]), dtype=abi.region_result_dt), "alleles": np.zeros(int(tot[1]), dtype=abi.allele_dt),
               "seqs": np.zeros(max(1, int(tot[2])), dtype=np.uint8), "counts": counts.reshape(-1, 3)}
        ctx._check(L.otg_gather_records(ctx._h, self._h, abi.ptr(counts), abi.ptr(res["regions"]), abi.ptr(res["alleles"]), abi.ptr(res["seqs"])), "otg_gather_records")
        return res


def device_count():
    return load().otg_device_count()


def emit_alleles(beds, chr_arena, res, read_group="", fasta=False):
    """Text of the allele records of a collected batch exactly as `otter assemble` prints them (otg_emit_alleles;
    src/assemble.cpp:143-149).  res: dict with "regions", "alleles", "seqs" (Context.assemble_collect)."""
    L = load()
    n = C.c_uint64(0)
    args = [abi.ptr(beds), abi.ptr(chr_arena, C.c_char_p), C.c_uint32(len(beds)), abi.ptr(res["regions"]), abi.ptr(res["alleles"]),
            abi.ptr(res["seqs"]), C.c_char_p(read_group.encode()), C.c_int(1 if fasta else 0)]
    rc = L.otg_emit_alleles(*args, None, C.c_uint64(0), C.byref(n))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_emit_alleles failed (%d): %s" % (rc, (L.otg_last_error(None) or b"").decode()))
    out = np.zeros(max(1, n.value), dtype=np.uint8)
    rc = L.otg_emit_alleles(*args, abi.ptr(out, C.c_char_p), C.c_uint64(out.size), C.byref(n))
    if rc != 0:
        raise OtterGpuError("otg_emit_alleles failed (%d)" % rc)
    return out[:n.value].tobytes()


def emit_sam_header(targets, read_group="", offset_l=0, offset_r=0):
    """targets: list of (name, length) -> the @SQ/@RG/@PG header lines of src/assemble.cpp:167-177."""
    L = load()
    names = b"".join(t[0].encode() for t in targets) + b"\0"
    off = np.cumsum([0] + [len(t[0].encode()) for t in targets[:-1]]).astype(np.uint64) if targets else np.zeros(0, np.uint64)
    ln = np.array([len(t[0].encode()) for t in targets], dtype=np.uint32)
    tl = np.array([t[1] for t in targets], dtype=np.uint64)
    out = np.zeros(64 + sum(40 + len(t[0]) for t in targets) + len(read_group), dtype=np.uint8)
    n = C.c_uint64(0)
    rc = L.otg_emit_sam_header(C.c_char_p(names), abi.ptr(off), abi.ptr(ln), abi.ptr(tl), C.c_uint32(len(targets)), C.c_char_p(read_group.encode()),
                               C.c_int32(offset_l), C.c_int32(offset_r), abi.ptr(out, C.c_char_p), C.c_uint64(out.size), C.byref(n))
    if rc != 0:
        raise OtterGpuError("otg_emit_sam_header failed (%d)" % rc)
    return out[:n.value].tobytes()


class Bam:
    """An indexed BAM (otg_bam_open: <path> + <path>.bai) as the source of region batches (otg_ingest_regions)."""

    def __init__(self, path):
        L = load()
        h = C.c_void_p()
        rc = L.otg_bam_open(C.c_char_p(path.encode()), C.byref(h))
        if rc != 0:
            raise OtterGpuError("otg_bam_open failed (%d): %s" % (rc, (L.otg_last_error(None) or b"").decode()))
        self._h, self._L, self._path = h, L, path
        L.otg_bam_target.restype = C.c_char_p
        L.otg_bam_n_targets.restype = C.c_uint32

    def close(self):
        if getattr(self, "_h", None):
            self._L.otg_bam_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def targets(self):
        out = []
        for i in range(self._L.otg_bam_n_targets(self._h)):
            ln = C.c_uint64(0)
            nm = self._L.otg_bam_target(self._h, C.c_uint32(i), C.byref(ln))
            out.append((nm.decode(), int(ln.value)))
        return out

    def sample_index(self):
        """SampleIndex of an allele BAM (otg_bam_sample_index): ([sample names in header order], offset_l, offset_r)."""
        n, ol, orr = C.c_uint32(0), C.c_int32(0), C.c_int32(0)
        rc = self._L.otg_bam_sample_index(self._h, C.byref(n), C.byref(ol), C.byref(orr))
        if rc != 0:
            raise OtterGpuError("otg_bam_sample_index failed (%d): %s" % (rc, (self._L.otg_last_error(None) or b"").decode()))
        self._L.otg_bam_sample.restype = C.c_char_p
        return [self._L.otg_bam_sample(self._h, C.c_uint32(i)).decode("latin-1") for i in range(n.value)], int(ol.value), int(orr.value)

    def ingest_alleles(self, regions, reference=None, threads=1):
        """The allele records of each region (otg_ingest_alleles) -> {"alleles", "first_allele", "arena"}; with reference (a Fasta)
        the reference allele is appended to every non-empty region, as `otter genotype -r` does."""
        beds, carena = regions if isinstance(regions, tuple) else abi.make_beds(regions)
        fsz = os.path.getsize(self._path)
        cap_n, cap_a = max(1024, fsz // 32), max(1 << 20, 8 * fsz)
        first = np.zeros(len(beds) + 1, dtype=np.uint32)
        while True:
            alleles = np.zeros(cap_n, dtype=abi.allele_dt)
            arena = np.zeros(cap_a, dtype=np.uint8)
            used, na = C.c_uint64(0), C.c_uint32(0)
            rc = self._L.otg_ingest_alleles(self._h, abi.ptr(beds), abi.ptr(carena, C.c_char_p), C.c_uint32(len(beds)), C.c_int32(threads),
                                            reference._h if reference is not None else None, abi.ptr(arena), C.c_uint64(cap_a), C.byref(used),
                                            abi.ptr(alleles), C.c_uint32(cap_n), C.byref(na), abi.ptr(first))
            if rc == abi.OTG_ERR_CAPACITY:
                cap_n, cap_a = max(cap_n, na.value + 16), max(cap_a, used.value + 4096)
                continue
            if rc != 0:
                raise OtterGpuError("otg_ingest_alleles failed (%d): %s" % (rc, (self._L.otg_last_error(None) or b"").decode()))
            return {"alleles": np.ascontiguousarray(alleles[:na.value]), "first_allele": first, "arena": np.ascontiguousarray(arena[:used.value + 64])}

    def ingest_compare(self, regions, sample0, sample1, truth, threads=1):
        """otg_ingest_compare_alleles: the allele records of each region as `otter compare` reads them (sample map {sample0: 0, sample1: 1};
        truth=True: local_parse_analleles, with the spanning values) -> {"alleles", "first_allele", "arena", "spannings", "first_spanning", "warn"}."""
        beds, carena = regions if isinstance(regions, tuple) else abi.make_beds(regions)
        fsz = os.path.getsize(self._path)
        cap_n, cap_a, cap_s, cap_w = max(1024, fsz // 32), max(1 << 20, 8 * fsz), max(1024, fsz // 32), 1 << 16
        first = np.zeros(len(beds) + 1, dtype=np.uint32)
        sfirst = np.zeros(len(beds) + 1, dtype=np.uint32)
        while True:
            alleles = np.zeros(cap_n, dtype=abi.allele_dt)
            arena = np.zeros(cap_a, dtype=np.uint8)
            sp = np.zeros(cap_s, dtype=np.int32)
            warn = np.zeros(cap_w, dtype=np.uint8)
            used, na, ns, wl = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
            rc = self._L.otg_ingest_compare_alleles(self._h, C.c_char_p(sample0.encode()), C.c_char_p(sample1.encode()), C.c_int32(int(truth)),
                                                    abi.ptr(beds), abi.ptr(carena, C.c_char_p), C.c_uint32(len(beds)), C.c_int32(threads),
                                                    abi.ptr(arena), C.c_uint64(cap_a), C.byref(used), abi.ptr(alleles), C.c_uint32(cap_n), C.byref(na),
                                                    abi.ptr(first), abi.ptr(sp), C.c_uint32(cap_s), C.byref(ns), abi.ptr(sfirst),
                                                    abi.ptr(warn, C.c_char_p), C.c_uint64(cap_w), C.byref(wl))
            if rc == abi.OTG_ERR_CAPACITY:
                cap_n, cap_a, cap_s, cap_w = max(cap_n, na.value + 16), max(cap_a, used.value + 4096), max(cap_s, ns.value + 16), max(cap_w, wl.value + 64)
                continue
            if rc != 0:
                raise OtterGpuError("otg_ingest_compare_alleles failed (%d): %s" % (rc, (self._L.otg_last_error(None) or b"").decode()))
            return {"alleles": np.ascontiguousarray(alleles[:na.value]), "first_allele": first, "arena": np.ascontiguousarray(arena[:used.value + 64]),
                    "spannings": np.ascontiguousarray(sp[:ns.value]) if truth else np.zeros(0, np.int32),
                    "first_spanning": sfirst if truth else np.zeros(len(beds) + 1, np.uint32), "warn": warn[:wl.value].tobytes()}

    def ingest(self, regions, offset_l=0, offset_r=0, mapq=0, nonprimary=False, omit_nonspanning=False, read_quality=0.0, threads=1,
               names=False):
        """regions: list of (chr, start, end), or the (beds, chr_arena) pair of parse_bed_file -> batch dict {"arena", "reads",
        "regions"} for Context.assemble_submit (reference flanks, needed only with -r: Fasta.region_flanks appends them).
        names=True adds "meta" / "names" (read name and rq per read, what --reads-only prints)."""
        beds, carena = regions if isinstance(regions, tuple) else abi.make_beds(regions)
        opts = np.zeros(1, dtype=abi.ingest_opts_dt)
        opts[0]["offset_l"] = offset_l; opts[0]["offset_r"] = offset_r; opts[0]["mapq"] = mapq
        opts[0]["nonprimary"] = int(nonprimary); opts[0]["omit_nonspanning"] = int(omit_nonspanning); opts[0]["read_quality"] = read_quality; opts[0]["threads"] = threads
        regs = np.zeros(len(beds), dtype=abi.region_dt)
        # generous first guess from the file size (untouched pages cost nothing), exact retry if it was too small
        fsz = os.path.getsize(self._path)
        cap_r, cap_a = max(1024, fsz // 64), max(1 << 20, 8 * fsz)
        cap_n = max(4096, fsz // 16) if names else 0
        while True:
            reads = np.empty(cap_r, dtype=abi.read_dt)
            arena = np.empty(cap_a, dtype=np.uint8)
            meta = np.empty(cap_r, dtype=abi.read_meta_dt) if names else None
            narena = np.empty(cap_n, dtype=np.uint8) if names else None
            used, nr, nused = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
            rc = self._L.otg_ingest_regions_named(self._h, abi.ptr(beds), abi.ptr(carena, C.c_char_p), C.c_uint32(len(beds)), abi.ptr(opts),
                                                  abi.ptr(arena), C.c_uint64(cap_a), C.byref(used), abi.ptr(reads), C.c_uint32(cap_r), C.byref(nr),
                                                  abi.ptr(regs), abi.ptr(meta) if names else None, abi.ptr(narena, C.c_char_p) if names else None,
                                                  C.c_uint64(cap_n), C.byref(nused) if names else None)
            if rc == abi.OTG_ERR_CAPACITY:
                cap_r, cap_a = max(cap_r, nr.value + 16), max(cap_a, used.value + 64 * (nr.value + 2) + 4096)
                cap_n = max(cap_n, nused.value + 64) if names else 0
                continue
            if rc != 0:
                raise OtterGpuError("otg_ingest_regions failed (%d): %s" % (rc, (self._L.otg_last_error(None) or b"").decode()))
            arena[used.value:used.value + 64] = 0
            if names:
                return {"arena": np.ascontiguousarray(arena[:used.value + 64]), "reads": np.ascontiguousarray(reads[:nr.value]), "regions": regs,
                        "meta": np.ascontiguousarray(meta[:nr.value]), "names": np.ascontiguousarray(narena[:nused.value])}
            return {"arena": np.ascontiguousarray(arena[:used.value + 64]), "reads": np.ascontiguousarray(reads[:nr.value]), "regions": regs}


def _err(L):
    return (L.otg_last_error(None) or b"").decode()


def parse_bed_file(path):
    """parse_bed_file (src/anbed.cpp:65-80) through the library -> (beds, chr_arena, n_skipped); beds is an abi.bed_dt array."""
    L = load()
    cap_b, cap_c = 1024, 1 << 14
    while True:
        beds = np.zeros(cap_b, dtype=abi.bed_dt)
        carena = np.zeros(cap_c, dtype=np.uint8)
        n, used, skipped = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        rc = L.otg_parse_bed_file(C.c_char_p(path.encode()), abi.ptr(beds), C.c_uint32(cap_b), C.byref(n), abi.ptr(carena, C.c_char_p),
                                  C.c_uint64(cap_c), C.byref(used), C.byref(skipped))
        if rc == abi.OTG_ERR_CAPACITY:
            cap_b, cap_c = max(cap_b, n.value), max(cap_c, used.value)
            continue
        if rc != 0:
            raise OtterGpuError("otg_parse_bed_file failed (%d): %s" % (rc, _err(L)))
        return np.ascontiguousarray(beds[:n.value]), np.ascontiguousarray(carena[:max(1, used.value)]), int(skipped.value)


def bed_tuples(beds, chr_arena):
    """(chr, start, end) per region with the coordinates as BED::toString prints them (unsigned 32-bit, src/anbed.hpp:16-17)."""
    raw = chr_arena.tobytes()
    return [(raw[int(b["chr_off"]):int(b["chr_off"]) + int(b["chr_len"])].decode("latin-1"), int(b["start"]) & 0xffffffff, int(b["end"]) & 0xffffffff)
            for b in beds]


def emit_reads(beds, chr_arena, batch, read_group="", fasta=False, max_cov=-1):
    """The --reads-only records of an ingested batch (Bam.ingest(..., names=True)) as bytes (otg_emit_reads)."""
    L = load()
    meta, names = batch.get("meta"), batch.get("names")
    cap = int(batch["reads"]["seq_len"].sum()) * 2 + 512 * (len(batch["reads"]) + 1)
    while True:
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_uint64(0)
        rc = L.otg_emit_reads(abi.ptr(beds), abi.ptr(chr_arena, C.c_char_p), C.c_uint32(len(beds)), abi.ptr(batch["regions"]),
                              abi.ptr(batch["reads"]), abi.ptr(batch["arena"]), abi.ptr(meta) if meta is not None else None,
                              abi.ptr(names, C.c_char_p) if names is not None else None, C.c_char_p(read_group.encode()),
                              C.c_int(int(fasta)), C.c_int32(max_cov), abi.ptr(out, C.c_char_p), C.c_uint64(cap), C.byref(n))
        if rc == abi.OTG_ERR_CAPACITY:
            cap = n.value
            continue
        if rc != 0:
            raise OtterGpuError("otg_emit_reads failed (%d): %s" % (rc, _err(L)))
        return out[:n.value].tobytes()


class Fasta:
    """An indexed, uncompressed FASTA (otg_fasta_open) — the source of the reference flanks of local_realignment (-r)."""

    def __init__(self, path):
        L = load()
        h = C.c_void_p()
        rc = L.otg_fasta_open(C.c_char_p(path.encode()), C.byref(h))
        if rc != 0:
            raise OtterGpuError("otg_fasta_open failed (%d): %s" % (rc, _err(L)))
        self._h, self._L = h, L
        L.otg_fasta_seq.restype = C.c_char_p
        L.otg_fasta_n_seqs.restype = C.c_uint32

    def close(self):
        if getattr(self, "_h", None):
            self._L.otg_fasta_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def seqs(self):
        out = []
        for i in range(self._L.otg_fasta_n_seqs(self._h)):
            ln = C.c_int64(0)
            nm = self._L.otg_fasta_seq(self._h, C.c_uint32(i), C.byref(ln))
            out.append((nm.decode(), int(ln.value)))
        return out

    def fetch(self, chr_, beg, end_inclusive):
        c = chr_.encode()
        cap = max(16, abs(int(end_inclusive) - int(beg)) + 2)
        out = C.create_string_buffer(cap)
        n = C.c_uint64(0)
        rc = self._L.otg_fasta_fetch(self._h, C.c_char_p(c), C.c_uint32(len(c)), C.c_int32(beg), C.c_int32(end_inclusive), out,
                                     C.c_uint64(cap), C.byref(n))
        if rc != 0:
            raise OtterGpuError("otg_fasta_fetch failed (%d): %s" % (rc, _err(self._L)))
        return out.raw[:n.value]

    def region_flanks(self, beds, chr_arena, batch, flank=100, offset_l=0, offset_r=0):
        """Appends the two flanks of every region to batch["arena"] and fills the flank fields of batch["regions"] (in place)."""
        arena = batch["arena"]
        base = len(arena)
        cap = base + 2 * (int(flank) + 1) * len(beds) + 128
        big = np.zeros(cap, dtype=np.uint8)
        big[:base] = arena
        used = C.c_uint64(base)
        rc = self._L.otg_fasta_region_flanks(self._h, abi.ptr(beds), abi.ptr(chr_arena, C.c_char_p), C.c_uint32(len(beds)), C.c_int32(offset_l),
                                             C.c_int32(offset_r), C.c_int32(flank), abi.ptr(big), C.c_uint64(cap), C.byref(used),
                                             abi.ptr(batch["regions"]))
        if rc != 0:
            raise OtterGpuError("otg_fasta_region_flanks failed (%d): %s" % (rc, _err(self._L)))
        batch["arena"] = np.ascontiguousarray(big[:used.value + 64])
        return batch


def _emit(call, cap):
    L = load()
    while True:
        out = np.empty(max(cap, 16), dtype=np.uint8)
        n = C.c_uint64(0)
        rc = call(abi.ptr(out, C.c_char_p), C.c_uint64(out.size), C.byref(n))
        if rc == abi.OTG_ERR_CAPACITY:
            cap = n.value
            continue
        if rc != 0:
            raise OtterGpuError("emit failed (%d): %s" % (rc, _err(L)))
        return out[:n.value].tobytes()


def emit_vcf_header(bam):
    """The VCF header of `otter genotype -r` for an allele BAM (after Bam.sample_index())."""
    L = load()
    return _emit(lambda o, c, n: L.otg_emit_vcf_header(bam._h, o, c, n), 4096)


def emit_vcf_lines(beds, chr_arena, blk, n_samples, gt, hsd, n_gt, reps, offset_l, offset_r):
    """One VCF line per region with alleles; blk = Bam.ingest_alleles(..., reference=...), gt / hsd / n_gt / reps from
    Context.genotype_cluster_batch on the same blocks."""
    L = load()
    gt = np.ascontiguousarray(gt, dtype=np.int32); hsd = np.ascontiguousarray(hsd, dtype=np.float64)
    n_gt = np.ascontiguousarray(n_gt, dtype=np.int32); reps = np.ascontiguousarray(reps, dtype=np.int32)
    cap = int(blk["alleles"]["seq_len"].sum()) * 2 + 256 * (len(beds) + 1) * (n_samples + 2)
    return _emit(lambda o, c, n: L.otg_emit_vcf_lines(abi.ptr(beds), abi.ptr(chr_arena, C.c_char_p), C.c_uint32(len(beds)), abi.ptr(blk["first_allele"]),
                                                      abi.ptr(blk["alleles"]), abi.ptr(blk["arena"]), C.c_uint32(n_samples), abi.ptr(gt), abi.ptr(hsd),
                                                      abi.ptr(n_gt), abi.ptr(reps), C.c_int32(offset_l), C.c_int32(offset_r), o, c, n), cap)


def emit_genotype_lengths(bam, beds, chr_arena, blk, n_samples):
    """`otter genotype` without a reference: region, sample, shorter and longer allele length per line."""
    L = load()
    return _emit(lambda o, c, n: L.otg_emit_genotype_lengths(bam._h, abi.ptr(beds), abi.ptr(chr_arena, C.c_char_p), C.c_uint32(len(beds)),
                                                             abi.ptr(blk["first_allele"]), abi.ptr(blk["alleles"]), C.c_uint32(n_samples), o, c, n),
                 128 * (len(beds) + 1) * (n_samples + 1))


def genotype_blocks(blk):
    """(seq_off, seq_len, first_allele, n_alleles) arrays of an ingested allele batch, the inputs of genotype_cluster_batch."""
    a = blk["alleles"]
    first = blk["first_allele"]
    return (np.ascontiguousarray(a["seq_off"], dtype=np.uint64), np.ascontiguousarray(a["seq_len"], dtype=np.uint32),
            np.ascontiguousarray(first[:-1], dtype=np.uint32), np.ascontiguousarray(np.diff(first.astype(np.int64)), dtype=np.uint32))


class BamSink:
    """otg_bam_sink: SAM text in (write(), in arbitrary pieces), coordinate-sorted BAM + BAI out at close().  sort=False takes the text in
    coordinate order and streams it; sort=True holds the records in memory and sorts them at close.  As a context manager it closes on a
    clean exit and removes what it wrote when the block raises.  `writer` is a callable with the otg_write_fn signature for the `sink`
    parameter of _run_files_job."""

    def __init__(self, path, sort=False, threads=1, level=-1):
        L = load()
        L.otg_bam_sink_open.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.otg_bam_sink_write.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.otg_bam_sink_close.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.otg_bam_sink_abort.argtypes = [C.c_void_p]
        L.otg_bam_sink_abort.restype = None
        L.otg_bam_sink_error.argtypes = [C.c_void_p]
        L.otg_bam_sink_error.restype = C.c_char_p
        opts = (C.c_int32 * 4)(int(bool(sort)), int(threads), int(level), 0)
        h = C.c_void_p()
        rc = L.otg_bam_sink_open(path.encode(), opts, C.byref(h))
        if rc != 0:
            raise OtterGpuError("otg_bam_sink_open failed (%d): %s" % (rc, _err(L)))
        self._h, self._L, self.path, self.n_records = h, L, path, None

    @property
    def error(self):
        """the text of the sink's refusal ("" when there is none)"""
        return (self._L.otg_bam_sink_error(self._h) or b"").decode(errors="replace") if self._h else ""

    def writer(self, _user, data, n):
        return self._L.otg_bam_sink_write(self._h, data, n)

    def write(self, data):
        data = bytes(data)
        rc = self._L.otg_bam_sink_write(self._h, data, len(data))
        if rc != 0:
            raise OtterGpuError("otg_bam_sink_write failed (%d): %s" % (rc, self.error))

    def close(self):
        """finishes the BAM and its index -> the number of records; after a refusal removes both and raises"""
        if not self._h:
            return self.n_records
        n = C.c_uint64(0)
        h, self._h = self._h, None
        rc = self._L.otg_bam_sink_close(h, C.byref(n))
        if rc != 0:
            raise OtterGpuError("otg_bam_sink_close failed (%d): %s" % (rc, _err(self._L)))
        self.n_records = int(n.value)
        return self.n_records

    def abort(self):
        if self._h:
            h, self._h = self._h, None
            self._L.otg_bam_sink_abort(h)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *a):
        if exc_type is None:
            self.close()
        else:
            self.abort()

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


def merge_bams(paths, out, threads=1, level=-1):
    """otg_bam_merge: coordinate-sorted BAMs with the same targets (per-sample allele BAMs) -> one BAM + BAI; returns the number of records."""
    L = load()
    L.otg_bam_merge.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    arr = (C.c_char_p * max(1, len(paths)))(*[p.encode() for p in paths])
    n = C.c_uint64(0)
    rc = L.otg_bam_merge(arr, len(paths), out.encode(), int(threads), int(level), C.byref(n))
    if rc != 0:
        raise OtterGpuError("otg_bam_merge failed (%d): %s" % (rc, _err(L)))
    return int(n.value)


def _into_sinks(sinks, run):
    """run() with the BamSinks open: closes them when it returns, removes their files when it raises (the sink's own refusal, which the
    dispatcher only sees as a failed writer, is appended to the error)."""
    try:
        out = run()
    except OtterGpuError as e:
        why = "; ".join(x.error for x in sinks if x.error)
        for x in sinks:
            x.abort()
        raise OtterGpuError("%s%s" % (e, " [" + why + "]" if why else "")) from None
    except BaseException:
        for x in sinks:
            x.abort()
        raise
    for i, x in enumerate(sinks):
        try:
            x.close()
        except BaseException:
            for y in sinks[i + 1:]:
                y.abort()
            raise
    return out


def _run_files_job(fn_name, job, job_type, callbacks=None, sink=None):
    """One otg_*_files entry point: collects what it writes and returns (text bytes, stats dict); OtterGpuError with the library's last
    error when it fails.  callbacks: {job field: (callback type, Python callable)} for the further writers a job struct carries (set on
    the job and kept alive here).  sink: a writer to use in place of the collecting one.  tests/dispatch_exits_child.py gets its refusing
    writers in by wrapping this function (looked up as a module global by the five public functions) and passing `sink` / replacing the
    callables in `callbacks` by field name: a change of this signature or of that layout has to be made there too."""
    L = load()
    chunks = []

    def collect(_user, data, n):
        chunks.append(C.string_at(data, n))
        return 0
    cb = abi.WRITE_FN(sink or collect)
    alive = [fn_type(fn) for fn_type, fn in (callbacks or {}).values()]
    for field, c in zip(callbacks or {}, alive):
        setattr(job, field, C.cast(c, C.c_void_p))
    st = abi.JobStats()
    fn = getattr(L, fn_name)
    fn.argtypes = [C.POINTER(job_type), abi.WRITE_FN, C.c_void_p, C.POINTER(abi.JobStats)]
    rc = fn(C.byref(job), cb, None, C.byref(st))
    if rc != 0:
        raise OtterGpuError("%s failed (%d): %s" % (fn_name, rc, _err(L)))
    return b"".join(chunks), {k: getattr(st, k) for k, _ in abi.JobStats._fields_}


def assemble_files(bam, bed, fasta=None, read_group="", is_fasta=False, reads_only=False, params=None, batch_regions=0, devices=None,
                   offset_l=1, offset_r=0, mapq=0, nonprimary=False, omit_nonspanning=False, read_quality=0.0, threads=1, *, bam_out=None, sort=False, bam_threads=None):
    """otg_assemble_files: `otter assemble` from files to record text (the library's dispatcher, include/otter_gpu.h).
    Returns (text bytes, stats dict).  bam_out: the SAM records go into that BAM (+ .bai) through a BamSink instead (text bytes = b"");
    sort=True for a BED that is not in coordinate order; bam_threads: the sink's deflate threads (default: `threads`)."""
    if bam_out is not None and is_fasta:
        raise OtterGpuError("assemble_files: bam_out takes SAM records, not is_fasta")
    job = abi.AssembleJob()
    job.bam_path = bam.encode(); job.bed_path = bed.encode(); job.fasta_path = fasta.encode() if fasta else None
    job.read_group = read_group.encode(); job.is_fasta = int(is_fasta); job.reads_only = int(reads_only)
    job.params = params if params is not None else abi.default_params()
    job.ingest = abi.IngestOpts(offset_l, offset_r, mapq, int(nonprimary), int(omit_nonspanning), threads, read_quality)
    job.batch_regions = batch_regions
    devs = (C.c_int32 * len(devices))(*devices) if devices else None
    job.n_devices = len(devices) if devices else 0
    job.devices = devs
    if bam_out is None:
        return _run_files_job("otg_assemble_files", job, abi.AssembleJob)
    bs = BamSink(bam_out, sort=sort, threads=threads if bam_threads is None else bam_threads)
    return _into_sinks([bs], lambda: _run_files_job("otg_assemble_files", job, abi.AssembleJob, None, bs.writer))


def spread_files(bam, bed, fasta=None, params=None, batch_regions=0, devices=None, offset_l=1, offset_r=0, mapq=0, nonprimary=False, omit_nonspanning=False,
                 read_quality=0.0, threads=1, match=2, mismatch=7, indel=7, min_score=24):
    """otg_spread_files: the spread from files to rows (include/otter_gpu.h): the batch loop of assemble_files over a catalogue BED (units in
    column 4), the spread of every batch right behind its run, one spread_emit row per consensus allele in BED order.  Returns (text bytes,
    stats dict)."""
    job = abi.SpreadJob()
    a = job.assemble
    a.bam_path = bam.encode(); a.bed_path = bed.encode(); a.fasta_path = fasta.encode() if fasta else None
    a.read_group = b""; a.is_fasta = 0; a.reads_only = 0
    a.params = params if params is not None else abi.default_params()
    a.ingest = abi.IngestOpts(offset_l, offset_r, mapq, int(nonprimary), int(omit_nonspanning), threads, read_quality)
    a.batch_regions = batch_regions
    devs = (C.c_int32 * len(devices))(*devices) if devices else None
    a.n_devices = len(devices) if devices else 0
    a.devices = devs
    job.match, job.mismatch, job.indel, job.min_score = match, mismatch, indel, min_score
    return _run_files_job("otg_spread_files", job, abi.SpreadJob)


def assemble_batch_plan(n_regions, batch_regions=0):
    """Batch sizes otg_assemble_files cuts a shard of n_regions into (otg_assemble_batch_plan)."""
    L = load()
    L.otg_assemble_batch_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    n = C.c_uint32(0)
    rc = L.otg_assemble_batch_plan(n_regions, batch_regions, None, 0, C.byref(n))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_assemble_batch_plan failed (%d)" % rc)
    out = (C.c_uint32 * max(1, n.value))()
    rc = L.otg_assemble_batch_plan(n_regions, batch_regions, out, n.value, C.byref(n))
    if rc != 0:
        raise OtterGpuError("otg_assemble_batch_plan failed (%d)" % rc)
    return [int(out[i]) for i in range(n.value)]


def genotype_files(bam, bed, fasta=None, params=None, threads=1, device=0, batch_regions=0, metric="length"):
    """otg_genotype_files: `otter genotype` from files to text (VCF with a reference FASTA, the two-length table without).
    metric: "length" (the reference) or "edit" (alleles clustered by exact edit distance).  Returns (text bytes, stats dict)."""
    job = abi.GenotypeJob()
    job.metric = abi.gt_metric(metric)
    job.bam_path = bam.encode(); job.bed_path = bed.encode(); job.fasta_path = fasta.encode() if fasta else None
    job.params = params if params is not None else abi.default_params()
    job.threads = threads; job.device = device; job.batch_regions = batch_regions
    return _run_files_job("otg_genotype_files", job, abi.GenotypeJob)


def cohort_files(bams, names, bed, fasta, params=None, batch_regions=0, devices=None, offset_l=1, offset_r=0, mapq=0, nonprimary=False,
                 omit_nonspanning=False, read_quality=0.0, threads=1, alleles=False, *, alleles_bam=None, matrix_k=None, gt_metric="length"):
    """otg_cohort_files: sample BAMs + BED + reference FASTA to one joint VCF, the alleles staying on the device between `otter assemble` and
    `otter genotype`.  Returns (VCF bytes, stats dict), and with alleles=True also the list of per-sample SAM texts (what assemble_files returns
    for each sample with read_group = its name).  alleles_bam: a list of paths, one per sample: the same records as BAM + BAI files.
    matrix_k: also the k-mer usage matrix of the joint alleles at that k (the text vcf2mat_files returns for the VCF), computed while the
    alleles are in HBM and appended to the returned tuple as its last element.  gt_metric: "length" or "edit", as genotype_files' metric."""
    if alleles_bam is not None and len(alleles_bam) != len(bams):
        raise OtterGpuError("cohort_files: alleles_bam has %d paths for %d samples" % (len(alleles_bam), len(bams)))
    job = abi.CohortJob()
    n = len(bams)
    pb = (C.c_char_p * max(1, n))(*[b.encode() for b in bams])
    pn = (C.c_char_p * max(1, n))(*[x.encode() for x in names])
    job.n_samples = n; job.batch_regions = batch_regions; job.gt_metric = abi.gt_metric(gt_metric)
    job.bam_paths = pb; job.sample_names = pn
    job.bed_path = bed.encode(); job.fasta_path = fasta.encode() if fasta else None
    job.params = params if params is not None else abi.default_params()
    job.ingest = abi.IngestOpts(offset_l, offset_r, mapq, int(nonprimary), int(omit_nonspanning), threads, read_quality)
    devs = (C.c_int32 * len(devices))(*devices) if devices else None
    job.n_devices = len(devices) if devices else 0
    job.devices = devs
    sams = [[] for _ in range(n)]

    sinks = [BamSink(p, threads=threads) for p in alleles_bam] if alleles_bam is not None else []

    def asink(_user, sample, data, ln):
        if alleles:
            sams[sample].append(C.string_at(data, ln))
        return sinks[sample].writer(None, data, ln) if sinks else 0
    mat = []

    def msink(_user, data, ln):
        mat.append(C.string_at(data, ln))
        return 0
    callbacks = {}
    if alleles or sinks:
        callbacks["allele_write"] = (abi.ALLELE_WRITE_FN, asink)
    if matrix_k is not None:
        job.matrix_k = int(matrix_k)
        callbacks["matrix_write"] = (abi.WRITE_FN, msink)
    text, stats = _into_sinks(sinks, lambda: _run_files_job("otg_cohort_files", job, abi.CohortJob, callbacks or None))
    out = (text, stats) + (([b"".join(x) for x in sams],) if alleles else ())
    return out + ((b"".join(mat),) if matrix_k is not None else ())


def assemble_files_release():
    """Frees the contexts (and their HBM workspaces) the dispatcher keeps for the next job of the process (otg_assemble_files_release)."""
    load().otg_assemble_files_release()


def wgat(bam, regions, read_group="", fasta=False, offset_l=1, offset_r=0, *, bam_out=None):
    """otg_wgat: `otter wgat` on an open Bam handle; regions = list of (chr, start, end) or the (beds, chr_arena) pair.  Returns the text and
    the number of records.  bam_out: the SAM records go into that BAM (+ .bai) instead, sorted by the sink (text = b"")."""
    L = load()
    beds, carena = regions if isinstance(regions, tuple) else abi.make_beds(regions)
    chunks = []
    if bam_out is not None and fasta:
        raise OtterGpuError("wgat: bam_out takes SAM records, not fasta")
    bs = BamSink(bam_out, sort=True) if bam_out is not None else None

    def sink(_user, data, n):
        chunks.append(C.string_at(data, n))
        return 0
    cb = abi.WRITE_FN(bs.writer if bs else sink)
    nrec = C.c_uint64(0)
    L.otg_wgat.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int32, C.c_int32, abi.WRITE_FN, C.c_void_p, C.POINTER(C.c_uint64)]
    rc = L.otg_wgat(bam._h, abi.ptr(beds), abi.ptr(carena, C.c_char_p), C.c_uint32(len(beds)), read_group.encode(), int(fasta), offset_l, offset_r, cb, None, C.byref(nrec))
    if rc != 0:
        why = bs.error if bs else ""
        if bs:
            bs.abort()
        raise OtterGpuError("otg_wgat failed (%d): %s%s" % (rc, _err(L), " [" + why + "]" if why else ""))
    if bs:
        bs.close()
    return b"".join(chunks), int(nrec.value)


def compare_emit(regions, truth, query, pair_first, pair_edit, pair_ops):
    """otg_compare_emit: the region logic of `otter compare` on ingested alleles (dicts of Bam.ingest_compare) and per-pair (edit, ops)
    -> (text bytes, warning bytes, counts dict)."""
    L = load()
    beds, carena = regions if isinstance(regions, tuple) else abi.make_beds(regions)
    pair_first = np.ascontiguousarray(pair_first, dtype=np.uint64)
    pe = np.ascontiguousarray(pair_edit, dtype=np.float64)
    po = np.ascontiguousarray(pair_ops, dtype=np.float64)
    if pe.size == 0:
        pe, po = np.zeros(1), np.zeros(1)
    sp = truth["spannings"] if truth["spannings"].size else np.zeros(1, np.int32)
    cnt = abi.CompareCounts()
    need, wneed = C.c_uint64(0), C.c_uint64(0)
    args = lambda out, cap, w, wcap: (abi.ptr(beds), abi.ptr(carena, C.c_char_p), C.c_uint32(len(beds)),
                                      abi.ptr(truth["first_allele"]), abi.ptr(truth["alleles"]), abi.ptr(truth["arena"]),
                                      abi.ptr(truth["first_spanning"]), abi.ptr(sp),
                                      abi.ptr(query["first_allele"]), abi.ptr(query["alleles"]), abi.ptr(query["arena"]),
                                      abi.ptr(pair_first), abi.ptr(pe), abi.ptr(po), out, C.c_uint64(cap), C.byref(need), w, C.c_uint64(wcap),
                                      C.byref(wneed), C.byref(cnt))
    rc = L.otg_compare_emit(*args(None, 0, None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_compare_emit failed (%d): %s" % (rc, (L.otg_last_error(None) or b"").decode()))
    out = C.create_string_buffer(need.value + 1)
    w = C.create_string_buffer(wneed.value + 1)
    rc = L.otg_compare_emit(*args(out, need.value, w, wneed.value))
    if rc != 0:
        raise OtterGpuError("otg_compare_emit failed (%d): %s" % (rc, (L.otg_last_error(None) or b"").decode()))
    return out.raw[:need.value], w.raw[:wneed.value], {k: getattr(cnt, k) for k, _ in abi.CompareCounts._fields_}


def compare_files(truth_bam, query_bam, bed, threads=1, device=0, batch_regions=0, heuristic=None):
    """otg_compare_files: `otter compare` from files to text.  heuristic: None = exact edit alignments, or the (min_wavefront_length,
    max_distance_threshold, steps_between_cutoffs) of wfadaptive.  Returns (text bytes, warning bytes, stats dict)."""
    job = abi.CompareJob()
    job.truth_bam_path = truth_bam.encode(); job.query_bam_path = query_bam.encode(); job.bed_path = bed.encode()
    job.threads = threads; job.device = device; job.batch_regions = batch_regions
    if heuristic is not None:
        job.heuristic = abi.OTG_HEURISTIC_WFADAPTIVE
        job.heur_min_wavefront_length, job.heur_max_distance_threshold, job.heur_steps_between_cutoffs = (int(x) for x in heuristic)
    warns = []

    def wsink(_user, data, n):
        warns.append(C.string_at(data, n))
        return 0
    text, stats = _run_files_job("otg_compare_files", job, abi.CompareJob, {"warn": (abi.WRITE_FN, wsink)})
    return text, b"".join(warns), stats


def vcf_read_alleles(path, max_alleles=1 << 16, max_bytes=64 << 20):
    """otg_vcf_read_alleles over a whole VCF (batches of at most max_alleles alleles / max_bytes sequence bytes) ->
    {"records": vcf_record_dt array, "regions": bytes, "seq_off", "seq_len", "arena": uint8 array, "bytes_in", "batches"}; the records of
    later batches are rebased onto the concatenated arrays."""
    L = load()
    L.otg_vcf_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.otg_vcf_close.argtypes = [C.c_void_p]
    h = C.c_void_p()
    if L.otg_vcf_open(path.encode(), C.byref(h)) != 0:
        raise OtterGpuError("otg_vcf_open failed: %s" % _err(L))
    recs, regs, offs, lens, arenas = [], [], [], [], []
    base_r, base_a, base_s, batches = 0, 0, 0, 0
    bytes_in = C.c_uint64(0)
    cap_r, cap_a, cap_s, cap_g = max_alleles, max_alleles, max_bytes, 1 << 20
    try:
        while True:
            rec = np.zeros(cap_r, dtype=abi.vcf_record_dt)
            reg = np.zeros(cap_g, dtype=np.uint8)
            off = np.zeros(cap_a, dtype=np.uint64)
            ln = np.zeros(cap_a, dtype=np.uint32)
            ar = np.zeros(cap_s, dtype=np.uint8)
            nr, ru, na, au = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
            rc = L.otg_vcf_read_alleles(h, abi.ptr(rec), C.c_uint32(cap_r), C.byref(nr), abi.ptr(reg), C.c_uint64(cap_g), C.byref(ru),
                                        abi.ptr(off), abi.ptr(ln), C.c_uint32(cap_a), C.byref(na), abi.ptr(ar), C.c_uint64(cap_s), C.byref(au),
                                        C.byref(bytes_in))
            if rc == abi.OTG_ERR_CAPACITY:
                cap_a, cap_r = max(cap_a, na.value), max(cap_r, 1)
                cap_g, cap_s = max(cap_g, ru.value), max(cap_s, au.value)
                continue
            if rc != 0:
                raise OtterGpuError("otg_vcf_read_alleles failed (%d): %s" % (rc, _err(L)))
            if nr.value == 0:
                break
            batches += 1
            r = rec[:nr.value].copy()
            r["region_off"] += base_r
            r["first_allele"] += base_a
            recs.append(r); regs.append(reg[:ru.value].tobytes())
            offs.append(off[:na.value] + np.uint64(base_s)); lens.append(ln[:na.value].copy()); arenas.append(ar[:au.value].copy())
            base_r += ru.value; base_a += na.value; base_s += au.value
    finally:
        L.otg_vcf_close(h)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    return {"records": cat(recs, abi.vcf_record_dt), "regions": b"".join(regs), "seq_off": cat(offs, np.uint64), "seq_len": cat(lens, np.uint32),
            "arena": cat(arenas, np.uint8), "bytes_in": int(bytes_in.value), "batches": batches}


def vcf2mat_emit(records, regions, seq_len, k, usage, gc, hsd):
    """otg_vcf2mat_emit: the rows of vcf2mat for the records (vcf_record_dt) and per-allele values -> text bytes."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    usage = np.ascontiguousarray(usage, dtype=np.float64)
    gc = np.ascontiguousarray(gc, dtype=np.float64)
    hsd = np.ascontiguousarray(hsd, dtype=np.float64)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(seq_len), C.c_int32(k), abi.ptr(usage),
                             abi.ptr(gc), abi.ptr(hsd), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_vcf2mat_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_vcf2mat_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_vcf2mat_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_vcf2mat_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def vcf2mat_files(vcf, bed, k=3, threads=1, device=0, batch_alleles=0):
    """otg_vcf2mat_files: `otter vcf2mat` from a VCF (plain, gzip or BGZF) to text.  Returns (text bytes, stats dict)."""
    job = abi.Vcf2matJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.k = k; job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    return _run_files_job("otg_vcf2mat_files", job, abi.Vcf2matJob)


def motif_emit(records, regions, seq_len, motifs, units):
    """otg_motif_emit: the rows of otter_motifs for the records (vcf_record_dt), per-allele motif records (motif_dt) and units [n, stride] -> text bytes."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    motifs = np.ascontiguousarray(motifs, dtype=abi.motif_dt)
    units = np.ascontiguousarray(units, dtype=np.uint8)
    stride = units.shape[1] if units.ndim == 2 else 0
    if units.size == 0:
        units = np.zeros(1, dtype=np.uint8)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(seq_len), abi.ptr(motifs), abi.ptr(units),
                             C.c_uint32(stride), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_motif_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_motif_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_motif_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_motif_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def motifs_files(vcf, bed, max_period=256, slack=50, threads=1, device=0, batch_alleles=0):
    """otg_motifs_files: the motif annotation of every allele of a VCF (plain, gzip or BGZF) as text.  Returns (text bytes, stats dict)."""
    job = abi.MotifsJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.max_period = max_period; job.slack = slack; job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    return _run_files_job("otg_motifs_files", job, abi.MotifsJob)


def repeat_emit(records, regions, arena, seq_off, seq_len, sums, seg_off, segs):
    """otg_repeat_emit: the rows of otter_repeats for the records (vcf_record_dt), the alleles (arena, seq_off, seq_len) and their structure as
    Context.repeat_batch returns it -> text bytes."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    sums = np.ascontiguousarray(sums, dtype=abi.repeat_sum_dt)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
    segs = np.ascontiguousarray(segs, dtype=abi.repeat_seg_dt)
    if arena.size == 0:
        arena = np.zeros(1, dtype=np.uint8)
    if segs.size == 0:
        segs = np.zeros(1, dtype=abi.repeat_seg_dt)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(arena), abi.ptr(seq_off), abi.ptr(seq_len), abi.ptr(sums),
                             abi.ptr(seg_off), abi.ptr(segs), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_repeat_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_repeat_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_repeat_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_repeat_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def repeats_files(vcf, bed, max_period=256, min_copies=2, min_span=12, threads=1, device=0, batch_alleles=0):
    """otg_repeats_files: the repeat structure of every allele of a VCF (plain, gzip or BGZF) as text.  Returns (text bytes, stats dict)."""
    job = abi.RepeatsJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.max_period = max_period; job.min_copies = min_copies; job.min_span = min_span
    job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    return _run_files_job("otg_repeats_files", job, abi.RepeatsJob)


_SEG_TYPES = {"repeat": (abi.repeat_sum_dt, abi.repeat_seg_dt), "unitparse": (abi.unitparse_sum_dt, abi.unitparse_seg_dt),
              "locus": (abi.locus_dt, abi.unitparse_seg_dt)}


def _rows(arena, seq_off, seq_len):
    """an operator's rows -> (the five leading arguments of its *_batch entry: arena, its bytes, offsets, lengths, their number; the lengths
    as a uint32 array)"""
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    ln = np.ascontiguousarray(seq_len, dtype=np.uint32)
    return _Kept((abi.ptr(arena), C.c_uint64(arena.size), abi.ptr(off), abi.ptr(ln), C.c_uint32(len(ln))), (arena, off, ln)), ln


def _pack_units(units):
    """a list of byte strings as (arena uint8 (never empty), offsets uint64, lengths uint32)"""
    units = [bytes(u) for u in units]
    ulen = np.array([len(u) for u in units], dtype=np.uint32)
    uoff = (np.cumsum(ulen, dtype=np.uint64) - ulen).astype(np.uint64)
    return np.frombuffer(b"".join(units) + b"\0", dtype=np.uint8).copy(), uoff, ulen


def _pack_unit_sets(unit_sets, task_seq, task_set):
    """a list of unit sets (lists of byte strings) and the task lists as the arguments of otg_unitparse_batch between the alleles and the tasks"""
    unit_sets = [[bytes(u) for u in s] for s in unit_sets]
    uarena, uoff, ulen = _pack_units([u for s in unit_sets for u in s])
    first = np.concatenate(([0], np.cumsum([len(s) for s in unit_sets], dtype=np.uint64))).astype(np.uint64)
    ts = np.ascontiguousarray(task_seq, dtype=np.uint32)
    tq = np.ascontiguousarray(task_set, dtype=np.uint32)
    if len(ts) != len(tq):
        raise ValueError("task_seq and task_set differ in length")
    keep = (uarena, uoff, ulen, first)
    args = (abi.ptr(uarena), C.c_uint64(int(ulen.sum())), abi.ptr(uoff), abi.ptr(ulen), C.c_uint32(len(ulen)), abi.ptr(first), C.c_uint32(len(unit_sets)))
    return _Kept(args, keep), ts, tq


class _Kept(tuple):
    """ctypes arguments that keep the arrays they point into alive"""

    def __new__(cls, args, keep):
        self = super().__new__(cls, args)
        self.keep = keep
        return self


def parse_bed_units(path):
    """otg_parse_bed_units: the repeat units of a tandem-repeat catalogue -> one list of byte strings per BED record (the records of
    parse_bed_file, in its order); empty where column 4 is missing or a name."""
    L = load()
    cap_r, cap_u, cap_a = 1024, 1024, 1 << 14
    while True:
        first = np.zeros(cap_r + 1, dtype=np.uint64)
        uoff, ulen, arena = np.zeros(cap_u, dtype=np.uint64), np.zeros(cap_u, dtype=np.uint32), np.zeros(cap_a, dtype=np.uint8)
        nr, nu, ab = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = L.otg_parse_bed_units(C.c_char_p(path.encode()), abi.ptr(first), C.c_uint64(cap_r + 1), C.byref(nr), abi.ptr(uoff), abi.ptr(ulen), C.c_uint64(cap_u),
                                   C.byref(nu), abi.ptr(arena), C.c_uint64(cap_a), C.byref(ab))
        if rc == abi.OTG_ERR_CAPACITY:
            cap_r, cap_u, cap_a = max(cap_r, nr.value), max(cap_u, nu.value), max(cap_a, ab.value)
            continue
        if rc != 0:
            raise OtterGpuError("otg_parse_bed_units failed (%d): %s" % (rc, _err(L)))
        raw = arena.tobytes()
        return [[raw[int(uoff[k]):int(uoff[k]) + int(ulen[k])] for k in range(int(first[r]), int(first[r + 1]))] for r in range(nr.value)]


def unitalign_emit(records, regions, seq_len, task_first, task_source, units, aligned):
    """otg_unitalign_emit: the rows of otter_copies for the records (vcf_record_dt): the tasks of allele a are task_first[a] .. task_first[a + 1],
    task t has source task_source[t] (abi.UNITALIGN_SOURCE_*), the unit units[t] (bytes, b"" for none) and the record aligned[t]
    (unitalign_dt) -> text bytes."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    task_first = np.ascontiguousarray(task_first, dtype=np.uint64)
    task_source = np.ascontiguousarray(task_source, dtype=np.uint8)
    aligned = np.ascontiguousarray(aligned, dtype=abi.unitalign_dt)
    uarena, uoff, ulen = _pack_units(units)
    if aligned.size == 0:
        aligned, task_source, uoff, ulen = np.zeros(1, dtype=abi.unitalign_dt), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(seq_len), abi.ptr(task_first), abi.ptr(task_source), abi.ptr(uarena),
                             abi.ptr(uoff), abi.ptr(ulen), abi.ptr(aligned), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_unitalign_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_unitalign_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_unitalign_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_unitalign_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def unitparse_emit(records, regions, seq_len, allele_sets, unit_sets, sums, seg_off, segs):
    """otg_unitparse_emit: the rows of otter_unitparse for the records (vcf_record_dt): allele a has the unit set unit_sets[allele_sets[a]] (None or
    abi.UNITPARSE_NO_SET: none), the summary sums[a] and the segments segs[seg_off[a]:seg_off[a + 1]] -> text bytes."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    aset = np.ascontiguousarray([abi.UNITPARSE_NO_SET if q is None else q for q in allele_sets] + [abi.UNITPARSE_NO_SET], dtype=np.uint32)
    sets, _, _ = _pack_unit_sets(unit_sets, [], [])
    sums = np.ascontiguousarray(sums, dtype=abi.unitparse_sum_dt)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
    segs = np.ascontiguousarray(segs, dtype=abi.unitparse_seg_dt)
    if sums.size == 0:
        sums = np.zeros(1, dtype=abi.unitparse_sum_dt)
    if segs.size == 0:
        segs = np.zeros(1, dtype=abi.unitparse_seg_dt)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(seq_len), abi.ptr(aset), sets[5], sets[0], sets[2], sets[3],
                             abi.ptr(sums), abi.ptr(seg_off), abi.ptr(segs), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_unitparse_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_unitparse_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_unitparse_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_unitparse_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def unitparse_files(vcf, bed, threads=1, device=0, batch_alleles=0):
    """otg_unitparse_files: every allele of a VCF (plain, gzip or BGZF) parsed against the unit set its region has in a tandem-repeat catalogue,
    as text.  Returns (text bytes, stats dict)."""
    job = abi.UnitparseJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    return _run_files_job("otg_unitparse_files", job, abi.UnitparseJob)


def copies_files(vcf, bed, max_period=256, slack=50, threads=1, device=0, batch_alleles=0):
    """otg_copies_files: the copy numbers of every allele of a VCF (plain, gzip or BGZF) against the units of a tandem-repeat catalogue, or
    against the allele's own motif-annotation unit where the catalogue gives none, as text.  Returns (text bytes, stats dict)."""
    job = abi.CopiesJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.max_period = max_period; job.slack = slack; job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    return _run_files_job("otg_copies_files", job, abi.CopiesJob)


def tract_emit(records, regions, seq_len, task_first, task_source, units, tracts):
    """otg_tract_emit: the rows of otter_tracts for the records (vcf_record_dt), arguments as unitalign_emit with tracts[t] (tract_dt) the record
    of task t -> text bytes."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    task_first = np.ascontiguousarray(task_first, dtype=np.uint64)
    task_source = np.ascontiguousarray(task_source, dtype=np.uint8)
    tracts = np.ascontiguousarray(tracts, dtype=abi.tract_dt)
    uarena, uoff, ulen = _pack_units(units)
    if tracts.size == 0:
        tracts, task_source, uoff, ulen = np.zeros(1, dtype=abi.tract_dt), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(seq_len), abi.ptr(task_first), abi.ptr(task_source), abi.ptr(uarena),
                             abi.ptr(uoff), abi.ptr(ulen), abi.ptr(tracts), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_tract_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_tract_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_tract_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_tract_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def tracts_files(vcf, bed, max_period=256, slack=50, match=2, mismatch=7, indel=7, min_score=24, threads=1, device=0, batch_alleles=0):
    """otg_tracts_files: the repeat tract inside every allele of a VCF (plain, gzip or BGZF) against the units of a tandem-repeat catalogue, or
    against the allele's own motif-annotation unit where the catalogue gives none, as text.  Returns (text bytes, stats dict)."""
    job = abi.TractsJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.max_period = max_period; job.slack = slack; job.match = match; job.mismatch = mismatch; job.indel = indel; job.min_score = min_score
    job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    return _run_files_job("otg_tracts_files", job, abi.TractsJob)


def locus_emit(records, regions, seq_len, allele_sets, unit_sets, loci, seg_off, segs):
    """otg_locus_emit: the rows of otter_loci for the records (vcf_record_dt), arguments as unitparse_emit with loci[a] (locus_dt) the record of
    allele a and its segments in allele positions -> text bytes."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    aset = np.ascontiguousarray([abi.UNITPARSE_NO_SET if q is None else q for q in allele_sets] + [abi.UNITPARSE_NO_SET], dtype=np.uint32)
    sets, _, _ = _pack_unit_sets(unit_sets, [], [])
    loci = np.ascontiguousarray(loci, dtype=abi.locus_dt)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
    segs = np.ascontiguousarray(segs, dtype=abi.unitparse_seg_dt)
    if loci.size == 0:
        loci = np.zeros(1, dtype=abi.locus_dt)
    if segs.size == 0:
        segs = np.zeros(1, dtype=abi.unitparse_seg_dt)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(seq_len), abi.ptr(aset), sets[5], sets[0], sets[2], sets[3],
                             abi.ptr(loci), abi.ptr(seg_off), abi.ptr(segs), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_locus_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_locus_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_locus_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_locus_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def spread_emit(beds, chr_arena, res, region_set, unit_sets, records, unit_off, unit_records):
    """otg_spread_emit: one row per consensus allele of a collected batch (res: Context.assemble_collect; beds, chr_arena: abi.make_beds) from
    the results of Context.assemble_spread with the same unit_sets and region_set -> text bytes."""
    L = load()
    sets, _, _ = _pack_unit_sets(unit_sets, [], [])
    rs = np.ascontiguousarray([abi.SPREAD_NONE if q is None else q for q in region_set] + [abi.SPREAD_NONE], dtype=np.uint32)
    records = np.ascontiguousarray(records, dtype=abi.spread_dt)
    unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
    unit_records = np.ascontiguousarray(unit_records, dtype=abi.spread_unit_dt)
    if records.size == 0:
        records = np.zeros(1, dtype=abi.spread_dt)
    if unit_records.size == 0:
        unit_records = np.zeros(1, dtype=abi.spread_unit_dt)
    alleles = res["alleles"] if len(res["alleles"]) else np.zeros(1, dtype=abi.allele_dt)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(beds), abi.ptr(chr_arena, C.c_char_p), C.c_uint32(len(res["regions"])), abi.ptr(res["regions"]), abi.ptr(alleles), abi.ptr(rs),
                             sets[5], sets[0], sets[2], sets[3], abi.ptr(records), abi.ptr(unit_off), abi.ptr(unit_records), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_spread_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_spread_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_spread_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_spread_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def loci_files(vcf, bed, match=2, mismatch=7, indel=7, min_score=24, threads=1, device=0, batch_alleles=0, discover=False, max_period=256, min_copies=2,
               min_span=12, min_bases=12, min_share=50, redundant=100):
    """otg_loci_files: the joint parse of the repeat inside every allele of a VCF (plain, gzip or BGZF) against the unit set its region has in a
    tandem-repeat catalogue, as text.  Returns (text bytes, stats dict).  discover=True (otg_units_loci_files): a region without units in the
    catalogue gets the set discovered from its alleles (the last six parameters, as units_files takes them)."""
    job = abi.LociJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.match = match; job.mismatch = mismatch; job.indel = indel; job.min_score = min_score
    job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    if not discover:
        return _run_files_job("otg_loci_files", job, abi.LociJob)
    dj = abi.UnitsJob()
    dj.max_period = max_period; dj.min_copies = min_copies; dj.min_span = min_span
    dj.min_bases = min_bases; dj.min_share = min_share; dj.redundant = redundant
    L = load()
    chunks = []

    def collect(_user, data, n):
        chunks.append(C.string_at(data, n))
        return 0
    cb = abi.WRITE_FN(collect)
    st = abi.JobStats()
    L.otg_units_loci_files.argtypes = [C.POINTER(abi.LociJob), C.POINTER(abi.UnitsJob), abi.WRITE_FN, C.c_void_p, C.POINTER(abi.JobStats)]
    rc = L.otg_units_loci_files(C.byref(job), C.byref(dj), cb, None, C.byref(st))
    if rc != 0:
        raise OtterGpuError("otg_units_loci_files failed (%d): %s" % (rc, _err(L)))
    return b"".join(chunks), {k: getattr(st, k) for k, _ in abi.JobStats._fields_}


def unitset_emit(records, regions, beds, sets, units):
    """otg_unitset_emit: one catalogue line per VCF record (vcf_record_dt; record r is group r of the discovery) -> text bytes.  beds = a list
    of (chrom bytes, start, end); sets (unitset_dt) and units (per group the list of (unit bytes, weight, segments, length)) as
    Context.unitset_repeats returns them."""
    L = load()
    records = np.ascontiguousarray(records, dtype=abi.vcf_record_dt)
    sets = np.ascontiguousarray(sets, dtype=abi.unitset_dt)
    bed = np.zeros(max(len(beds), 1), dtype=abi.bed_dt)
    chroms = b""
    for i, (c, s, e) in enumerate(beds):
        bed[i] = (len(chroms), len(c), s, e, 0)
        chroms += c
    chr_arena = np.frombuffer(chroms + b"\0", dtype=np.uint8)
    flat = [u for g in units for u in g]
    set_first = np.zeros(len(units) + 1, dtype=np.uint64)
    set_first[1:] = np.cumsum([len(g) for g in units])
    rec = np.zeros(max(len(flat), 1), dtype=abi.unitset_unit_dt)
    for k, u in enumerate(flat):
        rec[k] = (u[1], u[2], u[3])
    uarena, uoff, ulen = _pack_units([u[0] for u in flat])
    if not flat:
        uoff, ulen = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    reg = np.frombuffer(regions + b"\0", dtype=np.uint8)
    need = C.c_uint64(0)
    args = lambda out, cap: (abi.ptr(records), C.c_uint32(len(records)), abi.ptr(reg), abi.ptr(bed), abi.ptr(chr_arena), C.c_uint32(len(beds)), abi.ptr(sets),
                             abi.ptr(set_first), abi.ptr(rec), abi.ptr(uarena), abi.ptr(uoff), abi.ptr(ulen), out, C.c_uint64(cap), C.byref(need))
    rc = L.otg_unitset_emit(*args(None, 0))
    if rc not in (0, abi.OTG_ERR_CAPACITY):
        raise OtterGpuError("otg_unitset_emit failed (%d): %s" % (rc, _err(L)))
    out = C.create_string_buffer(need.value + 1)
    rc = L.otg_unitset_emit(*args(out, need.value))
    if rc != 0:
        raise OtterGpuError("otg_unitset_emit failed (%d): %s" % (rc, _err(L)))
    return out.raw[:need.value]


def units_files(vcf, bed, max_period=256, min_copies=2, min_span=12, min_bases=12, min_share=50, redundant=100, threads=1, device=0, batch_alleles=0):
    """otg_units_files: the unit set of every region of a VCF (plain, gzip or BGZF), discovered from the repeat structure of its alleles, as a
    catalogue BED (columns 1-3 from `bed`).  Returns (text bytes, stats dict)."""
    job = abi.UnitsJob()
    job.vcf_path = vcf.encode(); job.bed_path = bed.encode()
    job.max_period = max_period; job.min_copies = min_copies; job.min_span = min_span
    job.min_bases = min_bases; job.min_share = min_share; job.redundant = redundant
    job.threads = threads; job.device = device; job.batch_alleles = batch_alleles
    return _run_files_job("otg_units_files", job, abi.UnitsJob)

/*
 * otter_gpu.h — C-ABI of the MI355X-native drop-in for otter's per-region hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers + sizes, and replaces a named
 * interface of the reference (holstegelab/otter @ 2024_10_08, paths relative to the
 * reference root).  The library behind it (libotter_gpu.so) is hand-written HIP for gfx950;
 * there is NO CPU fallback inside: when no HIP device is usable every call returns
 * OTG_ERR_NO_DEVICE and otg_last_error() says why.
 *
 * Layers
 *   L1  batched aligners        — replace wfa::WFAligner (WFA2-lib, absent submodule) as used at
 *                                 src/analignments.cpp:25,31,37,70-71,88-97,268-280
 *   L2  per-region operators    — replace DistMatrix/otter_hclust/PPOA/anallele_cluster
 *                                 (src/andistmat.cpp, src/otterclust.cpp:20-320,463-527, src/anppoa.hpp)
 *   L3  region-batch pipeline   — replaces the five calls inside the region loop of
 *                                 assemble_process (src/assemble.cpp:74,126,129,137,141)
 *
 * Ownership: the caller owns every input buffer until the call returns (the library copies
 * to HBM); output buffers are caller-allocated.  No C++ types or exceptions cross the ABI.
 * Threading: an otg_ctx is single-threaded (one per host worker / GPU); distinct contexts are
 * independent.  Results are independent of batch composition.
 */
#ifndef OTTER_GPU_H
#define OTTER_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status codes */
#define OTG_OK               0
#define OTG_ERR_NO_DEVICE   -1   /* no usable HIP device / kernels missing                 */
#define OTG_ERR_ARG         -2   /* bad argument (null pointer, inconsistent sizes)        */
#define OTG_ERR_HIP         -3   /* a HIP runtime call failed (message in otg_last_error)  */
#define OTG_ERR_CAPACITY    -4   /* caller-provided output buffer too small                */
#define OTG_ERR_FATAL       -5   /* a condition on which the reference exit(1)s            */

/* per-region status, mirrors the reference's warnings / omissions (src/assemble.cpp:71,94,120) */
#define OTG_REGION_OK            0
#define OTG_REGION_SKIP_MAXCOV   1   /* reads > max_cov: "[WARNING] Skipping region with abnormal coverage" */
#define OTG_REGION_NO_SPANNING   2   /* "[WARNING] No spanning reads"                                         */
#define OTG_REGION_EMPTY         3   /* no reads at all                                                       */
#define OTG_REGION_HAP_CONFLICT  4   /* "ERROR: conflicting haplotag information" (reference exit(1)s)       */
#define OTG_REGION_ALIGN_CAPACITY 5  /* a gap-affine alignment of this region outgrew the device workspaces: no records for THIS region, the rest of
                                        the batch is unaffected (the reference has no length cap, src/assemble.cpp:51-154; here the last-resort tier
                                        holds one provenance byte per wavefront cell and its slab is a share of the device's memory)             */

typedef struct otg_ctx otg_ctx;

/* ---------------------------------------------------------------- parameters
 * Defaults = reference CLI defaults (src/command_assemble.cpp:34-45, src/command_genotype.cpp:25-27). */
typedef struct otg_params {
  int32_t max_alleles;          /* -a  2                                  */
  int32_t ignore_haps;          /* !--haps  => 1                          */
  int32_t max_cov;              /* -c  200                                */
  int32_t flank;                /* -f  100                                */
  int32_t bandwidth_length;     /* -h  second field, 500                  */
  int32_t min_cov_fraction2_l;  /* -A  first field, 500                   */
  int32_t mismatch;             /* WFAlignerGapAffine(4,6,2): 4           */
  int32_t gap_open;             /*                            6           */
  int32_t gap_ext;              /*                            2           */
  int32_t realign;              /* 1 iff -r <reference> was given (flanks present in the batch) */
  double  bandwidth_short;      /* -h  0.01                               */
  double  bandwidth_long;       /* -h  0.015                              */
  double  max_error;            /* -e  0.01                               */
  double  min_cov_fraction;     /* -F  0.2                                */
  double  min_cov_fraction2_f;  /* -A  0.1                                */
  double  min_sim;              /* -s  0.9                                */
  double  gt_max_error;         /* genotype -e 0.025                      */
  double  gt_max_cosdis;        /* genotype -c 0.025                      */
  /* Heuristic of BOTH aligners of the region pipeline (see otg_set_heuristic).  The reference never calls setHeuristic*
   * (src/assemble.cpp:49-50): its aligners run WFA2-lib's default.  0 = OTG_HEURISTIC_NONE (exact; the default here),
   * 1 = OTG_HEURISTIC_WFADAPTIVE with the three numbers below (WFA2-lib's own default values: 10, 50, 1).              */
  int32_t heuristic;
  int32_t heur_min_wavefront_length;
  int32_t heur_max_distance_threshold;
  int32_t heur_steps_between_cutoffs;
} otg_params;

void otg_params_default(otg_params* p);

/* ---------------------------------------------------------------- context */
int         otg_create(int device, otg_ctx** out);
void        otg_destroy(otg_ctx* ctx);
/* Gives the aligners' scratch workspaces (provenance slabs, row tables: tens of GB once long reads have been seen) back to the device;
 * the next call that needs them allocates them again.  Resident batches and results are untouched.  For hosts that share a device
 * between contexts or processes; the reference has no counterpart (its aligners own host memory, src/assemble.cpp:45-50).          */
int         otg_trim(otg_ctx* ctx);
const char* otg_last_error(otg_ctx* ctx);     /* ctx may be NULL: last global error           */
int         otg_device_count(void);           /* number of visible HIP devices (0 if none)    */
/* Which libm exp() rounding variant the device KDE mirrors (1 = glibc FMA build, 0 = non-FMA).
 * Chosen at otg_create by probing the host libm: the variant whose restatement equals exp() on every argument of a probe set that
 * holds the arguments on which the two builds differ (SURVEY.md §7.2 "FP determinism").  The densities then equal the reference's on
 * this host as far as that set shows; otg_exp_probe_mismatches is the evidence. */
int         otg_exp_variant(otg_ctx* ctx);
/* On how many arguments of the probe set the chosen variant differed from the host libm's exp() (0 on a glibc 2.28+ host; non-zero: the
 * host libm is neither build, and KDE densities may differ from the reference's on this host in the last place).  -1 without a context. */
long long   otg_exp_probe_mismatches(otg_ctx* ctx);
/* The probe itself, without a context or a device: the size of the set, on how many of its arguments the two restatements differ from each
 * other, and each one's mismatches against the host libm.  Returns the variant otg_create would choose.  Any pointer may be NULL. */
int         otg_exp_probe(uint64_t* n_args, uint64_t* n_differ, uint64_t* mismatches_fma, uint64_t* mismatches_nofma);
/* For tests: out[i] = the host restatement of glibc's exp() in `variant` (1 = FMA build, 0 = non-FMA) — needs no device — and the device
 * function the clustering kernel calls (in-place kernel over a copy of x).  Both return OTG_OK or OTG_ERR_ARG / a HIP error. */
int         otg_exp_host(const double* x, uint64_t n, int variant, double* out);
int         otg_exp_device(otg_ctx* ctx, const double* x, uint64_t n, int variant, double* out);

/* Heuristic of the L1 aligner calls on this context — wfa::WFAligner::setHeuristicNone() /
 * setHeuristicWFadaptive(min_wavefront_length, max_distance_threshold, steps_between_cutoffs) (bindings/cpp/WFAligner.hpp:107-122 of
 * WFA2-lib).  OTG_HEURISTIC_NONE: exact alignment (default).  OTG_HEURISTIC_WFADAPTIVE: WFA2-lib's
 * adaptive wavefront reduction — after each score, diagonals whose remaining distance to the end exceeds the best one by more than
 * max_distance_threshold are dropped from both ends of the wavefront (scores >= the exact ones; op strings of a valid, possibly
 * sub-optimal alignment).  The region pipeline takes its setting from otg_params instead.                                        */
#define OTG_HEURISTIC_NONE        0
#define OTG_HEURISTIC_WFADAPTIVE  1
int otg_set_heuristic(otg_ctx* ctx, int strategy, int min_wavefront_length, int max_distance_threshold, int steps_between_cutoffs);

/* ================================================================= L1: batched aligners
 * One task = one wfa::WFAligner call.  Sequences live in one byte arena (raw bytes, compared
 * raw: 'N'=='N', case-sensitive, as WFA2 does).
 *   all four *_free == 0 and endsfree == 0  -> alignEnd2End(pattern, text)
 *   endsfree == 1 -> alignEndsFree(pattern, pattern_begin_free, pattern_end_free,
 *                                  text, text_begin_free, text_end_free)                      */
typedef struct otg_align_task {
  uint64_t pattern_off;
  uint64_t text_off;
  uint32_t pattern_len;
  uint32_t text_len;
  int32_t  pattern_begin_free;
  int32_t  pattern_end_free;
  int32_t  text_begin_free;
  int32_t  text_end_free;
  int32_t  endsfree;
  int32_t  _pad;             /* reserved, 0 */
} otg_align_task;

/* Replaces WFAlignerEdit(Score, MemoryMed)::alignEnd2End/alignEndsFree + getAlignmentScore()
 * (src/assemble.cpp:49, src/analignments.cpp:70-71,88-97).  scores_out[i] = unit-cost edit distance
 * (>= 0).  cells_out (nullable): wavefront cells W_p evaluated.                */
int otg_edit_distance_batch(otg_ctx* ctx,
                            const uint8_t* seq_arena, uint64_t arena_bytes,
                            const otg_align_task* tasks, uint32_t n_tasks,
                            int32_t* scores_out, uint64_t* cells_out);

/* Replaces WFAlignerEdit(Alignment, MemoryMed)::alignEnd2End + getAlignmentScore() + getAlignmentCigar()
 * (src/compare.cpp:59-61,95).  End-to-end only: a task with endsfree != 0 is OTG_ERR_ARG, and so is a context whose heuristic is
 * OTG_HEURISTIC_WFADAPTIVE (exact alignment only).  scores_out[i] = unit-cost edit distance.  Op strings as otg_affine_align_batch
 * (M X I D, one char per column, I consumes text, D consumes pattern; bytes compared raw), the tie-break of WFA2-lib's edit piggy-back
 * (DESIGN.md §3).  cigar_arena == NULL: only cigar_len_out (= alignment columns) is produced, cigar_off_out may be NULL.
 * *cigar_bytes_used = total length; OTG_ERR_CAPACITY when cigar_capacity is smaller.  The same alignment under wfadaptive, asked for by
 * name and per call: otg_edit_align_heur_batch below.                                                                              */
int otg_edit_align_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes,
                         const otg_align_task* tasks, uint32_t n_tasks, int32_t* scores_out,
                         uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                         uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used);
/* otg_edit_align_batch under a heuristic named per call, the way otg_params.heuristic names the pipeline's: what
 * WFAlignerEdit(Alignment, MemoryMed)::alignEnd2End returns after setHeuristicNone() / setHeuristicWFadaptive(min_wavefront_length,
 * max_distance_threshold, steps_between_cutoffs).  OTG_HEURISTIC_NONE: the results of otg_edit_align_batch.  OTG_HEURISTIC_WFADAPTIVE: score
 * and op string of the alignment the reduced wavefronts find — the score and cells of otg_edit_distance_batch on a context set to that
 * heuristic, the piggy-back tie-break with sources taken from the wavefront the cut left; a valid alignment of its score,
 * possibly sub-optimal.  The parameters are validated as otg_set_heuristic validates them; the context's own heuristic is neither consulted
 * nor left changed.  Ends-free tasks are OTG_ERR_ARG.  Length-only protocol (cigar_arena == NULL) and OTG_ERR_CAPACITY as above.
 * cells_out (nullable): wavefront cells of the score chain, as otg_edit_distance_batch reports them.                                   */
int otg_edit_align_heur_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes,
                              const otg_align_task* tasks, uint32_t n_tasks,
                              int strategy, int min_wavefront_length, int max_distance_threshold, int steps_between_cutoffs,
                              int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                              uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used, uint64_t* cells_out);
/* Replaces WFAlignerEdit(Alignment, MemoryMed)::alignEnd2End / alignEndsFree + getAlignmentScore() + getAlignmentCigar(): the call above that
 * also takes tasks with endsfree != 0 (src/analignments.cpp:88-96), mixed freely with end-to-end ones, under the heuristic named per call.
 * End-to-end tasks give exactly what otg_edit_align_batch / otg_edit_align_heur_batch give.  A task with free ends: scores_out[i] = the edit
 * operations that are not free = otg_edit_distance_batch on the same task; the alignment starts on a diagonal of the score-0 wavefront
 * [max(-pattern_begin_free, -pattern_len), min(text_begin_free, text_len)] and ends at the first diagonal, in ascending order, whose
 * cell has reached the end of the text with at most pattern_end_free of the pattern left or the end of the pattern with at most text_end_free
 * of the text left.  Op strings over M X I D with the free end gaps explicit, as otg_affine_align_batch writes them: the start
 * diagonal's I or D run, the operations with their match runs, then I up to the end of the text and D up to the end of the pattern;
 * cigar_len_out = pattern_len + every I.  Length-only protocol, OTG_ERR_CAPACITY, parameter validation, the untouched context heuristic
 * and cells_out as above.                                                                                                              */
int otg_edit_align_span_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes,
                              const otg_align_task* tasks, uint32_t n_tasks,
                              int strategy, int min_wavefront_length, int max_distance_threshold, int steps_between_cutoffs,
                              int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                              uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used, uint64_t* cells_out);
/* HIP-event times (ms) of the latest otg_edit_align_batch / otg_edit_align_heur_batch / otg_edit_align_span_batch on this context: the score
 * chain and the provenance pass (which includes the backtrace and the unpack).  Measurement hook; the reference has no counterpart. */
int otg_edit_align_last_ms(otg_ctx* ctx, double* score_ms, double* prov_ms);
/* How many tasks of the latest edit alignment call on this context were finished by the LDS-window tier (finished[0]) and by the global-row
 * tier (finished[1]) of its provenance pass; under OTG_HEURISTIC_NONE, where the host knows the width beforehand: how many
 * were given to each.  Test hook, read-only. */
int otg_edit_align_last_tiers(otg_ctx* ctx, uint32_t finished[2]);

/* Replaces WFAlignerGapAffine(x,o,e, Alignment, MemoryMed)::alignEnd2End/alignEndsFree +
 * getAlignmentCigar() (src/assemble.cpp:50, src/analignments.cpp:25,31,37,268-280).
 * scores_out[i] = gap-affine penalty (>= 0; WFA2 reports its negative).  The op string of task i
 * (alphabet M X I D, one char per column, free end gaps explicit) is written at
 * cigar_arena + cigar_off_out[i], length cigar_len_out[i].  Returns OTG_ERR_CAPACITY (and the
 * needed size in *cigar_bytes_used) if cigar_capacity is too small.                            */
int otg_affine_align_batch(otg_ctx* ctx,
                           const uint8_t* seq_arena, uint64_t arena_bytes,
                           const otg_align_task* tasks, uint32_t n_tasks,
                           int32_t mismatch, int32_t gap_open, int32_t gap_ext,
                           int32_t* scores_out,
                           uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                           uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used,
                           uint64_t* cells_out);

/* Which tier of the exact gap-affine chain was given each alignment of the latest otg_affine_align_batch on this context, and which one
 * finished it.  Test and measurement hook, read-only; the reference has no counterpart.  Valid directly behind that call
 * with the same n_tasks; OTG_ERR_ARG (with a message) when the last tier chain launched on the context was another one (edit distance,
 * an adaptive chain, a region pipeline's launch on a list of slots), when that launch failed or had another task count, after otg_trim,
 * or when the context's heuristic is OTG_HEURISTIC_WFADAPTIVE.  Waits for the stream and copies the chain's counters, lists and bounds back.
 * Per task:
 *   bound_out     the score bound U of the bound pass in units of gcd(x, o+e, e) (INT32_MAX: the pass found none), -1 when the
 *                 launch ran without a bound pass;
 *   routed_out    the tier the counting sort assigned: 0..4 = the register tiers of 1024 / 1536 / 2048 / 4096 / 8192 diagonals,
 *                 5 = none, straight to tier A (every task when the register tiers did not run);
 *   finished_out  the tier that wrote the result: 0..4 a register tier, 5 = HBM-row tier A, 6 = tier B, 7 = the generic kernel,
 *                 -2 = the generic kernel gave up too (the task's score is negative).
 * counts_out / lists_out, both NULL or both given, receive the same launch's raw lists from the same snapshot.  counts_out[OTG_AFFINE_N_COUNTS]:
 * [0..6] the counting sort's segment bounds (register tier t owns sorted[counts[t] .. counts[t+1]), [5]..[6] is what no register tier
 * takes), [7] length of tier A's input (that rest, then what the register tiers gave up, appended), [8] what tier A gave up, [9] what
 * tier B gave up.  lists_out[4 * n_tasks]: tier A's give-ups | tier B's give-ups | the sort's output | tier A's input, each in a stride
 * of n_tasks; only the lengths above are meaningful.  Lists a launch did not write (no register tiers, no HBM-row tiers) have length 0.
 * Returns the mask of register tiers that ran (bit t = tier t; >= 0), or a negative error code. */
#define OTG_AFFINE_TIER_NONE  5
#define OTG_AFFINE_FIN_A      5
#define OTG_AFFINE_FIN_B      6
#define OTG_AFFINE_FIN_C      7
#define OTG_AFFINE_N_COUNTS   10
int otg_affine_last_routing(otg_ctx* ctx, uint32_t n_tasks, int32_t* bound_out, int8_t* routed_out, int8_t* finished_out,
                            uint32_t* counts_out, uint32_t* lists_out);

/* ================================================================= L2: per-region operators */

/* Replaces otter_hclust (src/otterclust.cpp:118-320) incl. otter_find_clustering_dist (:20-116),
 * KDE (src/ankde.cpp), hclust_fast / cutree_cdist / cutree_k (include/hclust-cpp/fastcluster.cpp).
 * Region r has n_valid[r] valid reads, its condensed FP64 matrix (DistMatrix layout,
 * src/andistmat.cpp:20) starts at dist + dist_off[r], its read lengths at read_len + len_off[r].
 * Outputs: labels (same indexing as read_len), ic/fc per region, bounds = 3 doubles per region
 * (dist0, dist1, cut0; NaN when the KDE was not evaluated).                                    */
int otg_cluster_batch(otg_ctx* ctx, const otg_params* params,
                      const double* dist, const uint64_t* dist_off,
                      const uint32_t* read_len, const uint64_t* len_off,
                      const uint32_t* n_valid, uint32_t n_regions,
                      int32_t* labels_out, int32_t* ic_out, int32_t* fc_out, double* bounds_out);

/* For tests (like otg_affine_last_routing): otg_cluster_batch with the intermediates of every region copied out.  exp_variant -1 = the
 * context's, 0 / 1 = that variant of exp().  A region that ends in an error code 1-5 does not fail the call: its code is in the trace
 * (labels -1, ic = fc = 0).  The caller allocates every array; what the kernel does not reach keeps the fill (every byte 0xff).
 *   per region, OTG_TRACE_GRID doubles (n_grid used): dens_raw = KDE::f on the grid, dens = normalised, sums = the window sums;
 *   per region, OTG_TRACE_EXT entries (n_max / n_min used): max_i / max_v, min_i / min_v = the extrema of KDE::maximas;
 *   state, 8 ints per region: evaluated (0: n <= 2 or max_alleles == 1, nothing else written), n_grid, n_max, n_min, do_hclust, err,
 *     cut_k (clusters of the first cut), recut (1: cutree_k(max_alleles) replaced the labels);  scalars, 2 doubles: bandwidth, dist_final;
 *   with do_hclust: merge (R convention, column-major, 2(n-1) ints at 2 * len_off[r]), height (n-1 doubles at len_off[r]),
 *     labels_first (n ints at len_off[r]: the first cut, before the coverage repair).                                                   */
#define OTG_TRACE_GRID 512
#define OTG_TRACE_EXT 258
typedef struct otg_cluster_trace {
  double *dens_raw, *dens, *sums;
  int32_t* max_i; double* max_v;
  int32_t* min_i; double* min_v;
  int32_t* state; double* scalars;
  int32_t* merge; double* height; int32_t* labels_first;
} otg_cluster_trace;
int otg_cluster_trace_batch(otg_ctx* ctx, const otg_params* params,
                            const double* dist, const uint64_t* dist_off,
                            const uint32_t* read_len, const uint64_t* len_off,
                            const uint32_t* n_valid, uint32_t n_regions,
                            int32_t* labels_out, int32_t* ic_out, int32_t* fc_out, double* bounds_out,
                            int exp_variant, const otg_cluster_trace* trace);

/* Replaces PPOA (src/anppoa.hpp:64-380) as driven by rapid_consensus (src/analignments.cpp:261-292):
 * graph g has backbone = task `backbone`, then members inserted in order; each member is a
 * sequence + its op string + spanning flags.  c/t are the adjust_weights arguments, per graph:
 * every edge weight w (a count, at most n_members + 1) becomes w - max(c, t * w) before the
 * heaviest-path sweep, in FP32, the product and the subtraction rounded separately (no
 * contraction into a fused multiply-add), as the reference's own build computes it.  Any finite
 * float of any sign is supported for both: c = 0, t = 1 makes every weight zero (the tie-breaks
 * alone pick the path), c > n_members + 1 makes every weight negative; the results match the
 * reference bit for bit there too.  NaN and infinities are the caller's problem (not checked).
 * rapid_consensus passes c = (float)(n * 0.4), 1 below four reads, and t = 0.3f.
 * Output consensus strings in out_arena (same off/len convention as cigars).                   */
typedef struct otg_poa_member {
  uint64_t seq_off;   uint32_t seq_len;   uint32_t cigar_len;
  uint64_t cigar_off;
  uint8_t  spanning_l, spanning_r; uint8_t _pad[6];
} otg_poa_member;

typedef struct otg_poa_graph {
  uint64_t backbone_off; uint32_t backbone_len;
  uint32_t first_member; uint32_t n_members;
  float    c, t; uint32_t _pad;
} otg_poa_graph;

int otg_poa_consensus_batch(otg_ctx* ctx,
                            const uint8_t* seq_arena, uint64_t arena_bytes,
                            const uint8_t* cigar_arena, uint64_t cigar_bytes,
                            const otg_poa_member* members, uint32_t n_members,
                            const otg_poa_graph* graphs, uint32_t n_graphs,
                            uint64_t* out_off, uint32_t* out_len,
                            uint8_t* out_arena, uint64_t out_capacity, uint64_t* out_bytes_used);

/* Replaces anallele_cluster (src/otterclust.cpp:463-527) for `otter genotype`.
 * Region r has n_alleles[r] allele sequences described by (seq_off,seq_len) entries starting at
 * allele index first_allele[r].  Outputs per allele: gt, gt_l, gt_k, hsd; per region: n_gt and
 * representative allele indices (region-local) written at reps_out + first_allele[r].           */
int otg_genotype_cluster_batch(otg_ctx* ctx, const otg_params* params,
                               const uint8_t* seq_arena, uint64_t arena_bytes,
                               const uint64_t* seq_off, const uint32_t* seq_len,
                               const uint32_t* first_allele, const uint32_t* n_alleles, uint32_t n_regions,
                               int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out,
                               int32_t* n_gt_out, int32_t* reps_out);

/* For tests (like otg_affine_last_routing): otg_genotype_cluster_batch with the kernel's matrices copied out.  Region r's condensed matrices
 * (row-major pairs i < j) start at the running sum of A (A - 1) / 2 over the regions before it, its per-allele rows at first_allele[r]:
 *   dl = length-ratio matrix, dk = 3-mer cosine-distance matrix (both as computed, before clustering);
 *   kvec = 65 frequencies per allele (64 three-mers + the bin of three-mers with a byte outside ACGT), vnorm = their Euclidean norm;
 *   height_l / height_k = the A - 1 merge heights of the two average-linkage clusterings, from the region's first allele on.
 * The caller allocates: dl, dk [total pairs], kvec [alleles x 65], vnorm, height_l, height_k [alleles].                                    */
typedef struct otg_genotype_trace {
  double *dl, *dk, *kvec, *vnorm, *height_l, *height_k;
} otg_genotype_trace;
int otg_genotype_cluster_trace_batch(otg_ctx* ctx, const otg_params* params,
                                     const uint8_t* seq_arena, uint64_t arena_bytes,
                                     const uint64_t* seq_off, const uint32_t* seq_len,
                                     const uint32_t* first_allele, const uint32_t* n_alleles, uint32_t n_regions,
                                     int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out,
                                     int32_t* n_gt_out, int32_t* reps_out, const otg_genotype_trace* trace);

/* The metric of anallele_cluster's FIRST matrix (the one cut at gt_max_error, "Maximum sequence dissimilarity").
 *   OTG_GT_METRIC_LENGTH  the reference's length-ratio matrix: otg_genotype_cluster_batch, bit for bit.
 *   OTG_GT_METRIC_EDIT    the sequence dissimilarity align_anreads computes (src/analignments.cpp:62-72): 0.0 for two equal byte strings,
 *                         otherwise edit(pattern, text) / (double)max(len), end to end, unit cost, the pattern being the longer sequence (the
 *                         lower index on equal length).  Always the EXACT distance, whatever otg_set_heuristic left on the context (which
 *                         the call neither reads nor changes).  The clustering, the cut, the 3-mer partition, hsd, the genotypes and the
 *                         medoids are computed as before, on this matrix.  Alleles with the same bytes are aligned once per region.
 * otg_genotype_cluster_metric_batch: the arguments and results of otg_genotype_cluster_batch, then the metric (any other value: OTG_ERR_ARG),
 *   dist_out (nullable): the first matrix as clustered, condensed, region after region at the running sum of A (A - 1) / 2;
 *   n_aligned_out (nullable): pairs of distinct sequences scored (0 under LENGTH).
 * OTG_ERR_CAPACITY: "batch too large: split it" when the pair slots of the batch pass 2^32 (EDIT; nothing is allocated), or a pair beyond
 * the capacity of the edit aligner (the message names the region; no partial results).                                              */
#define OTG_GT_METRIC_LENGTH 0
#define OTG_GT_METRIC_EDIT   1
int otg_genotype_cluster_metric_batch(otg_ctx* ctx, const otg_params* params,
                                      const uint8_t* seq_arena, uint64_t arena_bytes,
                                      const uint64_t* seq_off, const uint32_t* seq_len,
                                      const uint32_t* first_allele, const uint32_t* n_alleles, uint32_t n_regions,
                                      int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out,
                                      int32_t* n_gt_out, int32_t* reps_out,
                                      int32_t metric, double* dist_out, uint64_t* n_aligned_out);
/* HIP-event times (ms) of the two device parts of the latest otg_genotype_cluster_metric_batch / otg_genotype_cohort_metric on this context:
 * align_ms = allele classes + pair tasks + the edit chain + the fan-out (0 under LENGTH), cluster_ms = the clustering kernels.  Their sum is
 * what otg_last_kernel_ms reports.  Measurement hook, like otg_edit_align_last_ms.                                                   */
int otg_genotype_metric_last_ms(otg_ctx* ctx, double* align_ms, double* cluster_ms);

/* HIP-event time (ms, events on the context's own stream) of the device kernels of the latest otg_genotype_cluster_batch on this context:
 * what a roofline figure divides by; host copies excluded.  The reference has no counterpart (measurement hook).        */
int otg_last_kernel_ms(otg_ctx* ctx, double* ms);

/* Replaces seq2kcounts + KUSAGE + KUSAGE::hsdiv + get_gc_content for each allele of `otter vcf2mat` (src/anseqs.cpp:111-121,135-166,
 * 186,203-208; src/vcf2mat.cpp:38-46,66-72).  Allele i is seq_arena[seq_off[i] .. + seq_len[i]).  1 <= k <= OTG_KMER_MAX (OTG_ERR_ARG
 * otherwise).  Each of the L-k+1 windows is counted once: bin = base-4 code (A/a=0 C/c=1 G/g=2 T/t=3, first base most significant) when all k
 * bytes are ACGTacgt, else bin 4^k.  usage_out: n rows of 4^k+1 doubles, row-major, value = count / total (total = L-k+1 as an int; 0/0 = NaN
 * when L < k); gc_out[i] = (C/c/G/g bytes) / L (NaN when L = 0); hsd_out[i] = e^(-sum v log v) over the bins with v > 0 in ascending order
 * (1 when there is none).  Counts, values and GC are exact; hsd carries the device's log/pow.  A NULL output is left in HBM
 * (otg_kmer_usage_device_results).  A batch whose rows (and, for k >= 8, u32 histograms) exceed the 4 GiB workspace is OTG_ERR_CAPACITY. */
int otg_kmer_usage_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                         uint32_t n, int32_t k, double* usage_out, double* gc_out, double* hsd_out);
/* Device pointers of the latest otg_kmer_usage_batch of this context (n and k as passed to it): usage rows, gc, hsd.  Valid until the next
 * otg_kmer_usage_batch on this context or otg_destroy.  The reference has no counterpart. */
int otg_kmer_usage_device_results(otg_ctx* ctx, uint32_t n, int32_t k, const double** usage, const double** gc, const double** hsd);
/* HIP-event times (ms) of the latest otg_kmer_usage_batch on this context: counting (k <= 7: counting and epilogue in one kernel) and the
 * epilogue passes of k >= 8.  Measurement hook; the reference has no counterpart. */
int otg_kmer_usage_last_ms(otg_ctx* ctx, double* count_ms, double* epilogue_ms);

/* ================================================================= L3: region-batch pipeline
 * SoA image of std::vector<ANREAD> (src/anseqs.hpp:56-76) for a batch of regions.               */
typedef struct otg_read {
  uint64_t seq_off;          /* into seq_arena                                   */
  uint32_t seq_len;
  uint8_t  spanning_l;       /* ANREAD::is_spanning_l                            */
  uint8_t  spanning_r;       /* ANREAD::is_spanning_r                            */
  uint16_t _pad;
  int32_t  ps, hp;           /* HAPLOTAG (-1 = undefined)                        */
  int32_t  ccoord_first;     /* ANREAD::ccoords                                  */
  int32_t  ccoord_second;
} otg_read;

typedef struct otg_region {
  uint32_t first_read;       /* index into reads[]                               */
  uint32_t n_reads;
  uint64_t flank_l_off;      /* reference flank [start-flank,start], upper-cased  */
  uint64_t flank_r_off;      /* reference flank [end,end+flank]                   */
  uint32_t flank_l_len;      /* 0 when -r not given                              */
  uint32_t flank_r_len;
} otg_region;

/* image of ANALLELE (src/anseqs.hpp:40-54) */
typedef struct otg_allele {
  uint64_t seq_off;          /* into the output arena                            */
  uint32_t seq_len;
  int32_t  scov, acov, tcov;
  float    se;
  int32_t  ic;
  int32_t  ps, hp;
  uint32_t region;           /* batch-local region index                         */
  int32_t  label;            /* allele index within the region (0..fc-1)         */
} otg_allele;

typedef struct otg_region_result {
  uint32_t first_allele;
  uint32_t n_alleles;        /* = fc for OK regions, else 0                      */
  int32_t  status;           /* OTG_REGION_*                                     */
  int32_t  ic, fc;
  int32_t  n_valid;
} otg_region_result;

/* ---------------------------------------------------------------------------------------------
 * Record emit (the first "next" row after the hot path): the text `otter assemble`
 * prints for the allele records of a batch — reference: the emit loop src/assemble.cpp:143-149 ->
 * ANALLELE::stdout_sam / stdout_fa (src/anseqs.cpp:42-63), BED::toScString (src/anbed.cpp:17-20),
 * header lines src/assemble.cpp:167-177.  Host-side formatting (no device work), byte-identical to the
 * reference: regions in batch order (= BED order; the reference's own order with -t 1), alleles in label
 * order; `se` printed the way `std::cout << float` prints it.
 * ------------------------------------------------------------------------------------------- */
typedef struct otg_bed {
  uint64_t chr_off;          /* chromosome name: chr_arena + chr_off, chr_len bytes (no terminator needed) */
  uint32_t chr_len;
  int32_t  start, end;       /* the UN-modified BED coordinates (local_bed, src/assemble.cpp:53)           */
  uint32_t reserved;
} otg_bed;

/* Writes the record lines into `out` (capacity out_capacity) and their total length into *out_len; returns
 * OTG_ERR_CAPACITY (with *out_len = bytes needed) when the buffer is too small.  is_fasta: 0 = SAM lines
 * (name `chr:start-end_l`, read group tag when read_group is non-empty), 1 = FASTA (`>rg#chr:start-end#l#...`). */
int otg_emit_alleles(const otg_bed* beds, const char* chr_arena, uint32_t n_regions,
                     const otg_region_result* regions, const otg_allele* alleles, const uint8_t* seqs,
                     const char* read_group, int is_fasta, char* out, uint64_t out_capacity, uint64_t* out_len);
/* The three kinds of SAM header lines of src/assemble.cpp:167-177: @SQ per target, @RG, @PG with the offsets. */
int otg_emit_sam_header(const char* name_arena, const uint64_t* name_off, const uint32_t* name_len,
                        const uint64_t* target_len, uint32_t n_targets, const char* read_group,
                        int32_t offset_l, int32_t offset_r, char* out, uint64_t out_capacity, uint64_t* out_len);

/* ---------------------------------------------------------------------------------------------
 * BAM/BAI region ingest: the reads of each BED region as `parse_anreads` delivers them to the hot
 * path (src/anseqs.cpp:244-460, called at src/assemble.cpp:55-65), straight into the region batch of
 * otg_assemble_submit.  Host code (zlib + stdio); the index is `<bam>.bai` (src/anbamfilehelper.cpp:20).
 * ------------------------------------------------------------------------------------------- */
typedef struct otg_bam otg_bam;
typedef struct otg_fasta otg_fasta;     /* indexed FASTA handle, see otg_fasta_open below */
typedef struct otg_ingest_opts {
  int32_t offset_l, offset_r;   /* --offset: the query region is [start - offset_l, end + offset_r] (src/assemble.cpp:55-57) */
  int32_t mapq;                 /* --mapq                                                     */
  int32_t nonprimary;           /* --non-primary: keep secondary / supplementary alignments   */
  int32_t omit_nonspanning;     /* --omit-nonspanning                                         */
  int32_t threads;              /* host threads for the ingest (regions are split into contiguous slices); <= 1: one */
  double  read_quality;         /* --read-quality (tag rq)                                    */
} otg_ingest_opts;
int  otg_bam_open(const char* bam_path, otg_bam** out);
void otg_bam_close(otg_bam* bam);
uint32_t otg_bam_n_targets(const otg_bam* bam);
const char* otg_bam_target(const otg_bam* bam, uint32_t i, uint64_t* length);   /* name (owned by the handle) + length: @SQ lines */
/* Appends the reads of n_regions BED regions to arena / reads (in-out counters *arena_used, *n_reads) and fills
 * regions[i].first_read / n_reads (flank fields zeroed).  OTG_ERR_CAPACITY: buffers too small, the counters hold the
 * needed totals.  Reads come in file order; filters, sub-sequence, spanning flags and clip coordinates as the reference. */
int  otg_ingest_regions(otg_bam* bam, const otg_bed* beds, const char* chr_arena, uint32_t n_regions,
                        const otg_ingest_opts* opts, uint8_t* arena, uint64_t arena_capacity, uint64_t* arena_used,
                        otg_read* reads, uint32_t reads_capacity, uint32_t* n_reads, otg_region* regions);

/* The same, also returning what `--reads-only` prints per read: ANREAD::name and ANREAD::rq (src/anseqs.cpp:447,250-251).
 * meta[i] belongs to reads[i]; names are appended to name_arena (in-out counter *name_used, no terminators).  meta == NULL:
 * exactly otg_ingest_regions. */
typedef struct otg_read_meta {
  uint64_t name_off;         /* into name_arena                                   */
  uint32_t name_len;
  uint32_t reserved;
  double   rq;               /* tag rq, 0 when absent                             */
} otg_read_meta;
int  otg_ingest_regions_named(otg_bam* bam, const otg_bed* beds, const char* chr_arena, uint32_t n_regions,
                              const otg_ingest_opts* opts, uint8_t* arena, uint64_t arena_capacity, uint64_t* arena_used,
                              otg_read* reads, uint32_t reads_capacity, uint32_t* n_reads, otg_region* regions,
                              otg_read_meta* meta, char* name_arena, uint64_t name_capacity, uint64_t* name_used);
/* `otter assemble --reads-only`: the read records of each region instead of alleles (src/assemble.cpp:82-89 ->
 * ANREAD::stdout_sam / stdout_fa, src/anseqs.cpp:83-106).  Regions with more than max_cov reads print nothing
 * (src/assemble.cpp:69; max_cov < 0: no limit).  Same buffer protocol as otg_emit_alleles. */
int  otg_emit_reads(const otg_bed* beds, const char* chr_arena, uint32_t n_regions, const otg_region* regions,
                    const otg_read* reads, const uint8_t* seq_arena, const otg_read_meta* meta, const char* name_arena,
                    const char* read_group, int is_fasta, int32_t max_cov, char* out, uint64_t out_capacity, uint64_t* out_len);

/* ---------------------------------------------------------------------------------------------
 * `otter genotype` ingest: the allele BAM written by `otter assemble`.
 * ------------------------------------------------------------------------------------------- */
/* SampleIndex::init (src/anbamdb.cpp:10-63): sample names = the `@RG ID:` values in header order (everything after "ID:",
 * as the reference takes it), offsets from `@PG ID:otter OF:l,r` (defaults 1, 0).  Errors as the reference's exit(1) cases. */
int  otg_bam_sample_index(otg_bam* bam, uint32_t* n_samples, int32_t* offset_l, int32_t* offset_r);
const char* otg_bam_sample(const otg_bam* bam, uint32_t i);      /* valid after otg_bam_sample_index */
/* parse_analleles (src/anseqs.cpp:462-524) per BED region: the records whose `ta` tag equals "chr:start-end", in file order, as
 * otg_allele records (seq, sc/ac/tc, se, ic, PS/HP; .region = region index, .label = SAMPLE index of the RG tag; an unknown
 * read group is the reference's exit(1): OTG_ERR_ARG).  With a FASTA handle the reference allele of genotype_process
 * (src/genotype.cpp:92-101: bases [start - offset_l, end + offset_r - 1], sample index = n_samples) is appended to every
 * non-empty region.  first_allele has n_regions + 1 entries (in-out counter *n_alleles is the running total). */
int  otg_ingest_alleles(otg_bam* bam, const otg_bed* beds, const char* chr_arena, uint32_t n_regions, int32_t threads,
                        const otg_fasta* reference, uint8_t* arena, uint64_t arena_capacity, uint64_t* arena_used,
                        otg_allele* alleles, uint32_t alleles_capacity, uint32_t* n_alleles, uint32_t* first_allele);

/* `otter genotype` record emit.  The header: output_vcf_header (src/genotype.cpp:16-40; contigs = BAM targets,
 * one column per sample of otg_bam_sample_index).  The lines: per region with alleles, genotype numbers re-centred on the reference
 * allele (src/genotype.cpp:139-150) and output_vcf_line (:43-78) — alleles / first_allele as otg_ingest_alleles delivers them with a
 * reference (reference allele last in every region, .label = sample index, n_samples = number of real samples); gt / hsd / n_gt /
 * reps exactly as otg_genotype_cluster_batch returns them (per allele, per region, region-local representative indices at
 * reps + first_allele[r]).  Without a reference `otter genotype` prints the shorter and longer allele length per sample instead
 * (src/genotype.cpp:112-121): otg_emit_genotype_lengths.  Same buffer protocol as otg_emit_alleles. */
int  otg_emit_vcf_header(const otg_bam* bam, char* out, uint64_t out_capacity, uint64_t* out_len);
int  otg_emit_vcf_lines(const otg_bed* beds, const char* chr_arena, uint32_t n_regions, const uint32_t* first_allele,
                        const otg_allele* alleles, const uint8_t* seqs, uint32_t n_samples, const int32_t* gt, const double* hsd,
                        const int32_t* n_gt, const int32_t* reps, int32_t offset_l, int32_t offset_r,
                        char* out, uint64_t out_capacity, uint64_t* out_len);
int  otg_emit_genotype_lengths(const otg_bam* bam, const otg_bed* beds, const char* chr_arena, uint32_t n_regions,
                               const uint32_t* first_allele, const otg_allele* alleles, uint32_t n_samples,
                               char* out, uint64_t out_capacity, uint64_t* out_len);

/* ---------------------------------------------------------------------------------------------
 * The two text inputs beside the BAM: the BED file of regions and the indexed FASTA the reference
 * flanks of local_realignment come from.  Host code.
 * ------------------------------------------------------------------------------------------- */
/* parse_bed_file (src/anbed.cpp:23-80): tab-separated `chr start end [...]` or single-column `chr:start-end` lines;
 * '#' lines, empty lines and lines the reference calls ambiguous are skipped (*n_skipped counts the latter two kinds,
 * nullable); coordinates go through the same unsigned-32-bit conversion.  A coordinate that is not a number makes the
 * reference terminate: OTG_ERR_ARG here.  OTG_ERR_CAPACITY: *n_beds / *chr_used hold the needed sizes. */
int  otg_parse_bed_file(const char* path, otg_bed* beds, uint32_t beds_capacity, uint32_t* n_beds, char* chr_arena,
                        uint64_t chr_capacity, uint64_t* chr_used, uint32_t* n_skipped);
/* FaidxInstance (src/anfahelper.cpp:6-20) over an uncompressed FASTA with its `.fai` (read when present, otherwise built
 * as src/faidx.c:64-133 does and written beside the file when possible).  Handles are read-only after open: one may be
 * shared by threads. */
int  otg_fasta_open(const char* fasta_path, otg_fasta** out);
void otg_fasta_close(otg_fasta* fa);
uint32_t otg_fasta_n_seqs(const otg_fasta* fa);
const char* otg_fasta_seq(const otg_fasta* fa, uint32_t i, int64_t* length);
/* FaidxInstance::fetch: bases [beg, end_inclusive] (0-based), clamped into the contig as faidx_fetch_seq clamps them
 * (src/faidx.c:418-445), upper-cased; an unknown contig gives length 0. */
int  otg_fasta_fetch(const otg_fasta* fa, const char* chr, uint32_t chr_len, int32_t beg, int32_t end_inclusive,
                     char* out, uint64_t out_capacity, uint64_t* out_len);
/* The two flanks of every region, [start - offset_l - flank, start - offset_l] and [end + offset_r, end + offset_r + flank]
 * (src/analignments.cpp:22,28 on mod_bed, src/assemble.cpp:55-57), appended to the region batch's arena (in-out counter
 * *arena_used); fills regions[i].flank_{l,r}_{off,len} and leaves the read fields alone. */
int  otg_fasta_region_flanks(const otg_fasta* fa, const otg_bed* beds, const char* chr_arena, uint32_t n_regions,
                             int32_t offset_l, int32_t offset_r, int32_t flank, uint8_t* arena, uint64_t arena_capacity,
                             uint64_t* arena_used, otg_region* regions);

/* A sink for record text: called with consecutive pieces of the output; a non-zero return aborts the call. */
typedef int (*otg_write_fn)(void* user, const char* data, uint64_t len);

/* ---------------------------------------------------------------------------------------------
 * `otter wgat`: the BED regions sliced out of whole-genome assembly alignments, as allele records `otter genotype`
 * reads — wgat() / wga_bam_genotyper_process (src/wgat.cpp:31-179) with get_op_intervals (src/opinterval.cpp:12-34).  Host code.
 * Per BAM target in header order, per alignment in file order, per overlapping region in the order the reference's interval tree reports
 * them: the query interval under [start - offset_l, end + offset_r] from the CIGAR operations that overlap it; alignments clipped inside
 * the interval are skipped (the reference's warning).  Record lines as ANALLELE::stdout_sam / stdout_fa print them (name
 * `contig#chr:start-end_index`, tc / ac / sc = 1, sp:A:b); SAM output starts with the @SQ / @RG / @PG OF: lines.  Order = the reference's
 * with -t 1.  *n_records (nullable) = records written. */
int otg_wgat(otg_bam* bam, const otg_bed* beds, const char* chr_arena, uint32_t n_beds, const char* read_group, int is_fasta,
             int32_t offset_l, int32_t offset_r, otg_write_fn write, void* user, uint64_t* n_records);

/* Workload statistics of the last otg_assemble_run (for the roofline figure). */
typedef struct otg_run_stats {
  uint64_t n_regions, n_regions_ok;
  uint64_t edit_tasks,   edit_cells,   edit_seq_bytes;
  uint64_t affine_tasks, affine_cells, affine_seq_bytes;
  uint64_t allele_bytes;
  uint64_t algorithmic_bytes;         /* Σ (a+b) + 4·W (+ W/2 for CIGAR scope) + Σ(len+40) */
  double   ms_edit, ms_cluster, ms_reassign, ms_affine, ms_poa, ms_realign, ms_total;
  double   ms_edit_kernel;            /* HIP-event time of the edit WFA kernel launches (tier 1, summed)   */
  uint64_t edit_kernel_launches;
  double   ms_affine_kernel;          /* HIP-event time of the gap-affine WFA kernel launches (tier 1)     */
  uint64_t affine_kernel_launches;
  uint64_t affine_visited_cells;      /* (score, diagonal) cells the exact gap-affine kernels actually evaluated (pruned wavefronts) */
} otg_run_stats;

/* Upload a batch (H2D).  After it returns the inputs are resident in HBM.                       */
int otg_assemble_submit(otg_ctx* ctx, const otg_params* params,
                        const uint8_t* seq_arena, uint64_t arena_bytes,
                        const otg_read* reads, uint32_t n_reads,
                        const otg_region* regions, uint32_t n_regions);
/* Run the whole hot path on the resident batch: [local_realignment] -> fill_dist_matrix ->
 * otter_hclust -> invalid_reassignment -> rapid_consensus.  Results stay resident.             */
int otg_assemble_run(otg_ctx* ctx);
/* `otter assemble --reads-only -r`: run local_realignment alone on the resident batch (src/assemble.cpp:72-89 stops there), then read
 * the read descriptors back: a rescued read has its seq_off / seq_len trimmed (src/analignments.cpp:53-54) and both spanning flags
 * set; everything else is as submitted.  otg_emit_reads on them prints what the reference prints.  n_reads = the submitted count. */
int otg_assemble_realign(otg_ctx* ctx);
int otg_assemble_collect_reads(otg_ctx* ctx, otg_read* reads_out, uint32_t n_reads);
/* Sizes needed by otg_assemble_collect for the last run.                                        */
int otg_assemble_result_sizes(otg_ctx* ctx, uint32_t* n_alleles, uint64_t* seq_bytes);
/* Device-resident results of the last run, for callers that forward them without a host round trip
 * (one process per GPU: the end-of-run gather of allele records to rank 0, north_star / src/assemble.cpp:143-149
 * in the single-process reference).  Pointers are HBM addresses on the context's device, valid until the next
 * otg_assemble_submit / otg_assemble_run / otg_destroy; sizes: n_regions records, and the two figures of
 * otg_assemble_result_sizes.  The library's stream is synchronised before returning.             */
int otg_assemble_device_results(otg_ctx* ctx, const otg_region_result** d_regions, const otg_allele** d_alleles,
                                const uint8_t** d_seqs);
/* ---------------------------------------------------------------------------------------------
 * One process per GPU: the end-of-run gather of the allele records to rank 0 over RCCL (xGMI) — north_star's multi-GPU form; the
 * single-process reference prints under a mutex instead (src/assemble.cpp:143-149).  Rank r owns the r-th contiguous BED shard
 * (src/BS_thread_pool.hpp:183-198), so rank order is BED order.  librccl is loaded at run time by the first call.
 *   otg_comm_unique_id   rank 0 makes the 128-byte id; the host hands it to the other ranks (file, socket, environment: its business);
 *   otg_comm_create      every rank, with its device, its rank and the world size (collective: returns when all ranks have called it);
 *   otg_gather_sizes     after otg_assemble_run: counts_out[3 * r + {0, 1, 2}] = regions, allele records, sequence bytes of rank r (every rank);
 *   otg_gather_records   rank 0 passes buffers for the totals and receives regions / alleles / sequences of all ranks in rank order,
 *                        region / allele / sequence indices rebased to job-wide ones; the other ranks pass NULL.  Records travel
 *                        device -> device; the one device-to-host copy happens on rank 0.
 * ------------------------------------------------------------------------------------------- */
#define OTG_COMM_ID_BYTES 128
typedef struct otg_comm otg_comm;
int  otg_comm_unique_id(uint8_t* id_out);
int  otg_comm_create(int device, int rank, int world, const uint8_t* id, otg_comm** out);
void otg_comm_destroy(otg_comm* comm);
int  otg_gather_sizes(otg_ctx* ctx, otg_comm* comm, uint64_t* counts_out);
int  otg_gather_records(otg_ctx* ctx, otg_comm* comm, const uint64_t* counts, otg_region_result* regions_out, otg_allele* alleles_out, uint8_t* seqs_out);

/* D2H of the results.  labels_out (nullable) gets the final per-read label (-1 unassigned).     */
int otg_assemble_collect(otg_ctx* ctx,
                         otg_region_result* region_out,
                         otg_allele* alleles_out, uint32_t allele_capacity,
                         uint8_t* seq_out, uint64_t seq_capacity,
                         int32_t* labels_out);
int otg_assemble_stats(otg_ctx* ctx, otg_run_stats* out);
/* The distance matrices fill_dist_matrix left on the device in the last run (src/analignments.cpp:103-124), for tests and diagnosis: region r's
 * condensed matrix over its V valid reads (row-major upper triangle, V (V - 1) / 2 values) starts at the sum of N (N - 1) / 2 over the regions
 * before it, N = a region's submitted read count (0 for a region above max_cov).  n_slots = that sum over all regions.                  */
int otg_assemble_collect_dist(otg_ctx* ctx, double* dist_out, uint64_t n_slots);

/* ---------------------------------------------------------------------------------------------
 * The dispatcher: `otter assemble` from files to record text in one call — the role of assemble() /
 * assemble_process() (src/assemble.cpp:39-179) over BS::thread_pool::parallelize_loop (src/BS_thread_pool.hpp:175-200).
 * The BED list is split into one contiguous shard per device (the reference's static split, GPUs for threads); every shard is cut
 * into bounded batches of `batch_regions` regions that are ingested on host threads, run through the hot path on the device (two
 * contexts per device: the upload of a batch overlaps the kernels of the previous one) and emitted, the three stages concurrently.
 * Text reaches `write` strictly in BED order (SAM header first unless is_fasta), whatever the batch size or the number of devices.
 * Host memory is bounded by the batch size.  A non-zero return of `write` aborts the job.
 * ------------------------------------------------------------------------------------------- */
typedef struct otg_assemble_job {
  const char* bam_path;          /* <BAM> (its index is <BAM>.bai)                                   */
  const char* bed_path;          /* -b                                                               */
  const char* fasta_path;        /* -r (NULL or "": no local re-alignment)                           */
  const char* read_group;        /* -R sample name                                                   */
  int32_t     is_fasta;          /* --fasta                                                          */
  int32_t     reads_only;        /* --reads-only                                                     */
  otg_params  params;            /* heuristics (realign is set from fasta_path)                      */
  otg_ingest_opts ingest;        /* --offset, --mapq, --non-primary, --omit-nonspanning, --read-quality; .threads = -t (host ingest threads) */
  uint32_t    batch_regions;     /* regions per batch; 0 = the library's plan: 256, 512, 1024 first, then
                                  * batches of 2048, the last stretch in two equal halves                */
  int32_t     n_devices;         /* 0: device 0 only                                                 */
  const int32_t* devices;        /* HIP device ordinals, one shard each                              */
} otg_assemble_job;
typedef struct otg_job_stats {
  uint64_t n_regions, n_regions_ok, n_regions_skipped, n_reads, n_alleles, input_bytes, output_bytes;
  uint32_t n_devices, reserved;
  double   ms_total;             /* wall                                                             */
  double   ms_ingest, ms_hot_path, ms_emit;   /* busy time of the three stages, summed over their threads (they overlap) */
} otg_job_stats;
/* (otg_write_fn is declared above, with otg_wgat) */
int otg_assemble_files(const otg_assemble_job* job, otg_write_fn write, void* user, otg_job_stats* stats);
/* `otter genotype` from files to text in one call — genotype() / genotype_process() (src/genotype.cpp:69-192): BED regions in bounded
 * batches through allele ingest (otg_ingest_alleles on `threads` host threads), anallele_cluster on the device (otg_genotype_cluster_batch)
 * and the VCF text (header first; otg_emit_vcf_lines), in BED order.  Without a reference FASTA the reference prints region, sample and the
 * two allele lengths instead (src/genotype.cpp:112-121): otg_emit_genotype_lengths, no device work.  stats: n_reads counts allele records. */
typedef struct otg_genotype_job {
  const char* bam_path;          /* the allele BAM `otter assemble` wrote (its index is <BAM>.bai)  */
  const char* bed_path;          /* -b                                                               */
  const char* fasta_path;        /* -r (NULL or "": the length table instead of VCF)                 */
  otg_params  params;            /* gt_max_error (-e), gt_max_cosdis (-c)                            */
  int32_t     threads;           /* -t: host threads of the allele ingest                            */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_regions;     /* regions per batch, 0 = 1024                                      */
  uint32_t    metric;            /* OTG_GT_METRIC_LENGTH (0) or OTG_GT_METRIC_EDIT; ignored without a FASTA; other values: OTG_ERR_ARG */
} otg_genotype_job;
int otg_genotype_files(const otg_genotype_job* job, otg_write_fn write, void* user, otg_job_stats* stats);
/* ---------------------------------------------------------------------------------------------
 * `otter compare` (src/compare.cpp, src/command_compare.cpp): truth alleles against assembled alleles per BED region.
 * ------------------------------------------------------------------------------------------- */
/* The allele records of each region as compare() reads them (src/compare.cpp:26-48,104-105), with its own sample map: sample0 (the truth
 * BAM's first @RG) -> 0, then sample1 (the query BAM's first @RG) -> 1; one key (-> 1) when the names are equal.  An allele whose read group
 * is not in the map is the reference's exit(1): OTG_ERR_ARG.  truth != 0 (local_parse_analleles): only records whose name starts with the
 * chromosome are looked at, and each of them appends its `sp:A` value to `spannings` (u or absent -1, b 0, l 1, r 2, n 3, anything else
 * nothing) whether or not its `ta` tag selects it — so spannings[i] need not belong to allele i, as in the reference.  first_spanning has
 * n_regions + 1 entries (in-out counter *n_spannings).  The query side (truth == 0) is parse_analleles.  Regions whose query fails add
 * "WARNING: query failed at region chr:start-end\n" to `warn` (nullable; in-out *warn_len).  Otherwise as otg_ingest_alleles. */
int otg_ingest_compare_alleles(otg_bam* bam, const char* sample0, const char* sample1, int32_t truth, const otg_bed* beds, const char* chr_arena,
                               uint32_t n_regions, int32_t threads, uint8_t* arena, uint64_t arena_capacity, uint64_t* arena_used,
                               otg_allele* alleles, uint32_t alleles_capacity, uint32_t* n_alleles, uint32_t* first_allele,
                               int32_t* spannings, uint32_t spannings_capacity, uint32_t* n_spannings, uint32_t* first_spanning,
                               char* warn, uint64_t warn_capacity, uint64_t* warn_len);
typedef struct otg_compare_counts {
  uint64_t n_compared;           /* regions that printed their two lines                             */
  uint64_t skip_many_truth;      /* > 2 truth alleles                                                 */
  uint64_t skip_one_truth;       /* 1 truth allele                                                    */
  uint64_t skip_no_truth;        /* 0 truth alleles                                                   */
  uint64_t skip_no_query;        /* 0 query alleles                                                   */
} otg_compare_counts;
/* The region logic of compare() (src/compare.cpp:106-146) on ingested alleles: host code.  Region r has truth alleles
 * truth[truth_first[r] .. truth_first[r+1]), spanning values spannings[span_first[r] ..), query alleles likewise.  A region with exactly two
 * truth alleles and at least one query allele has 2 x max(n_query, 2) pairs (the single query allele is duplicated), truth-major, at
 * pair_first[r] ..: pair_edit / pair_ops = edit distance and alignment columns of truth i against query j aligned end-to-end with the longer
 * one as the pattern (ties: the query) — otg_edit_align_batch.  Pairs the reference does not align (equal alleles, "N" / "NDNNN") take their
 * fixed values here, whatever the arrays hold.  Every other region is skipped with the reference's warning line (no timestamp) in `warn`.
 * Output lines: region, truth length, query length, spanning, edit, ops (the two doubles as ostream prints them: %g).  A spanning index past
 * the values the region pushed prints -1 (the reference reads outside its vector there).  Same buffer protocol as otg_emit_alleles for both
 * buffers (warn nullable). */
int otg_compare_emit(const otg_bed* beds, const char* chr_arena, uint32_t n_regions,
                     const uint32_t* truth_first, const otg_allele* truth, const uint8_t* truth_seqs,
                     const uint32_t* span_first, const int32_t* spannings,
                     const uint32_t* query_first, const otg_allele* query, const uint8_t* query_seqs,
                     const uint64_t* pair_first, const double* pair_edit, const double* pair_ops,
                     char* out, uint64_t out_capacity, uint64_t* out_len,
                     char* warn, uint64_t warn_capacity, uint64_t* warn_len, otg_compare_counts* counts);
/* `otter compare` from files to text in one call — compare() (src/compare.cpp:68-150): BED regions in bounded batches through the two ingests
 * (host threads), the edit alignments of all pairs of a batch on the device (otg_edit_align_batch; otg_edit_align_heur_batch when the job
 * names OTG_HEURISTIC_WFADAPTIVE — a zeroed job is exact), and otg_compare_emit; text in BED
 * order (the reference's threads interleave theirs).  The ingest of the next batch overlaps the device work and the emit of the current one.
 * warn (nullable) receives the reference's warning lines without the timestamp.  stats: n_regions_ok = compared regions, n_regions_skipped
 * the rest, n_alleles = truth + query alleles, n_reads = aligned pairs. */
typedef struct otg_compare_job {
  const char* truth_bam_path;    /* first positional <BAM>: the truth alleles                        */
  const char* query_bam_path;    /* second positional <BAM>: the assembled alleles                   */
  const char* bed_path;          /* -b                                                               */
  int32_t     threads;           /* -t: host threads of the ingest                                   */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_regions;     /* regions per batch, 0 = 1024                                      */
  uint32_t    reserved;
  otg_write_fn warn;             /* nullable                                                         */
  void*       warn_user;
  int32_t     heuristic;         /* of the edit alignments: OTG_HEURISTIC_NONE (0, exact) or OTG_HEURISTIC_WFADAPTIVE with the three below */
  int32_t     heur_min_wavefront_length;
  int32_t     heur_max_distance_threshold;
  int32_t     heur_steps_between_cutoffs;
} otg_compare_job;
int otg_compare_files(const otg_compare_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * `otter vcf2mat` (src/vcf2mat.cpp, src/command_vcf2mat.cpp): one row of k-mer usage per allele of a VCF.
 * ------------------------------------------------------------------------------------------- */
#define OTG_KMER_MAX 12          /* largest supported k (the reference accepts 32)      */
typedef struct otg_vcf otg_vcf;
typedef struct otg_vcf_record {
  uint64_t region_off;           /* the ID column (vcf2mat's region string) in the region arena      */
  uint32_t region_len;
  uint32_t first_allele;         /* index of allele 0 (REF) in the batch's allele arrays             */
  uint32_t n_alleles;            /* REF + the ALT alleles                                            */
  uint32_t reserved;
} otg_vcf_record;
/* Replaces GZIPiter (src/angzipiter.hpp) on a VCF: plain text, gzip or BGZF through zlib's gz* reader. */
int  otg_vcf_open(const char* path, otg_vcf** out);
void otg_vcf_close(otg_vcf* v);
/* Replaces the line loop and parse_alleles of vcf2mat (src/vcf2mat.cpp:16-36,57-65): the next records of the file, in file order, as many as
 * fit the capacities.  Lines starting with '#' are skipped; a line is split on '\t' with std::getline semantics (a trailing empty field is
 * dropped); column 3 is the region, column 4 (REF) allele 0, column 5 (ALT) adds nothing when it is ".", the allele "N" when it is exactly
 * "<DEL>", else its ','-separated fields (getline semantics again).  A line with fewer than 4 columns gives no record.  Unlike the reference, a
 * last line without '\n' is read and lines may be longer than 1 MB.  Alleles are packed in seq_arena at seq_off[i], length seq_len[i]; region
 * strings in region_arena.  *n_records == 0 at the end of the file.  OTG_ERR_CAPACITY when even the next record does not fit: the counters
 * then hold what it alone needs, and it is returned by the next call.  *bytes_in (nullable) += the text bytes consumed. */
int  otg_vcf_read_alleles(otg_vcf* v, otg_vcf_record* records, uint32_t records_capacity, uint32_t* n_records,
                          char* region_arena, uint64_t region_capacity, uint64_t* region_used,
                          uint64_t* seq_off, uint32_t* seq_len, uint32_t alleles_capacity, uint32_t* n_alleles,
                          uint8_t* seq_arena, uint64_t arena_capacity, uint64_t* arena_used, uint64_t* bytes_in);
/* Replaces the output of vcf2mat (src/vcf2mat.cpp:66-72): per allele a of record r, the row
 * region \t i \t gc[a] \t seq_len[a] \t hsd[a] (\t usage[a][b] for the 4^k+1 bins) \n, with a = records[r].first_allele + i.  Doubles as
 * std::cout prints them (%g); every NaN prints "-nan", as the reference's 0/0 does on x86-64.  Same buffer protocol as otg_emit_alleles. */
int  otg_vcf2mat_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len, int32_t k,
                      const double* usage, const double* gc, const double* hsd, char* out, uint64_t out_capacity, uint64_t* out_len);
/* `otter vcf2mat` from a file to text in one call (src/vcf2mat.cpp:48-77): the BED is parsed and filters nothing; records in bounded batches
 * (sized by the bytes of a row, so that k = 12 fits), otg_kmer_usage_batch on the device, the rows formatted by `threads` host threads and
 * written in file order.  Reading the next batch overlaps the device pass and the emit of the current one.  stats: n_regions = records,
 * n_alleles, input_bytes = VCF text bytes, output_bytes, ms_ingest = reading, ms_hot_path = device, ms_emit = formatting. */
typedef struct otg_vcf2mat_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, parsed, unused (as in the reference)               */
  int32_t     k;                 /* -k: 1..OTG_KMER_MAX                                               */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = sized from k                              */
} otg_vcf2mat_job;
int otg_vcf2mat_files(const otg_vcf2mat_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Cohort: sample BAMs to one joint VCF, the alleles staying in HBM between `otter assemble` and `otter genotype`.  The reference's workflow
 * writes the allele records of every sample as SAM text (src/assemble.cpp:143-149), merges the per-sample BAMs outside otter and reads them
 * back (parse_analleles, src/anseqs.cpp:462-524; genotype_process, src/genotype.cpp:80-157).  Here, for one batch of regions:
 *   otg_cohort_begin     opens a staging area for n_regions regions and n_samples samples on ctx;
 *   otg_cohort_stage     after otg_assemble_run on src_ctx (ctx itself or another context on the same device) over the SAME n_regions regions:
 *                        copies that run's allele records and bytes device to device as sample `sample` (each sample once, any order);
 *                        src_ctx may run its next batch as soon as the call returns;
 *   otg_cohort_regroup   all samples staged: uploads the reference alleles (region r: ref_arena + ref_off[r], ref_len[r] bytes — what
 *                        genotype_process fetches, bases [start - offset_l, end + offset_r - 1], src/genotype.cpp:93-101) and regroups on the
 *                        device into the inputs of anallele_cluster: region-major; inside a region sample-major in sample order, the alleles of
 *                        a sample in label order, the reference allele last with sample index n_samples.  A region in which no sample has an
 *                        allele has no alleles at all (src/genotype.cpp:90); a zero-length allele becomes "N" (src/anseqs.cpp:505-507);
 *   otg_cohort_genotype  anallele_cluster on the regrouped buffers (the kernels of otg_genotype_cluster_batch; gt_max_error, gt_max_cosdis);
 *   otg_genotype_cohort_metric  the same under a metric (otg_genotype_cluster_metric_batch: OTG_GT_METRIC_EDIT aligns the alleles in HBM,
 *                        exactly, whatever heuristic the assemble runs left on the context); everything after it works unchanged;
 *   otg_cohort_collect   D2H; every output is nullable.  first_allele_out has n_regions + 1 entries; alleles_out are the records in regrouped
 *                        order as otg_ingest_alleles would deliver them (.seq_off into seq_out, .region = batch-local region, .label = sample
 *                        index); sample_out / seq_off_out / seq_len_out are the arrays the kernels read; gt .. reps as
 *                        otg_genotype_cluster_batch returns them (they need otg_cohort_genotype, the others only otg_cohort_regroup).
 *                        Sizes: otg_cohort_result_sizes; OTG_ERR_CAPACITY when a capacity is smaller;
 *   otg_cohort_end       closes the batch; the staging buffers stay with the context for the next one.
 * ------------------------------------------------------------------------------------------- */
int otg_cohort_begin(otg_ctx* ctx, uint32_t n_regions, uint32_t n_samples);
int otg_cohort_stage(otg_ctx* ctx, otg_ctx* src_ctx, uint32_t sample);
int otg_cohort_regroup(otg_ctx* ctx, const uint8_t* ref_arena, uint64_t ref_bytes, const uint64_t* ref_off, const uint32_t* ref_len);
int otg_cohort_genotype(otg_ctx* ctx, const otg_params* params);      /* = otg_genotype_cohort_metric(.., OTG_GT_METRIC_LENGTH) */
int otg_genotype_cohort_metric(otg_ctx* ctx, const otg_params* params, int32_t metric);
int otg_cohort_result_sizes(otg_ctx* ctx, uint32_t* n_alleles, uint64_t* seq_bytes);
int otg_cohort_collect(otg_ctx* ctx, uint32_t* first_allele_out, otg_allele* alleles_out, uint32_t allele_capacity, int32_t* sample_out,
                       uint64_t* seq_off_out, uint32_t* seq_len_out, uint8_t* seq_out, uint64_t seq_capacity,
                       int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out, int32_t* n_gt_out, int32_t* reps_out);
int otg_cohort_end(otg_ctx* ctx);

/* The k-mer usage matrix of the joint alleles (`otter vcf2mat` on the VCF of this batch, src/vcf2mat.cpp:23-46,66-72) without the VCF in
 * between: after otg_cohort_genotype the alleles of every VCF line are selected on the device and the k-mer tiers of otg_kmer_usage_batch read
 * them in the regrouped arena, in place.
 *   otg_kmer_cohort_rows   builds the row list of the open, clustered batch (OTG_ERR_ARG "has not been clustered" before otg_cohort_genotype).
 *                          A region with alleles contributes n_gt rows, the alleles of its VCF line in column order: row 0 its reference
 *                          allele (the REF column), row i >= 1 the representative of ALT i (src/genotype.cpp:149-153).  A zero-length allele is
 *                          the row of "N", as vcf2mat reads a lone <DEL> back (beside other ALT alleles vcf2mat counts the text "<DEL>" itself:
 *                          otg_cohort_files substitutes that row in its matrix text, these building blocks do not).  *n_rows = the rows of the batch; row_first_out (n_regions + 1):
 *                          the first row of every region; row_allele_out (n_rows): the row's allele, an index into the arrays of
 *                          otg_cohort_collect; sample_gt_out (n_regions x n_samples x 2): the two GT numbers the VCF prints for a sample, -1 -1
 *                          where it prints ./. and in regions without alleles.  Every output is nullable; the list is built once per
 *                          otg_cohort_genotype, so a first call may ask for *n_rows alone.
 *   otg_kmer_cohort_usage  rows [row_begin, row_begin + n) through the tiers of otg_kmer_usage_batch (builds the row list when it has not been
 *                          built): usage_out n x (4^k + 1), gc_out n, hsd_out n; nullable, NULL leaves them in HBM for
 *                          otg_kmer_usage_device_results(ctx, n, k, ..) and otg_kmer_usage_last_ms.  k outside 1..OTG_KMER_MAX and a range past
 *                          *n_rows are OTG_ERR_ARG; rows beyond the 4 GiB workspace (about 21 at k = 12) are OTG_ERR_CAPACITY before anything is
 *                          allocated: the caller walks the row list in ranges.
 *   otg_kmer_cohort_device_rows  device pointers of the row list (valid until the next otg_cohort_regroup or otg_destroy): row_first
 *                          (n_regions + 1), row_allele (n_rows), sample_gt (n_regions x n_samples x 2).  Every output is nullable. */
int otg_kmer_cohort_rows(otg_ctx* ctx, uint32_t* n_rows, uint32_t* row_first_out, uint32_t* row_allele_out, int32_t* sample_gt_out);
int otg_kmer_cohort_usage(otg_ctx* ctx, int32_t k, uint32_t row_begin, uint32_t n, double* usage_out, double* gc_out, double* hsd_out);
int otg_kmer_cohort_device_rows(otg_ctx* ctx, uint32_t* n_rows, const uint32_t** row_first, const uint32_t** row_allele, const int32_t** sample_gt);

/* Sample BAMs + BED + reference FASTA to one joint VCF in one call: per batch of regions and per sample, read ingest on host threads ->
 * otg_assemble_submit / run -> otg_cohort_stage; then otg_cohort_regroup / genotype / collect and the VCF text (otg_emit_vcf_header with the
 * contigs of the FIRST BAM and one column per sample name, otg_emit_vcf_lines), in BED order.  The ingest of a sample overlaps the device run of
 * the previous one (two contexts per device, as in otg_assemble_files); BED sharding over devices[] and the batch plan as otg_assemble_files.
 * The text equals what otg_genotype_files prints for the merged allele BAM of the per-sample otg_assemble_files runs with read_group =
 * sample_names[s].  OTG_ERR_ARG, with the offending item in otg_last_error(NULL): no samples, an empty or repeated sample name, no FASTA, a BAM
 * whose targets differ from the first BAM's, two BED records with the same chr:start-end (the file round trip would hand each of them the alleles
 * of both; this path identifies regions by index).
 * allele_write (nullable): receives per sample the SAM text otg_assemble_files would have written for it (header first, records in BED order);
 * when NULL no SAM text is formatted and the allele records are never copied to the host.
 * matrix_write (nullable; matrix_user, matrix_k): receives the k-mer usage matrix of the joint alleles, the text otg_vcf2mat_files prints for
 * the VCF of this call at k = matrix_k (rows in BED order, the region string = the ID column chr:start-end), from otg_kmer_cohort_rows /
 * otg_kmer_cohort_usage on the batch while it is still in HBM.  matrix_k outside 1..OTG_KMER_MAX with a writer set is OTG_ERR_ARG with vcf2mat's
 * message.  With matrix_write NULL no k-mer work is done.
 * stats: n_reads = reads ingested over all samples, n_alleles = staged alleles (reference alleles excluded), n_regions_ok = regions with a VCF
 * line, ms_ingest / ms_hot_path / ms_emit = busy times summed over their threads; output_bytes = the VCF text (the matrix is not counted). */
typedef int (*otg_cohort_allele_write_fn)(void* user, uint32_t sample, const char* data, uint64_t len);
typedef struct otg_cohort_job {
  uint32_t    n_samples;
  uint32_t    batch_regions;     /* regions per batch; 0 = the plan of otg_assemble_files                                   */
  const char* const* bam_paths;  /* n_samples reads BAMs (index <BAM>.bai)                                                 */
  const char* const* sample_names; /* the -R of each assemble = the VCF column names: unique, non-empty                    */
  const char* bed_path;          /* -b                                                                                     */
  const char* fasta_path;        /* -r: required (local re-alignment flanks AND the reference alleles)                     */
  otg_params  params;            /* assemble heuristics and gt_max_error / gt_max_cosdis (realign is set by the library)   */
  otg_ingest_opts ingest;        /* one --offset pair for the whole cohort (one `OF:` header line carries it); .threads = host ingest threads */
  int32_t     n_devices;         /* 0: device 0 only                                                                       */
  int32_t     gt_metric;         /* of the joint genotyping: OTG_GT_METRIC_LENGTH (0) or OTG_GT_METRIC_EDIT; other values: OTG_ERR_ARG */
  const int32_t* devices;        /* HIP device ordinals, one contiguous BED shard each                                     */
  otg_cohort_allele_write_fn allele_write;   /* nullable                                                                   */
  void*       allele_user;
  otg_write_fn matrix_write;     /* nullable: the k-mer usage matrix of the joint alleles                                   */
  void*       matrix_user;
  int32_t     matrix_k;          /* 1..OTG_KMER_MAX when matrix_write is set                                               */
  int32_t     reserved2;
} otg_cohort_job;
int otg_cohort_files(const otg_cohort_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Tandem-repeat motif annotation of alleles: which unit, how many copies, how pure.  The reference has no counterpart; this is the
 * definition (all integers).  For a sequence s of length L, 1 <= max_period <= OTG_MOTIF_MAX_PERIOD and a slack in per mille,
 * 0 <= slack <= 999:
 *   1. c[i] = 0..3 for A/a C/c G/g T/t, 4 for any other byte (the table of otg_kmer_usage_batch);
 *   2. P = min(max_period, L / 2);
 *   3. m(p) = #{ i in [0, L - p) : c[i] == c[i + p] and c[i] < 4 } for p in 1..P;
 *   4. best = 1, then for p = 2..P ascending: best = p when m(p) (L - best) > m(best) (L - p) (strict: ties keep the smaller period);
 *   5. period = the smallest p in 1..best with m(p) (L - best) 1000 >= (1000 - slack) m(best) (L - p).  (Without the slack one substitution
 *      in (CAG)20 makes p = 30 the best period: its window avoids the mismatch twice.)
 *   6. P == 0 or m(best) == 0: period = matches = compared = best_period = 0 and the unit is empty (L < 2, an all-N allele, "AC");
 *   7. unit[j], j < period: the majority base over the ACGT bytes at i = j (mod period); ties to the lower code (A < C < G < T); a phase
 *      without an ACGT byte gives 'N';
 *   8. the unit is reported as its lexicographically smallest rotation by byte value, ties to the smallest rotation offset;
 *   9. matches = m(period), compared = L - period, best_period = best; copies = L / period and purity = matches / compared are the caller's;
 *  10. L > OTG_MOTIF_MAX_LEN (the bound that keeps step 5 inside 64 bits): period = 0 and flags = OTG_MOTIF_TOO_LONG; the batch does not fail.
 * A shifted self-comparison is not indel-tolerant: the targets are assembled alleles (consensus sequences), not noisy reads.
 *   otg_motif_batch           allele i is seq_arena[seq_off[i] .. + seq_len[i]).  out: n records; unit i: period bytes at unit_out + i * unit_stride
 *                             (the rest of a slot is zero).  unit_stride < min(max_period, max(seq_len) / 2), max_period or slack out of range:
 *                             OTG_ERR_ARG.  NULL outputs leave the results in HBM.  At most 2^24 alleles per call (OTG_ERR_CAPACITY);
 *   otg_motif_device_results  device pointers of the latest results on this context (n records, then n x unit_stride unit bytes), valid until
 *                             the next motif call on the context or otg_destroy; every output is nullable;
 *   otg_motif_last_ms         HIP-event times (ms) of the latest motif call: count_ms = the pack and match-count kernels, reduce_ms = the reduce
 *                             and unit kernel;
 *   otg_motif_cohort          the same kernels over rows [row_begin, row_begin + n) of the row list of otg_kmer_cohort_rows, the alleles read in the
 *                             regrouped cohort arena in place (as otg_kmer_cohort_usage: not clustered or a range past *n_rows is OTG_ERR_ARG; a
 *                             zero-length allele is the row of "N");
 *   otg_motif_emit            per allele a of record r the row region \t i \t seq_len[a] \t period \t unit \t copies \t purity \n with
 *                             a = records[r].first_allele + i: unit "." when period == 0, copies "%.2f" of seq_len / period (0.00 when period
 *                             == 0), purity "%.4f" of matches / compared (0.0000 when period == 0).  Buffer protocol of otg_emit_alleles.
 * The device sweeps all periods of an allele with planes of 32 bases per word; OTG_MOTIF_WIDE=1 in the environment (read once per process)
 * sends every allele through the tier that keeps the planes in HBM.
 * ------------------------------------------------------------------------------------------- */
#define OTG_MOTIF_MAX_PERIOD 4096
#define OTG_MOTIF_MAX_LEN    1048575
#define OTG_MOTIF_LDS_LEN    32768       /* alleles up to this length keep their planes in LDS, longer ones in HBM */
#define OTG_MOTIF_TOO_LONG   1u          /* otg_motif.flags */
typedef struct otg_motif {
  uint32_t period;               /* 0: no repeat found                                               */
  uint32_t matches;              /* m(period)                                                        */
  uint32_t compared;             /* L - period                                                       */
  uint32_t best_period;          /* the period of the highest match ratio (step 4)                   */
  uint32_t flags;                /* OTG_MOTIF_TOO_LONG                                               */
  uint32_t reserved;
} otg_motif;
int otg_motif_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                    uint32_t n, uint32_t max_period, uint32_t slack, otg_motif* out, uint8_t* unit_out, uint32_t unit_stride);
int otg_motif_device_results(otg_ctx* ctx, uint32_t* n, const otg_motif** records, const uint8_t** units, uint32_t* unit_stride);
int otg_motif_last_ms(otg_ctx* ctx, double* count_ms, double* reduce_ms);
int otg_motif_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, uint32_t max_period, uint32_t slack, otg_motif* out, uint8_t* unit_out,
                     uint32_t unit_stride);
int otg_motif_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len, const otg_motif* motifs,
                   const uint8_t* units, uint32_t unit_stride, char* out, uint64_t out_capacity, uint64_t* out_len);
/* One row of otg_motif_emit per allele of a VCF, in file order: built on otg_vcf_open / otg_vcf_read_alleles and the batching of
 * otg_vcf2mat_files (same record and allele rules; the BED is parsed and filters nothing; reading the next batch overlaps the device pass and
 * the emit of the current one).  max_period and slack as above; out-of-range values are OTG_ERR_ARG with the message the tool
 * prints.  stats as otg_vcf2mat_files. */
typedef struct otg_motifs_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, parsed, unused                                     */
  uint32_t    max_period;        /* -p: 1..OTG_MOTIF_MAX_PERIOD (the tool's default: 256)            */
  uint32_t    slack;             /* --slack: 0..999 per mille (the tool's default: 50)               */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = 65536                                     */
  uint32_t    reserved;
} otg_motifs_job;
int otg_motifs_files(const otg_motifs_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Repeat structure of alleles: every allele as a left-to-right sequence of exact tandem repeats and literals, (CAG)20(CCG)20 or
 * (CGG)10AGG(CGG)9.  The motif annotation above gives an allele one period; it cannot say where a repeat starts, where it stops, or that
 * the unit changes along the way.  The reference has no counterpart; this is the definition (all integers).  Parameters:
 * 1 <= max_period <= OTG_REPEAT_MAX_PERIOD, 2 <= min_copies <= 1024, 2 <= min_span <= 65535 bases.  For a sequence s of length L:
 *   1. Codes.  c[i] = 0..3 for A/a C/c G/g T/t, 4 for any other byte (the motif table); P = min(max_period, L / 2).
 *   2. Match bits.  e_p[i] = (c[i] == c[i + p] and c[i] < 4) for i in [0, L - p), p in 1..P (the bits whose number is m(p) above).
 *   3. Runs.  A run of period p is a maximal interval [a, b) of ones in e_p; it covers the bases [a, e) with e = b + p: that stretch has
 *      exact period p and all of it is ACGT.  A copy count k at period p is ENOUGH when k >= min_copies and k p >= min_span.  A run is kept
 *      when k = (e - a) / p is enough; R is the set of kept runs (p, a, e) over all p.
 *   4. best(lo, hi).  For every run (p, a, e) in R: st = max(a, lo), en = min(e, hi), k = (en - st) / p; the run is skipped when en <= st or
 *      k is not enough.  Its gain is g = st - lo + k p, its cost w = st - lo + p.  The best run has the highest g / w, compared by
 *      cross-multiplication in 64 bits; ties go to the smaller st, then to the smaller p (two runs never share (st, p): a total order).
 *      best may be none.
 *   5. Parse.  x = 0, H = L, an empty stack, prev = none.  Loop on b = best(x, H):
 *        b is none:  emit the literal [x, H) and set x = H; stop when the stack is empty, otherwise pop (run, H'), set H = H' and place
 *                    the run at x;
 *        b.st > x:   push (b's run, H) and set H = b.st (the gap in front of the run is parsed first, under that horizon);
 *        otherwise:  place b's run at x; H stays.
 *   6. Placing the run (p, a, e) at x under the horizon H.  en = min(e, H), st = x.  If prev has the same period p and begins at pb: take
 *      the smallest t in [x, min(x + p, en - p + 1)) with c[t .. t + p) == c[pb .. pb + p); st = t if such a t exists and (en - t) / p is
 *      still enough.  (This keeps the unit's phase across an interruption: (CGG)10AGG(CGG)9, not (CGG)10A(GGC)9GG.)  Emit the literal
 *      [x, st), then the repeat (begin = st, period = p, copies = k = (en - st) / p, length = k p); prev = (p, st) and x = st + k p.
 *   7. Literals.  Adjacent literals merge; an empty literal is not emitted; a literal is (begin, period 0, copies 0, length).
 *   8. Per allele the summary n_segments, n_repeats, covered = the sum of the repeat lengths, flags.  L > OTG_REPEAT_MAX_LEN: one literal
 *      [0, L) and flags = OTG_REPEAT_TOO_LONG; the batch does not fail.  L = 0: no segments.
 * It follows that the segments tile [0, L) in order, that expanding unit x copies and the literals gives the allele back up to letter case,
 * and that no two literals are adjacent.  Runs are exact: a substitution inside a copy shows as a literal of one unit, an indel re-phases
 * the run behind it.
 *   otg_repeat_batch           allele i is seq_arena[seq_off[i] .. + seq_len[i]).  sums: n summaries; seg_off: n + 1 offsets into the segments,
 *                              which stay in HBM; *n_segments = seg_off[n].  Every output is nullable.  A parameter out of range or an
 *                              allele outside the arena: OTG_ERR_ARG.  At most 2^24 alleles per call (OTG_ERR_CAPACITY);
 *   otg_repeat_collect         copies the segments of the latest call on the context to segs[0 .. total); capacity < total is
 *                              OTG_ERR_CAPACITY with the needed count in the message;
 *   otg_repeat_device_results  device pointers of the latest results on this context (n summaries, n + 1 offsets, total segments), valid
 *                              until the next repeat call on the context or otg_destroy; every output is nullable;
 *   otg_repeat_last_ms         HIP-event times (ms) of the latest repeat call: runs_ms = pack, count, scans and run write (with the host's
 *                              read of the run total in between), select_ms = the parse and the compaction of the segments;
 *   otg_repeat_cohort          the same kernels over rows [row_begin, row_begin + n) of the row list of otg_kmer_cohort_rows, the alleles read
 *                              in the regrouped cohort arena in place (preconditions and refusals as otg_motif_cohort; a zero-length allele
 *                              is the row of "N");
 *   otg_repeat_emit            per allele a = records[r].first_allele + i the row region \t i \t seq_len[a] \t n_repeats \t covered \t
 *                              structure \n.  structure is the concatenation of the segments of the allele (segs[seg_off[a] ..
 *                              seg_off[a + 1])), "." when there are none: a repeat is (UNIT)copies with the unit's bases written through the
 *                              code table (upper case), a literal its own bytes when its length is at most OTG_REPEAT_TEXT_LITERAL, else
 *                              [length].  A segment outside its allele is OTG_ERR_ARG.  Buffer protocol of otg_emit_alleles.
 * The planes and their two tiers are those of the motif annotation, OTG_MOTIF_WIDE included.
 * ------------------------------------------------------------------------------------------- */
#define OTG_REPEAT_MAX_PERIOD   4096
#define OTG_REPEAT_MAX_LEN      1048575
#define OTG_REPEAT_TOO_LONG     1u       /* otg_repeat_sum.flags */
#define OTG_REPEAT_TEXT_LITERAL 24       /* a longer literal is written [length] by otg_repeat_emit */
typedef struct otg_repeat_seg {
  uint32_t begin;                /* first base of the segment                                        */
  uint32_t period;               /* 0: a literal                                                     */
  uint32_t copies;               /* whole copies of the unit s[begin .. begin + period); 0: a literal */
  uint32_t length;               /* bases; period * copies for a repeat                              */
} otg_repeat_seg;
typedef struct otg_repeat_sum {
  uint32_t n_segments;
  uint32_t n_repeats;
  uint32_t covered;              /* bases in repeat segments                                         */
  uint32_t flags;                /* OTG_REPEAT_TOO_LONG                                              */
} otg_repeat_sum;
int otg_repeat_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                     uint32_t n, uint32_t max_period, uint32_t min_copies, uint32_t min_span, otg_repeat_sum* sums, uint64_t* seg_off,
                     uint64_t* n_segments);
int otg_repeat_collect(otg_ctx* ctx, otg_repeat_seg* segs, uint64_t capacity);
int otg_repeat_device_results(otg_ctx* ctx, uint32_t* n, const otg_repeat_sum** sums, const uint64_t** seg_off, const otg_repeat_seg** segs,
                              uint64_t* total);
int otg_repeat_last_ms(otg_ctx* ctx, double* runs_ms, double* select_ms);
int otg_repeat_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, uint32_t max_period, uint32_t min_copies, uint32_t min_span,
                      otg_repeat_sum* sums, uint64_t* seg_off, uint64_t* n_segments);
int otg_repeat_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint8_t* seq_arena, const uint64_t* seq_off,
                    const uint32_t* seq_len, const otg_repeat_sum* sums, const uint64_t* seg_off, const otg_repeat_seg* segs, char* out,
                    uint64_t out_capacity, uint64_t* out_len);
/* One row of otg_repeat_emit per allele of a VCF, in file order, built exactly as otg_motifs_files is.  Out-of-range parameters are
 * OTG_ERR_ARG with the message the tool prints.  stats as otg_vcf2mat_files. */
typedef struct otg_repeats_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, parsed, unused                                     */
  uint32_t    max_period;        /* -p: 1..OTG_REPEAT_MAX_PERIOD (the tool's default: 256)           */
  uint32_t    min_copies;        /* --min-copies: 2..1024 (the tool's default: 2)                    */
  uint32_t    min_span;          /* --min-span: 2..65535 bases (the tool's default: 12)              */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = 65536                                     */
} otg_repeats_job;
int otg_repeats_files(const otg_repeats_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Indel-tolerant copy numbers: an allele aligned to a cyclic repeat unit.  The two annotations above compare an allele with itself, so one
 * inserted base moves every later copy out of phase.  Here the allele is aligned against a given unit repeated without end, free in where
 * it starts and stops on the unit (the wraparound dynamic programme), which gives the edit count and the number of unit bases spanned
 * whatever indels lie in between.  The reference has no counterpart; this is the definition (all integers).  For a sequence s
 * of length L and a unit u of length p, 1 <= p <= OTG_UNITALIGN_MAX_UNIT:
 *   1. Codes.  c = 0..3 for A/a C/c G/g T/t, 4 for any other byte (the motif table).  Code 4 matches nothing, in s or in u, not even
 *      another 4.
 *   2. Let t range over the substrings of u repeated infinitely, the empty one included.  edits = the minimum over t of the unit-cost edit
 *      distance between s and t; unit_bases = the length of the shortest t that reaches that minimum.
 *   3. end_phase comes from this DP.  Cell (i, j) is "i bases of s consumed, the next unit base is u[j]"; its key is
 *      edits * 2^32 + unit_bases.
 *        V[0][j] = 0 for every j;
 *        the diagonal step:              V[i+1][(j+1) % p] <= V[i][j] + (c_s[i] == c_u[j] && c_s[i] < 4 ? 0 : 2^32) + 1;
 *        a base of s outside the unit:   V[i+1][j] <= V[i][j] + 2^32;
 *        a skipped unit base:            V[i][(j+1) % p] <= V[i][j] + 2^32 + 1, taken to its least fixed point around the cycle;
 *      end_phase = the smallest j with V[L][j] minimal; (edits, unit_bases) are the fields of that minimum.
 *   4. The start phase follows as (end_phase - unit_bases) mod p and is not stored.
 *   5. L = 0: (0, 0, 0).
 *   6. p = 0: zeros and flags = OTG_UNITALIGN_NO_UNIT.
 *   7. L > OTG_UNITALIGN_MAX_LEN: zeros and flags = OTG_UNITALIGN_TOO_LONG; the batch does not fail.
 *   8. p > OTG_UNITALIGN_MAX_UNIT: OTG_ERR_ARG when the caller passes the unit in; zeros and flags = OTG_UNITALIGN_UNIT_TOO_LONG when the
 *      unit comes from the motif annotation (max_period goes to OTG_MOTIF_MAX_PERIOD there).
 * It follows that edits <= L, that unit_bases <= L + edits, that rotating the unit changes only end_phase, and that letter case changes
 * nothing.  copies = unit_bases / p and identity = 1 - edits / max(L, unit_bases) are the caller's.
 *   otg_unitalign_batch           allele i is seq_arena[seq_off[i] .. + seq_len[i]) as in otg_motif_batch; unit k is unit_arena[unit_off[k] ..
 *                                 + unit_len[k]); task t aligns allele task_seq[t] to unit task_unit[t].  out: n_tasks records, NULL leaves
 *                                 them in HBM.  An index out of range, a unit over OTG_UNITALIGN_MAX_UNIT bytes, an allele or a unit outside
 *                                 its arena: OTG_ERR_ARG.  More than 2^24 tasks: OTG_ERR_CAPACITY;
 *   otg_unitalign_motifs          task i = allele i of the latest motif call on the context (otg_motif_batch / otg_motif_cohort) against that
 *                                 call's unit i; both are read where they lie in HBM.  No motif results on the context: OTG_ERR_ARG;
 *   otg_unitalign_cohort          rows [row_begin, row_begin + n) of the row list of otg_kmer_cohort_rows, the alleles read in the regrouped
 *                                 cohort arena in place (preconditions and refusals as otg_motif_cohort).  unit_arena == NULL: task i = row
 *                                 row_begin + i against unit i of the latest otg_motif_cohort, which must have covered the same rows.
 *                                 Otherwise the caller's units and task lists as in otg_unitalign_batch, task_seq relative to row_begin;
 *   otg_unitalign_device_results  the device pointer of the latest records on this context, valid until the next unit alignment on the
 *                                 context or otg_destroy; every output is nullable;
 *   otg_unitalign_last_ms         HIP-event time (ms) of the latest call: the binning and the alignment kernels;
 *   otg_parse_bed_units           the units of a tandem-repeat catalogue: record i is record i of otg_parse_bed_file on the same file.  When
 *                                 column 4 holds `MOTIFS=` at its start or after a `;` the value up to the next `;` is taken, otherwise the
 *                                 whole field; it is split on `,`.  If every item is 1..OTG_UNITALIGN_MAX_UNIT bytes of ACGTNacgtn the items
 *                                 are the record's units in that order (duplicates kept); otherwise, and with fewer than four columns, the
 *                                 record has none (the column is a name).  rec_first[i] .. rec_first[i + 1] are the units of record i
 *                                 (rec_first has *n_records + 1 entries); capacities too small: OTG_ERR_CAPACITY with the needs in the outputs;
 *   otg_unitalign_emit            per task t the row region \t i \t seq_len \t source \t unit \t edits \t unit_bases \t copies \t identity \n.
 *                                 The tasks of allele a = records[r].first_allele + i are task_first[a] .. task_first[a + 1] (one entry per
 *                                 allele and one more), in that order.  source = "bed" or "motif" (task_source[t] = OTG_UNITALIGN_SOURCE_*),
 *                                 unit = the task_unit_len[t] bytes at unit_arena + task_unit_off[t] as given ("." when there are none),
 *                                 copies "%.2f" of unit_bases / p and identity "%.4f" of 1 - edits / max(seq_len, unit_bases); both are 0.00 /
 *                                 0.0000 when the denominator is 0 or a flag is set.  Buffer protocol of otg_emit_alleles.
 * The row lives in registers, unit positions across lanes; a task takes 4 .. 64 lanes by its unit length, so a wave carries up to sixteen.
 * Alleles up to OTG_UNITALIGN_NARROW_LEN keep the key in 32 bits (two 16-bit fields; the bound is derived in otg_unitalign_core.hpp from
 * every value a lane can hold).  OTG_UNITALIGN_WIDE=1 sends every task through the 64-bit tier, OTG_UNITALIGN_SEG64=1 gives every task a
 * whole wave (both read once per process).
 * ------------------------------------------------------------------------------------------- */
#define OTG_UNITALIGN_MAX_UNIT      256
#define OTG_UNITALIGN_MAX_LEN       1048575
#define OTG_UNITALIGN_NARROW_LEN    ((65535 - 2 * OTG_UNITALIGN_MAX_UNIT + 1) / 2)   /* 32512: the longest allele of the 32-bit key */
#define OTG_UNITALIGN_NO_UNIT       1u   /* otg_unitalign.flags */
#define OTG_UNITALIGN_TOO_LONG      2u
#define OTG_UNITALIGN_UNIT_TOO_LONG 4u
#define OTG_UNITALIGN_SOURCE_BED    0u
#define OTG_UNITALIGN_SOURCE_MOTIF  1u
typedef struct otg_unitalign {
  uint32_t edits;                /* the fewest edits against any stretch of the repeated unit        */
  uint32_t unit_bases;           /* the length of the shortest such stretch                          */
  uint32_t end_phase;            /* the unit position after its last base                            */
  uint32_t flags;                /* OTG_UNITALIGN_NO_UNIT / _TOO_LONG / _UNIT_TOO_LONG               */
} otg_unitalign;
int otg_unitalign_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                        uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                        uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks, otg_unitalign* out);
int otg_unitalign_motifs(otg_ctx* ctx, otg_unitalign* out);
int otg_unitalign_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                         const uint32_t* unit_len, uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks,
                         otg_unitalign* out);
int otg_unitalign_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_unitalign** records);
int otg_unitalign_last_ms(otg_ctx* ctx, double* ms);
int otg_parse_bed_units(const char* path, uint64_t* rec_first, uint64_t rec_capacity, uint64_t* n_records, uint64_t* unit_off, uint32_t* unit_len,
                        uint64_t unit_capacity, uint64_t* n_units, uint8_t* unit_arena, uint64_t arena_capacity, uint64_t* arena_bytes);
int otg_unitalign_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len, const uint64_t* task_first,
                       const uint8_t* task_source, const uint8_t* unit_arena, const uint64_t* task_unit_off, const uint32_t* task_unit_len,
                       const otg_unitalign* aligned, char* out, uint64_t out_capacity, uint64_t* out_len);
/* Copy numbers of the alleles of a VCF against a tandem-repeat catalogue, in file order, built as otg_motifs_files is.  Per VCF record the
 * BED record whose region string (chr:start-end, as the VCF writer prints it) equals the ID column is looked up; the first one wins when the
 * BED repeats a region.  Where that record has units (otg_parse_bed_units) every allele gets one row per unit with source = bed.  Otherwise,
 * and for a region the BED does not hold, every allele gets one row against its own motif-annotation unit (max_period, slack as
 * otg_motifs_files; the unit stays on the device in between) with source = motif; the unit is "." with zeros when the period is 0.
 * Out-of-range parameters are OTG_ERR_ARG with the message the tool prints.  stats as otg_vcf2mat_files. */
typedef struct otg_copies_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, the catalogue                                      */
  uint32_t    max_period;        /* -p: 1..OTG_MOTIF_MAX_PERIOD (the tool's default: 256)            */
  uint32_t    slack;             /* --slack: 0..999 per mille (the tool's default: 50)               */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = 65536                                     */
  uint32_t    reserved;
} otg_copies_job;
int otg_copies_files(const otg_copies_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Joint parse of an allele against several repeat units.  A catalogue describes a locus as several units (MOTIFS=CAG,CCG); the unit
 * alignment above takes one unit per task, so each unit counts the other's tract as edits and nothing says where one tract ends.  Here one
 * alignment runs over all units of a set, joined at their unit boundaries, and a traceback gives the segments: how many copies of each unit,
 * in which order, over which allele bases, at how many edits.  The reference has no counterpart; this is the definition (all integers;
 * DESIGN.md §9).  A task is a sequence s of length L and an ordered unit set u_0 .. u_{K-1}, 1 <= K <= OTG_UNITPARSE_MAX_UNITS, every p_k in
 * 1..OTG_UNITALIGN_MAX_UNIT.  Codes and matching are those of the unit alignment: code 4 matches nothing, letter case changes nothing.
 *   1. Language.  Let t range over the concatenations of pieces, the empty one included.  A piece is a non-empty substring of one u_k
 *      repeated without end.  Two adjacent pieces belong to different units and meet at a unit boundary: the left one ends with the last base
 *      of a copy, the right one starts at base 0.  switches(t) = pieces - 1, 0 for the empty t.  The result is the lexicographic minimum over
 *      t of (the unit-cost edit distance of s and t, switches(t), |t|), reported as edits, switches, unit_bases.
 *   2. The DP that defines phases, ties and the path.  Cell (i, k, j) is "i bases of s consumed, the next unit base is u_k[j]"; its key is
 *      edits * 2^42 + switches * 2^21 + unit_bases, so one unsigned minimum gives the lexicographic order.
 *        V[0][k][j] = 0 everywhere;
 *        the diagonal step:              V[i+1][k][(j+1) % p_k] <= V[i][k][j] + (c_s[i] == c_u[j] && c_s[i] < 4 ? 0 : 2^42) + 1;
 *        a base of s outside the unit:   V[i+1][k][j] <= V[i][k][j] + 2^42;
 *        a skipped unit base:            V[i][k][(j+1) % p_k] <= V[i][k][j] + 2^42 + 1;
 *        a switch, only at phase 0:      V[i][k'][0] <= V[i][k][0] + 2^21 for k' != k;
 *      the skip and the switch are taken together to their least fixed point within a row.  The end cell is the smallest (k, j) in unit-set
 *      order with V[L] minimal: end_unit, end_phase.
 *   3. The reported path is traced back from the end cell.  At every cell the first predecessor in this order whose value plus step cost
 *      equals the cell's value is taken: the diagonal; the base outside the unit; the skip from position j - 1 of the same unit (for j = 0
 *      from p_k - 1); the switch from the lowest k'.  The trace stops at row 0 (every cell there is 0).  In-row steps all cost something, so
 *      the trace cannot cycle.
 *   4. Segments.  A segment is a maximal stretch of the path inside one unit: {unit, begin, end, unit_bases, edits, start_phase}.  [begin,
 *      end) are allele positions (the rows the stretch consumed) and the segments tile [0, L); start_phase is the unit position at the
 *      path's start for the first segment and 0 for the others; the edits and unit_bases of the segments sum to the task's; n_segments =
 *      switches + 1 when L > 0.  L = 0: no segments, all zeros.
 *   5. Refusals.  An empty unit set, K > OTG_UNITPARSE_MAX_UNITS, a unit of 0 or over OTG_UNITALIGN_MAX_UNIT bytes, or a set that does not fit
 *      one wave (the sum of ceil(p_k / 4) over the set exceeds OTG_UNITPARSE_MAX_LANES) is OTG_ERR_ARG from a caller.  L >
 *      OTG_UNITPARSE_MAX_LEN: zeros, no segments and flags = OTG_UNITPARSE_TOO_LONG; the batch does not fail.  OTG_UNITPARSE_MAX_LEN is the
 *      largest L for which no key field carries (derived value by value in otg_unitparse_core.hpp).
 * It follows that K = 1 gives the (edits, unit_bases, end_phase) of the unit alignment, and that an interruption that is itself a unit of
 * the set is a segment, not an edit.
 *   otg_unitparse_batch           alleles and units as in otg_unitalign_batch; set q is units set_first[q] .. set_first[q + 1) in that order
 *                                 (the rec_first of otg_parse_bed_units); task t parses allele task_seq[t] against set task_set[t].  sums:
 *                                 n_tasks summaries; seg_off: n_tasks + 1 offsets into the segments, which stay in HBM; *n_segments =
 *                                 seg_off[n_tasks].  Every output is nullable.  An index out of range, an allele or a unit outside its arena
 *                                 and the refusals of step 5: OTG_ERR_ARG.  More than 2^24 tasks: OTG_ERR_CAPACITY;
 *   otg_unitparse_collect         copies the segments of the latest call on the context to segs[0 .. total); capacity < total is
 *                                 OTG_ERR_CAPACITY with the needed count in the message;
 *   otg_unitparse_device_results  device pointers of the latest results on this context (n summaries, n + 1 offsets, total segments), valid
 *                                 until the next unit parse on the context or otg_destroy; every output is nullable;
 *   otg_unitparse_last_ms         HIP-event times (ms) of the latest call: forward_ms = the alignment kernels, trace_ms = the scan of the
 *                                 segment counts and the backward walk;
 *   otg_unitparse_cohort          rows [row_begin, row_begin + n) of the row list of otg_kmer_cohort_rows, the alleles read in the regrouped
 *                                 cohort arena in place (preconditions and refusals as otg_unitalign_cohort with caller units; only the row
 *                                 lengths come to the host, where the tasks are ordered); task_seq is relative to row_begin;
 *   otg_unitparse_emit            per allele a = records[r].first_allele + i the row region \t i \t seq_len[a] \t units \t edits \t switches \t
 *                                 unit_bases \t identity \t counts \t structure \n.  The unit set of allele a is set allele_set[a] (units
 *                                 set_first[q] .. set_first[q + 1), or OTG_UNITPARSE_NO_SET), unit k the unit_len[k] bytes at unit_arena +
 *                                 unit_off[k]; sums[a] and seg_off[a] are the allele's; units = the set comma-joined as given; identity as in otg_unitalign_emit; counts = per unit of
 *                                 the set the unit bases of its segments / p_k as "%.2f", comma-joined; structure = the segments
 *                                 (segs[seg_off[a] .. seg_off[a + 1])) left to right as (UNIT)c, c = unit_bases / p as an integer when it
 *                                 divides and "%.2f" otherwise, followed by ~e when the segment has e > 0 edits; "." when there are none.  An
 *                                 allele without units gives "." for units, zeros, and "." for counts and structure.  A segment that names a
 *                                 unit outside its set is OTG_ERR_ARG.  Buffer protocol of otg_emit_alleles.
 * The forward pass keeps the row in registers as the unit alignment does, every unit at a lane boundary.  It stores decisions, not keys:
 * two bits per cell and one per unit and row, as wave ballots (2 R + 1 words of 64 bits per row and wave).  A call is cut into chunks of
 * tasks whose store stays under OTG_UNITPARSE_TRACE_MB megabytes (default 1024; read once per process; a single task above it runs alone;
 * DESIGN.md §8); with more than one chunk the forward pass runs once more without the store, for the segment counts.
 * ------------------------------------------------------------------------------------------- */
#define OTG_UNITPARSE_MAX_UNITS 8
#define OTG_UNITPARSE_MAX_LANES 64
#define OTG_UNITPARSE_MAX_LEN   ((2097151 - 2 * OTG_UNITALIGN_MAX_UNIT + 1) / 2)   /* 1048320 */
#define OTG_UNITPARSE_TOO_LONG  1u   /* otg_unitparse_sum.flags */
#define OTG_UNITPARSE_NO_SET    0xffffffffu   /* otg_unitparse_emit: an allele without units */
typedef struct otg_unitparse_sum {
  uint32_t edits;                /* the fewest edits against any word of the language               */
  uint32_t switches;             /* the fewest switches at those edits                               */
  uint32_t unit_bases;           /* the shortest such word                                           */
  uint32_t n_segments;           /* switches + 1; 0 for an empty or refused allele                   */
  uint32_t end_unit;             /* the unit of the end cell, an index into the set                  */
  uint32_t end_phase;            /* the unit position after the path's last base                     */
  uint32_t flags;                /* OTG_UNITPARSE_TOO_LONG                                           */
  uint32_t reserved;             /* 0                                                                */
} otg_unitparse_sum;
typedef struct otg_unitparse_seg {
  uint32_t unit;                 /* an index into the task's unit set                                */
  uint32_t begin;                /* allele positions [begin, end)                                    */
  uint32_t end;
  uint32_t unit_bases;
  uint32_t edits;
  uint32_t start_phase;          /* the unit position at the path's start; 0 behind a switch         */
} otg_unitparse_seg;
int otg_unitparse_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                        uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                        uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set,
                        uint32_t n_tasks, otg_unitparse_sum* sums, uint64_t* seg_off, uint64_t* n_segments);
int otg_unitparse_collect(otg_ctx* ctx, otg_unitparse_seg* segs, uint64_t capacity);
int otg_unitparse_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_unitparse_sum** sums, const uint64_t** seg_off,
                                 const otg_unitparse_seg** segs, uint64_t* total);
int otg_unitparse_last_ms(otg_ctx* ctx, double* forward_ms, double* trace_ms);
int otg_unitparse_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                         const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                         const uint32_t* task_set, uint32_t n_tasks, otg_unitparse_sum* sums, uint64_t* seg_off, uint64_t* n_segments);
int otg_unitparse_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                       const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off,
                       const uint32_t* unit_len, const otg_unitparse_sum* sums, const uint64_t* seg_off, const otg_unitparse_seg* segs, char* out, uint64_t out_capacity,
                       uint64_t* out_len);
/* The joint parse of the alleles of a VCF against a tandem-repeat catalogue, in file order, built as otg_copies_files is.  Per VCF record the
 * BED record whose region string equals the ID column is looked up (the first one wins); every allele gets one row against that record's
 * unit set.  A region with no units in the catalogue, or one not in it, gives the row without units.  A unit set the parse refuses (step 5)
 * is OTG_ERR_ARG with the region in the message.  stats as otg_vcf2mat_files. */
typedef struct otg_unitparse_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, the catalogue                                      */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = 65536                                     */
  uint32_t    reserved;
} otg_unitparse_job;
int otg_unitparse_files(const otg_unitparse_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Tract mode of the copy numbers: find the repeat inside a flanked allele.  The unit alignment above is global in the allele, so flank
 * bases inside a region count as edits.  Here a local (Smith-Waterman style) wraparound alignment locates the tract, and the unit
 * alignment is then applied to exactly that tract.  The reference has no counterpart; this is the definition (all integers).
 * Codes, folding and matching are those of the unit alignment: code 4 matches nothing, letter case changes nothing.  The scores are
 * otg_tract_params {match, mismatch, indel, min_score}; otg_tract_params_default gives (2, 7, 7, 24); 1 <= match <= 16, 1 <= mismatch <= 64,
 * 1 <= indel <= 64 and min_score <= 2^24, anything else is OTG_ERR_ARG.  For an allele s of length L and a unit u of length p,
 * 1 <= p <= OTG_UNITALIGN_MAX_UNIT:
 *   1. Cell (i, j) is "i bases of s consumed, the next unit base is u[j]".  Its value is the pair (score, begin), ordered by the larger
 *      score, then the LARGER begin (the tight tract).
 *   2. C[0][j] = (0, 0).
 *   3. Row i + 1 starts every position at the fresh start (0, i + 1) and takes the maximum of
 *        the diagonal step             C[i][j] -> C[i+1][(j+1) % p] with + match when c_s[i] == c_u[j] && c_s[i] < 4, else - mismatch;
 *        a base of s outside the unit  C[i][j] -> C[i+1][j] with - indel;
 *        a skipped unit base           C[i+1][j] -> C[i+1][(j+1) % p] with - indel, taken to its fixed point around the cycle.
 *      A candidate whose score is not positive is dropped (a fresh start beats it: it has the largest begin a row can hold).  Steps keep begin.
 *   4. The best cell over all rows 0..L and positions: the largest score, then the SMALLEST i (= end), then the larger begin, then the
 *      smallest j.
 *   5. score = 0 or score < min_score: begin = end = edits = unit_bases = end_phase = start_phase = 0, flags = OTG_TRACT_NONE; score is
 *      still reported.
 *   6. Otherwise (edits, unit_bases, end_phase) are, by definition, the otg_unitalign record of the bytes s[begin, end) against u, and
 *      start_phase = (end_phase - unit_bases) mod p.
 *   7. p = 0: zeros and OTG_TRACT_NO_UNIT.  L > OTG_TRACT_MAX_LEN: zeros and OTG_TRACT_TOO_LONG.  p > OTG_UNITALIGN_MAX_UNIT: OTG_ERR_ARG when
 *      the caller passes the unit in, zeros and OTG_TRACT_UNIT_TOO_LONG when it comes from the motif annotation.  L = 0: score 0 and
 *      OTG_TRACT_NONE.
 * It follows that N bytes in front of s move begin and end by their count and change nothing else, that N bytes behind s change nothing,
 * that a rotated unit changes only the two phases, that score <= match * (end - begin), and that a tract begins and ends on a match.
 *   otg_tract_batch           alleles, units and tasks as in otg_unitalign_batch; params == NULL: the defaults.  out: n_tasks records, NULL
 *                             leaves them in HBM.  Refusals as otg_unitalign_batch, and OTG_ERR_ARG for scores out of range;
 *   otg_tract_motifs          task i = allele i of the latest motif call on the context against that call's unit i, both read where they
 *                             lie in HBM (as otg_unitalign_motifs): a motif unit found on a flanked allele;
 *   otg_tract_cohort          rows of the cohort arena in place, with the caller's units or (unit_arena == NULL) those of the latest
 *                             otg_motif_cohort; preconditions and refusals as otg_unitalign_cohort;
 *   otg_tract_device_results  the device pointer of the latest records on this context, valid until the next tract call on the context or
 *                             otg_destroy; every output is nullable;
 *   otg_tract_last_ms         HIP-event times (ms) of the latest call: *ms = both passes, *local_ms (nullable) = the local pass alone;
 *   otg_tract_emit            per task t the row region \t i \t seq_len \t source \t unit \t begin \t end \t score \t edits \t unit_bases \t
 *                             copies \t identity \n, arguments as otg_unitalign_emit: copies "%.2f" of unit_bases / p and identity "%.4f" of
 *                             1 - edits / max(end - begin, unit_bases); both are 0.00 / 0.0000 when a flag is set or the denominator is 0.
 *                             Buffer protocol of otg_emit_alleles.
 * A tract call runs the unit alignment as its second pass, on sub-rows of the same arena, so it counts as a unit alignment on the context:
 * it replaces what otg_unitalign_device_results and otg_unitalign_last_ms return (task t: the record of s[begin, end), an empty row for a
 * task without a tract).  The local pass has the layout of the unit alignment (the row in registers, 4 .. 64 lanes per task).  The key is
 * score * 2^16 + begin in 32 bits while the allele is no longer than the bound otg_tract_core.hpp derives from the call's scores and the
 * unit length, 32 / 32 in 64 bits above.  OTG_TRACT_WIDE=1 sends every task through the 64-bit tier, OTG_TRACT_SEG64=1 gives every task a
 * whole wave (both read once per process).
 * ------------------------------------------------------------------------------------------- */
#define OTG_TRACT_MAX_LEN       1048575
#define OTG_TRACT_NO_UNIT       1u   /* otg_tract.flags */
#define OTG_TRACT_TOO_LONG      2u
#define OTG_TRACT_UNIT_TOO_LONG 4u
#define OTG_TRACT_NONE          8u   /* no tract: score 0 or below min_score                             */
typedef struct otg_tract_params {
  uint32_t match;                /* added per matching base: 1..16                                   */
  uint32_t mismatch;             /* taken off per mismatching base: 1..64                            */
  uint32_t indel;                /* taken off per inserted or skipped base: 1..64                    */
  uint32_t min_score;            /* a tract scores at least this: 0..2^24                            */
} otg_tract_params;
typedef struct otg_tract {
  uint32_t score;                /* of the best local alignment, also when there is no tract         */
  uint32_t begin;                /* the tract is s[begin, end)                                       */
  uint32_t end;
  uint32_t edits;                /* the otg_unitalign record of the tract                            */
  uint32_t unit_bases;
  uint32_t end_phase;
  uint32_t start_phase;          /* (end_phase - unit_bases) mod p                                   */
  uint32_t flags;                /* OTG_TRACT_NO_UNIT / _TOO_LONG / _UNIT_TOO_LONG / _NONE           */
} otg_tract;
void otg_tract_params_default(otg_tract_params* params);
int otg_tract_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                    uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                    uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks, const otg_tract_params* params,
                    otg_tract* out);
int otg_tract_motifs(otg_ctx* ctx, const otg_tract_params* params, otg_tract* out);
int otg_tract_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                     const uint32_t* unit_len, uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks,
                     const otg_tract_params* params, otg_tract* out);
int otg_tract_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_tract** records);
int otg_tract_last_ms(otg_ctx* ctx, double* ms, double* local_ms);
int otg_tract_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len, const uint64_t* task_first,
                   const uint8_t* task_source, const uint8_t* unit_arena, const uint64_t* task_unit_off, const uint32_t* task_unit_len,
                   const otg_tract* tracts, char* out, uint64_t out_capacity, uint64_t* out_len);
/* The tracts of the alleles of a VCF against a tandem-repeat catalogue, in file order, built as otg_copies_files is: the same catalogue
 * lookup, the motif-annotation unit where the catalogue gives none, one otg_tract_emit row per allele and unit.  Out-of-range parameters
 * are OTG_ERR_ARG with the message the tool prints.  stats as otg_vcf2mat_files. */
typedef struct otg_tracts_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, the catalogue                                      */
  uint32_t    max_period;        /* -p: 1..OTG_MOTIF_MAX_PERIOD (the tool's default: 256)            */
  uint32_t    slack;             /* --slack: 0..999 per mille (the tool's default: 50)               */
  uint32_t    match;             /* --scores match,mismatch,indel (the tool's default: 2,7,7)        */
  uint32_t    mismatch;
  uint32_t    indel;
  uint32_t    min_score;         /* --min-score: 0..2^24 (the tool's default: 24)                    */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = 65536                                     */
  uint32_t    reserved;
} otg_tracts_job;
int otg_tracts_files(const otg_tracts_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Locus mode: the joint unit-set parse inside a flanked allele.  The joint parse above is global in the allele, so flank bases count as edits
 * and are attributed to segments; the tract mode above trims the flanks, but for one unit.  Here a local wraparound alignment over the whole
 * unit set locates the repeat, and the joint parse is then applied to exactly that stretch.  The reference has no counterpart; this is the
 * definition (all integers).  A task is an allele s of length L and an ordered unit set u_0 .. u_{K-1}; the refusals are
 * exactly those of the joint parse (step 5 there).  Codes, folding and matching are those of the unit alignment.  The scores are an
 * otg_tract_params with the same ranges and the same defaults (2, 7, 7, 24).
 *   1. Cell (i, k, j) is "i bases of s consumed, the next unit base is u_k[j]".  Its value is the pair (score, begin), ordered by the larger
 *      score, then the LARGER begin.
 *   2. C[0][k][j] = (0, 0).
 *   3. Row i + 1 starts every position at the fresh start (0, i + 1) and takes the maximum of
 *        the diagonal step             C[i][k][j] -> C[i+1][k][(j+1) % p_k] with + match when c_s[i] == c_u[j] && c_s[i] < 4, else - mismatch;
 *        a base of s outside the unit  C[i][k][j] -> C[i+1][k][j] with - indel;
 *        a skipped unit base           C[i+1][k][j] -> C[i+1][k][(j+1) % p_k] with - indel;
 *        a switch, only at phase 0     C[i+1][k][0] -> C[i+1][k'][0] for k' != k, at no score;
 *      the last two taken together to their fixed point within the row.  A candidate whose score is not positive is dropped.  Steps keep
 *      begin.  A switch is free here for the reason it costs no edit in the joint parse; the second pass orders the switches, the local
 *      pass only finds where the repeat lies.
 *   4. The best cell over all rows and positions: the largest score, then the SMALLEST i (= end), then the larger begin, then the smallest
 *      (k, j) in set order.
 *   5. score = 0 or score < min_score: everything but score is 0, no segments, flags = OTG_LOCUS_NONE.
 *   6. Otherwise (edits, switches, unit_bases, n_segments) and the segments are, by definition, the joint parse of the bytes s[begin, end)
 *      against the same set, the segments' begin and end shifted by the tract's begin: they are allele positions and tile [begin, end).
 *   7. L > OTG_LOCUS_MAX_LEN (= OTG_UNITPARSE_MAX_LEN, the smaller cap of the two passes): zeros and OTG_LOCUS_TOO_LONG; the batch does not
 *      fail.  L = 0: OTG_LOCUS_NONE.
 * It follows that K = 1 gives the (score, begin, end, edits, unit_bases) of otg_tract_batch for that unit, that N bytes in front of s move
 * begin, end and the segment positions by their count and change nothing else, that N bytes behind s change nothing, that letter case
 * changes nothing, and that score <= match * (end - begin).  There is one tract per allele: a spacer between two repeats that is cheaper
 * than a restart lies inside it.
 *   otg_locus_batch           alleles, units, sets and tasks as in otg_unitparse_batch; params == NULL: the defaults.  out: n_tasks records;
 *                             seg_off: n_tasks + 1 offsets into the segments, which stay in HBM; *n_segments = seg_off[n_tasks].  Every
 *                             output is nullable.  Refusals as otg_unitparse_batch, and OTG_ERR_ARG for scores out of range;
 *   otg_locus_collect         copies the segments of the latest locus call on the context to segs[0 .. total), as otg_unitparse_collect;
 *   otg_locus_device_results  device pointers of the latest results on this context (n records, n + 1 offsets, total segments), valid until
 *                             the next locus call or unit parse on the context or otg_destroy; every output is nullable;
 *   otg_locus_last_ms         HIP-event times (ms) of the latest call: *ms = both passes, *local_ms (nullable) = the local pass alone;
 *   otg_locus_last_tiers      how many tasks of the latest call the local pass ran on the 32-bit key and on the 64-bit key (tasks that were
 *                             not aligned, L = 0 or over the cap, count for neither); every output is nullable;
 *   otg_locus_cohort          rows of the cohort arena in place; arguments, preconditions and refusals as otg_unitparse_cohort, plus params;
 *   otg_locus_emit            per allele a = records[r].first_allele + i the row region \t i \t seq_len[a] \t units \t begin \t end \t score \t
 *                             edits \t switches \t unit_bases \t identity \t counts \t structure \n, arguments as otg_unitparse_emit with
 *                             loci[a] the allele's record: identity "%.4f" of 1 - edits / max(end - begin, unit_bases), 0.0000 when a flag
 *                             is set; counts and structure as otg_unitparse_emit formats them; an allele without a tract gives zeros (the
 *                             score stays) and "." for the structure, one without a set zeros and "." for units, counts and structure.  Buffer protocol of
 *                             otg_emit_alleles.
 * A locus call runs the joint parse as its second pass, on sub-rows of the same arena, so it counts as a unit parse on the context: afterwards
 * otg_unitparse_device_results and otg_unitparse_collect give, per task, the summary of the sub-row s[begin, end) (an empty row for a task
 * without a tract: zeros) and the segments already in allele coordinates; otg_unitparse_last_ms gives the second pass.  otg_assemble_spread
 * (below) runs two locus calls, the reads' one last: after it these entries hold the READS' records by otg_spread_read.task.  The local pass has
 * the lane layout of the joint parse (every unit at a lane boundary, 4 .. 64 lanes per task) and the key of the tract mode: score * 2^16 +
 * begin in 32 bits while the allele is no longer than the bound otg_locus_core.hpp derives from the call's scores and the largest unit of
 * the set, 32 / 32 in 64 bits above.  OTG_LOCUS_WIDE=1 sends every task through the 64-bit tier, OTG_LOCUS_SEG64=1 gives every task a
 * whole wave (both read once per process).
 * ------------------------------------------------------------------------------------------- */
#define OTG_LOCUS_MAX_LEN  OTG_UNITPARSE_MAX_LEN
#define OTG_LOCUS_TOO_LONG 1u   /* otg_locus.flags */
#define OTG_LOCUS_NONE     2u   /* no tract: score 0 or below min_score                             */
typedef struct otg_locus {
  uint32_t score;                /* of the best local alignment, also when there is no tract         */
  uint32_t begin;                /* the tract is s[begin, end)                                       */
  uint32_t end;
  uint32_t edits;                /* the joint parse of the tract                                     */
  uint32_t switches;
  uint32_t unit_bases;
  uint32_t n_segments;           /* switches + 1; 0 without a tract                                  */
  uint32_t flags;                /* OTG_LOCUS_TOO_LONG / _NONE (OTG_UNITSET_LOCUS_NO_SET after otg_unitset_locus) */
} otg_locus;
int otg_locus_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                    uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                    uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set,
                    uint32_t n_tasks, const otg_tract_params* params, otg_locus* out, uint64_t* seg_off, uint64_t* n_segments);
int otg_locus_collect(otg_ctx* ctx, otg_unitparse_seg* segs, uint64_t capacity);
int otg_locus_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_locus** records, const uint64_t** seg_off,
                             const otg_unitparse_seg** segs, uint64_t* total);
int otg_locus_last_ms(otg_ctx* ctx, double* ms, double* local_ms);
int otg_locus_last_tiers(otg_ctx* ctx, uint32_t* narrow, uint32_t* wide);
int otg_locus_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                     const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                     const uint32_t* task_set, uint32_t n_tasks, const otg_tract_params* params, otg_locus* out, uint64_t* seg_off,
                     uint64_t* n_segments);
int otg_locus_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                   const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off,
                   const uint32_t* unit_len, const otg_locus* loci, const uint64_t* seg_off, const otg_unitparse_seg* segs, char* out,
                   uint64_t out_capacity, uint64_t* out_len);
/* The locus mode over the alleles of a VCF against a tandem-repeat catalogue, in file order, built as otg_unitparse_files is: the same
 * catalogue lookup, one otg_locus_emit row per allele, a refused unit set is OTG_ERR_ARG with the region in the message.  Out-of-range
 * scores are OTG_ERR_ARG with the message the tool prints.  stats as otg_vcf2mat_files. */
typedef struct otg_loci_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, the catalogue                                      */
  uint32_t    match;             /* --scores match,mismatch,indel (the tool's default: 2,7,7)        */
  uint32_t    mismatch;
  uint32_t    indel;
  uint32_t    min_score;         /* --min-score: 0..2^24 (the tool's default: 24)                    */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = 65536                                     */
  uint32_t    reserved;
} otg_loci_job;
int otg_loci_files(const otg_loci_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Unit sets from the alleles: the repeat units of a region, discovered from the repeat structure of its alleles.  The joint parse and the
 * locus mode above need a unit set per region; a three-column BED has none.  The repeat structure already writes, per allele, the exact
 * units that occur; this operator turns "the units seen in the alleles of a region" into "the unit set of that region", one set for all
 * alleles of the region, so that their parses are comparable.  The reference has no counterpart; this is the definition (all integers;
 * DESIGN.md §9).  The input is the latest repeat call on the context (its n alleles, its segments, its parameters), a grouping of those
 * alleles into n_groups contiguous groups, group_first[0] = 0 <= group_first[1] <= .. <= group_first[n_groups] = n (a group is a region: the
 * alleles of a VCF record, or row_first of otg_kmer_cohort_rows), and otg_unitset_params {min_bases, min_permille, redundant_permille,
 * reserved}: 1..2^24, 0..1000, 0..1000, 0; otg_unitset_params_default gives (12, 50, 100, 0).  Per group:
 *   1. Candidates.  Every repeat segment (begin, period p, copies, length) of every allele of the group with p <= OTG_UNITALIGN_MAX_UNIT.
 *      Its unit is the p codes c[begin .. begin + p) (the motif table: letter case folds; a run is exact and code 4 matches nothing, so a
 *      unit holds only ACGT).  Longer periods and literals are ignored.  The repeat parse prefers the smaller period, so a unit is never a
 *      repetition of a shorter one.
 *   2. Classes.  The class of a unit is its smallest rotation, compared code by code: CAG, AGC and GCA are one class.  Per class: weight =
 *      the sum of the segment lengths (64 bits), segments = their number, length = p, and the REPRESENTATIVE = the unit exactly as the
 *      class's longest segment wrote it, ties to the lower allele index, then to the lower begin.  The set carries the representative,
 *      not the smallest rotation: the joint parse switches units only at phase 0, so a rotated unit costs edits at every junction.
 *   3. Rank.  Classes in the order weight descending, length ascending, smallest rotation ascending code by code (a total order).  A class
 *      with weight < min_bases, or with weight * 1000 < min_permille * (the largest weight of the group), is dropped; the first
 *      OTG_UNITSET_TOP of the rest are ranked, later ones are dropped.
 *   4. Redundancy.  Ranked class c with representative u of length p is redundant when for some class d ranked before it (redundant or
 *      not) the unit alignment (the rule of otg_unitalign_*, unchanged) of the sequence u u against rep(d) has edits * 1000 <=
 *      redundant_permille * 2 p.  Two copies, so that the junction counts: AGAA is a substring of GAA repeated, AGAAAGAA needs one edit.
 *   5. Selection.  In rank order over the ranked classes that are not redundant: a class is taken when fewer than OTG_UNITPARSE_MAX_UNITS
 *      are taken and the lanes used so far plus ceil(p / 4) stay within OTG_UNITPARSE_MAX_LANES; otherwise it is skipped and the walk goes
 *      on.  The set of the group is the representatives of the taken classes in rank order, as upper-case ACGT bytes: the joint parse and
 *      the locus mode accept every discovered set.
 *   6. The group's record otg_unitset: n_units; n_classes = the distinct classes seen; n_ranked = the classes ranked in step 3;
 *      weight_total = the sum of all candidate lengths; flags: OTG_UNITSET_NONE when no unit was selected (an empty group, no repeat
 *      segment, everything under the thresholds), OTG_UNITSET_OVERFLOW (with OTG_UNITSET_NONE) when the group has more than
 *      OTG_UNITSET_MAX_CLASSES distinct classes: no set, n_classes = OTG_UNITSET_MAX_CLASSES + 1, n_ranked = 0; the batch does not fail.
 *   7. Per selected unit otg_unitset_unit {weight, segments, length} of its class.  The units of group g are set_first[g] ..
 *      set_first[g + 1] of the unit list, their bytes unit_arena[unit_off[k] .. + unit_len[k]): the four arrays otg_unitparse_batch and
 *      otg_locus_batch take.
 * It follows that the result does not depend on the order in which segments are processed, that permuting the alleles of a group changes
 * at most which of several equally long segments gives a representative, and that rotating every copy of a unit in every allele changes
 * only the representatives.  No reverse-complement merging: all alleles of a region are on the reference strand.
 *   otg_unitset_repeats         discovery over the latest otg_repeat_batch / otg_repeat_cohort on the context, whose alleles are read where
 *                               that call read them (they must still lie there: the check of otg_unitalign_motifs).  sets: n_groups
 *                               records; set_first: n_groups + 1 offsets into the unit list; *n_units, *unit_bytes: the sizes
 *                               otg_unitset_collect needs.  Every output is nullable; params == NULL: the defaults.  The results stay in
 *                               HBM.  No repeat results, a bad group_first or bad params: OTG_ERR_ARG; more than 2^24 groups:
 *                               OTG_ERR_CAPACITY;
 *   otg_unitset_collect         copies the unit records, unit_off, unit_len (unit_capacity entries each) and the unit bytes of the latest
 *                               discovery to host arrays; a capacity too small is OTG_ERR_CAPACITY with the needs in the message;
 *   otg_unitset_device_results  device pointers of all of it, valid until the next discovery on the context or otg_destroy; every output is
 *                               nullable;
 *   otg_unitset_last_ms         HIP-event times (ms) of the latest discovery: vote_ms = candidates and vote, select_ms = the pair
 *                               lists, the pair alignments and the select;
 *   otg_unitset_locus          the locus mode of allele i of that repeat call against the set of its group, for every allele, the alleles
 *                               read in place.  No repeat call may lie between the discovery and this.  Tasks are the alleles whose group
 *                               has a set; the record of any other allele is zero with flags = OTG_UNITSET_LOCUS_NO_SET, and it has no segments.
 *                               out: n records, seg_off: n + 1 offsets; otg_locus_collect, otg_locus_device_results, otg_locus_last_ms and
 *                               otg_locus_last_tiers work on the result as after otg_locus_batch (otg_unitparse_device_results gives the
 *                               tasks of the second pass, which are fewer);
 *   otg_unitset_emit            one catalogue line per VCF record r, whose group is r: chrom \t start \t end \t MOTIFS=CAG,CCG;BASES=120,48;
 *                               SEGMENTS=3,2;ALLELES=2 \n, columns 1-3 those of the first BED record whose region string (chr:start-end)
 *                               equals the record's ID; a record without one is OTG_ERR_ARG naming it.  A group without a set has "." in
 *                               column 4, which otg_parse_bed_units reads as "no units".  Buffer protocol of otg_emit_alleles.
 * The redundancy test runs the unit alignment's own kernels on the representatives where they lie in the alleles (a repeat segment holds at
 * least two copies of its unit), so a discovery replaces what otg_unitalign_device_results and otg_unitalign_last_ms return.  The class
 * table of a group lies in LDS and is keyed by (length, a 64-bit hash of the smallest rotation); a hash match is confirmed on the bases.
 * OTG_UNITSET_HASH_BITS=<1..64> keeps only that many bits of the hash (read once per process), so that tests reach the
 * compare.
 * ------------------------------------------------------------------------------------------- */
#define OTG_UNITSET_TOP          16
#define OTG_UNITSET_MAX_CLASSES  2048
#define OTG_UNITSET_NONE         1u   /* otg_unitset.flags */
#define OTG_UNITSET_OVERFLOW     2u
#define OTG_UNITSET_LOCUS_NO_SET         4u   /* otg_locus.flags after otg_unitset_locus: the allele's group has no set */
typedef struct otg_unitset_params {
  uint32_t min_bases;            /* 1..2^24: the least weight of a class                             */
  uint32_t min_permille;         /* 0..1000: the least weight as a share of the group's largest      */
  uint32_t redundant_permille;   /* 0..1000: edits per 1000 bases of u u that still count as explained */
  uint32_t reserved;             /* 0                                                                */
} otg_unitset_params;
typedef struct otg_unitset {
  uint32_t n_units;
  uint32_t n_classes;
  uint32_t n_ranked;
  uint32_t flags;                /* OTG_UNITSET_NONE / _OVERFLOW                                     */
  uint64_t weight_total;
} otg_unitset;
typedef struct otg_unitset_unit {
  uint64_t weight;               /* bases in the class's segments                                    */
  uint32_t segments;
  uint32_t length;
} otg_unitset_unit;
void otg_unitset_params_default(otg_unitset_params* params);
int otg_unitset_repeats(otg_ctx* ctx, const uint32_t* group_first, uint32_t n_groups, const otg_unitset_params* params, otg_unitset* sets,
                        uint64_t* set_first, uint64_t* n_units, uint64_t* unit_bytes);
int otg_unitset_collect(otg_ctx* ctx, otg_unitset_unit* units, uint64_t* unit_off, uint32_t* unit_len, uint64_t unit_capacity, uint8_t* unit_arena,
                        uint64_t arena_capacity);
int otg_unitset_device_results(otg_ctx* ctx, uint32_t* n_groups, const otg_unitset** sets, const uint64_t** set_first, uint64_t* n_units,
                               const otg_unitset_unit** units, const uint64_t** unit_off, const uint32_t** unit_len, const uint8_t** unit_arena,
                               uint64_t* unit_bytes);
int otg_unitset_last_ms(otg_ctx* ctx, double* vote_ms, double* select_ms);
int otg_unitset_locus(otg_ctx* ctx, const otg_tract_params* params, otg_locus* out, uint64_t* seg_off, uint64_t* n_segments);
int otg_unitset_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const otg_bed* beds, const char* chr_arena,
                     uint32_t n_beds, const otg_unitset* sets, const uint64_t* set_first, const otg_unitset_unit* units, const uint8_t* unit_arena,
                     const uint64_t* unit_off, const uint32_t* unit_len, char* out, uint64_t out_capacity, uint64_t* out_len);
/* The unit sets of the regions of a VCF as a catalogue BED, in file order, built as otg_repeats_files is: per batch the repeat structure, the
 * discovery with one group per VCF record, one otg_unitset_emit line per record.  A batch ends at a record boundary, so the alleles of a
 * region are always in one discovery call; a record larger than batch_alleles runs alone.  The output is the input every catalogue tool
 * reads (otter_copies, otter_tracts, otter_unitparse, otter_loci).  Out-of-range parameters are OTG_ERR_ARG with the message the tool prints;
 * a VCF record without a BED record is OTG_ERR_ARG naming it.  stats as otg_vcf2mat_files. */
typedef struct otg_units_job {
  const char* vcf_path;          /* positional <VCF[.GZ]>                                            */
  const char* bed_path;          /* -b: required, gives columns 1-3                                  */
  uint32_t    max_period;        /* -p: 1..OTG_REPEAT_MAX_PERIOD (the tool's default: 256)           */
  uint32_t    min_copies;        /* --min-copies: 2..1024 (the tool's default: 2)                    */
  uint32_t    min_span;          /* --min-span: 2..65535 bases (the tool's default: 12)              */
  uint32_t    min_bases;         /* --min-bases: 1..2^24 (the tool's default: 12)                    */
  uint32_t    min_share;         /* --min-share: 0..1000 per mille (the tool's default: 50)          */
  uint32_t    redundant;         /* --redundant: 0..1000 per mille (the tool's default: 100)         */
  int32_t     threads;           /* -t: host threads of the emit                                     */
  int32_t     device;            /* HIP device ordinal                                               */
  uint32_t    batch_alleles;     /* alleles per batch, 0 = 65536                                     */
  uint32_t    reserved;
} otg_units_job;
int otg_units_files(const otg_units_job* job, otg_write_fn write, void* user, otg_job_stats* stats);
/* otg_loci_files with the unit sets discovered where the catalogue has none, in one pass per batch: the repeat structure, the discovery (one
 * group per VCF record; the parameters of `discover`, whose paths are ignored), the locus mode on the batch's alleles where the repeat call
 * left them in HBM.  A region whose catalogue record has units keeps them; any other region gets the set discovered from its alleles.  Rows
 * as otg_locus_emit, the units column holding the set that was used.  otg_loci_files itself is unchanged. */
int otg_units_loci_files(const otg_loci_job* job, const otg_units_job* discover, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Spread: the per-read copy numbers behind each consensus allele.  Every operator above reads consensus alleles, one sequence per haplotype;
 * this one reads the READS of an assemble batch where otg_assemble_run left them in HBM and reports, per consensus allele, the distribution
 * of the repeat length among the reads that voted for it (somatic expansion, mosaicism, a consensus off its reads' median).  No base and no
 * segment comes back to the host.  The reference has no counterpart; this is the definition (all integers).  The inputs are
 * the resident batch of the latest otg_assemble_run on the context, unit sets in the layout of otg_unitparse_batch, region_set[n_regions] (a
 * set index, or OTG_SPREAD_NONE = 0xffffffff for "this region has no set") and an otg_tract_params (NULL: the defaults).
 *   1. Read i of region r is COUNTED when the region's status is OTG_REGION_OK, the region has a set, the read's final label is >= 0 and both
 *      spanning flags of its descriptor are set (a reassigned non-spanning read carries a cut tract).
 *   2. A counted read's row is the bytes its device-side otg_read names as the run left them (a read rescued by local re-alignment is the
 *      trimmed one).  Its record is, by definition, the otg_locus record and segments of otg_locus_batch on those bytes against the region's
 *      set with those scores.  The read is CALLED when that record's flags are 0; its value is unit_bases, its value for unit k the sum of
 *      unit_bases over its segments with unit == k (0 without one).
 *   3. Every consensus allele (the n_alleles records of otg_assemble_result_sizes, in that order) is parsed the same way: ref_bases and the
 *      per-unit ref_bases are its unit_bases and per-unit sums; without a tract they are zeros and OTG_SPREAD_REF_NONE is set.
 *   4. The members of allele a are the called reads of its region whose label equals otg_allele.label.  With m members and their values
 *      sorted v_0 <= .. <= v_{m-1}: q[j] = v[floor(j (m - 1) / 4)], j = 0..4 (min, lower quartile, lower median, upper quartile, max); the
 *      same independently for every unit's series over the same members.  m = 0: q is zeros and OTG_SPREAD_NO_CALLS is set.
 *   5. For the total series only: n_below / n_above = the members with a value < / > ref_bases, sum_below = the sum of ref_bases - v and
 *      sum_above = the sum of v - ref_bases over them (64 bits); all four are 0 under OTG_SPREAD_REF_NONE.
 *   6. n_reads = the counted reads carrying the allele's label, n_called = m.  An allele of a region without a set: zeros and
 *      OTG_SPREAD_NO_SET.
 * It follows that q[0] <= .. <= q[4], that n_below + n_above <= n_called <= n_reads <= the region's read count, that letter case changes
 * nothing, that a single-unit set gives per-unit records equal to the total, and that with identical member reads every q[j] is their
 * common unit_bases, with n_below = n_above = 0 when that also equals ref_bases.
 *   otg_assemble_spread         out: n_alleles records (nullable); unit_off_out: n_alleles + 1 offsets into the unit records (nullable);
 *                               *n_unit_records (nullable) = their number, the size otg_spread_collect needs.  OTG_ERR_ARG: no completed
 *                               run on the context, n_regions not the batch's, a set index that is neither below n_sets nor
 *                               OTG_SPREAD_NONE, the unit-set refusals of otg_unitparse_batch, scores out of range;
 *   otg_spread_collect          the otg_spread_unit records of the latest call: allele a's are unit_off[a] .. unit_off[a + 1], one per unit
 *                               of its region's set in set order; a capacity too small is OTG_ERR_CAPACITY;
 *   otg_spread_collect_reads    one otg_spread_read per read of the batch: the row as the operator saw it, the label, counted, and task = the
 *                               read's index among the records of the reads' locus call (OTG_SPREAD_NONE for an uncounted read);
 *   otg_spread_device_results   device pointers of all of it, valid until the next spread call on the context or otg_destroy; every output
 *                               is nullable;
 *   otg_spread_last_ms          HIP-event times (ms) of the latest call: *ms = the device work of the call summed (the three parts that follow
 *                               and the row, reference and read-record kernels; not the host's planning, copies and waits between them),
 *                               the reads' locus call, the consensus locus call, the stats kernel; every output is nullable;
 *   otg_spread_emit             per allele of region r the row region \t label \t allele length \t units \t n_reads \t n_called \t ref \t min \t
 *                               q1 \t median \t q3 \t max \t n_below \t n_above \t sum_below \t sum_above \t per-unit \n, the totals in unit
 *                               bases, the per-unit column UNIT:ref:min/q1/med/q3/max joined by `,`, in copies ("%.2f" of bases / unit
 *                               length, as otg_unitparse_emit formats its counts column); a row without a set has "." as its units and
 *                               per-unit columns.  Regions in batch order, alleles in record order.  Buffer protocol of otg_emit_alleles.
 * The call runs the locus mode twice, the consensus alleles first and the reads last, so it counts as a locus call (and as a unit parse) on
 * the context: afterwards otg_locus_device_results and otg_locus_collect hold the READS' records and segments, indexed by otg_spread_read.task.
 * The statistics are found by selection on the value bits (otg_spread_core.hpp), one wave per allele, so the depth of a region is not capped;
 * regions of up to 256 reads keep their values in registers, deeper ones re-read the records per pass.  OTG_SPREAD_REREAD=1 sends every
 * allele through the second tier (read once per process).
 * ------------------------------------------------------------------------------------------- */
#define OTG_SPREAD_NONE     0xffffffffu   /* region_set: no set; otg_spread_read.task: not counted    */
#define OTG_SPREAD_NO_SET   1u            /* otg_spread.flags                                         */
#define OTG_SPREAD_NO_CALLS 2u
#define OTG_SPREAD_REF_NONE 4u
typedef struct otg_spread {
  uint32_t n_reads;              /* counted reads with the allele's label                            */
  uint32_t n_called;             /* of those, the members: their locus record has a tract            */
  uint32_t ref_bases;            /* unit_bases of the consensus allele itself                        */
  uint32_t q[5];                 /* min, lower quartile, lower median, upper quartile, max           */
  uint32_t n_below;              /* members with a value < ref_bases                                 */
  uint32_t n_above;
  uint64_t sum_below;            /* sum of ref_bases - value over them                               */
  uint64_t sum_above;
  uint32_t flags;                /* OTG_SPREAD_NO_SET / _NO_CALLS / _REF_NONE                        */
  uint32_t reserved;             /* 0                                                                */
} otg_spread;
typedef struct otg_spread_unit {
  uint32_t ref_bases;
  uint32_t q[5];
} otg_spread_unit;
typedef struct otg_spread_read {
  uint64_t seq_off;              /* the read's row in the batch's arena as the run left it           */
  uint32_t seq_len;
  int32_t  label;
  uint32_t counted;              /* 0 / 1                                                            */
  uint32_t task;                 /* its record of the reads' locus call, OTG_SPREAD_NONE: none       */
} otg_spread_read;
int otg_assemble_spread(otg_ctx* ctx, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                        uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* region_set, uint32_t n_regions,
                        const otg_tract_params* params, otg_spread* out, uint64_t* unit_off_out, uint64_t* n_unit_records);
int otg_spread_collect(otg_ctx* ctx, otg_spread_unit* units, uint64_t capacity);
int otg_spread_collect_reads(otg_ctx* ctx, otg_spread_read* reads, uint32_t capacity);
int otg_spread_device_results(otg_ctx* ctx, uint32_t* n_alleles, const otg_spread** records, const uint64_t** unit_off, uint64_t* n_unit_records,
                              const otg_spread_unit** units, uint32_t* n_reads, const otg_spread_read** reads);
int otg_spread_last_ms(otg_ctx* ctx, double* ms, double* reads_ms, double* consensus_ms, double* stats_ms);
int otg_spread_emit(const otg_bed* beds, const char* chr_arena, uint32_t n_regions, const otg_region_result* regions, const otg_allele* alleles,
                    const uint32_t* region_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off,
                    const uint32_t* unit_len, const otg_spread* records, const uint64_t* spread_unit_off, const otg_spread_unit* units, char* out,
                    uint64_t out_capacity, uint64_t* out_len);
/* The spread from files to rows in one call: the batch loop of otg_assemble_files (ingest, hot path, emit; the same bounded batches and
 * shards), with otg_assemble_spread on each batch right behind its run, on the same context, and one otg_spread_emit row per allele in BED
 * order where otg_assemble_files writes allele records; no header.  The BED is a catalogue: the units of a region are column 4 as
 * otg_parse_bed_units reads it, one set per record; a region without units gives OTG_SPREAD_NO_SET rows.  assemble.reads_only and
 * assemble.is_fasta must be 0.  Out-of-range scores are OTG_ERR_ARG with the message the tool prints; a unit set the locus mode refuses is
 * OTG_ERR_ARG.  otg_assemble_files itself writes what it wrote before.  stats as otg_assemble_files. */
typedef struct otg_spread_job {
  otg_assemble_job assemble;     /* BAM, catalogue BED, FASTA, assemble options, batches, devices    */
  uint32_t    match;             /* --scores match,mismatch,indel (the tool's default: 2,7,7)        */
  uint32_t    mismatch;
  uint32_t    indel;
  uint32_t    min_score;         /* --min-score: 0..2^24 (the tool's default: 24)                    */
} otg_spread_job;
int otg_spread_files(const otg_spread_job* job, otg_write_fn write, void* user, otg_job_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * Indexed allele BAMs from the product's own SAM text.  Every writer above emits SAM text and every reader wants a
 * coordinate-sorted BAM with its `.bai`; the reference's workflow goes through `samtools view -bh | samtools sort`, `samtools index` and
 * `samtools merge -pco` in between.  Host code (zlib + threads), no device work.
 *   otg_bam_sink_open    starts <bam_path>.  opts (NULL: all 0 / level -1): sort = 0 takes records in (target, position) order, unmapped last,
 *                        and streams them out with bounded memory (an out-of-order record is refused); sort = 1 holds every record in memory
 *                        as BAM bytes and stable-sorts them at close (ties keep input order).  threads: host threads that deflate the BGZF
 *                        blocks (<= 1: one); level: zlib's, -1 = its default.  The file bytes depend on neither threads nor on how the
 *                        text was cut into pieces;
 *   otg_bam_sink_write   has the otg_write_fn signature with user = the sink: pass it as `write` to otg_assemble_files (allele and
 *                        --reads-only SAM output) and otg_wgat, or call it from an otg_cohort_allele_write_fn with one sink per sample.
 *                        SAM text in arbitrary pieces (a piece may end inside a line): header lines first, then records with the eleven
 *                        mandatory fields and tags of type A, i, f, Z.  Records are byte for byte what sam_parse1 (src/sam.c:504-668) makes
 *                        of the line: integer tags take the smallest of c C s S i I, POS 0 and a `*` CIGAR make the record unmapped the way
 *                        it does.  The header text is `@HD VN:1.6 SO:coordinate` followed by the input's header lines (its own @HD dropped);
 *                        the targets are the @SQ lines.  Refused (OTG_ERR_ARG, line number and reason in otg_bam_sink_error): a header line
 *                        after the first record, fewer than eleven fields, a malformed number or CIGAR, a tag of another type, an RNAME that
 *                        is no @SQ, SEQ / QUAL / CIGAR lengths that disagree, more than 65535 CIGAR operations, a record that ends past
 *                        2^29 (BAI cannot index it), an out-of-order record with sort = 0.  After a refusal every later write fails with the same code
 *                        (OTG_ERR_FATAL when the file could not be written);
 *   otg_bam_sink_close   finishes <bam_path> (the BGZF EOF block last), writes <bam_path>.bai (binning index + 16-kb linear index, every chunk
 *                        begin the virtual offset of a record start) and frees the sink; after a refusal it behaves like otg_bam_sink_abort
 *                        and returns the error (its text stays in otg_last_error(NULL)).  *n_records (nullable) = records written;
 *   otg_bam_sink_abort   removes what was written and frees the sink;
 *   otg_bam_sink_error   the text of the sink's refusal ("" when there is none).
 * ------------------------------------------------------------------------------------------- */
typedef struct otg_bam_sink otg_bam_sink;
typedef struct otg_bam_sink_opts { int32_t sort, threads, level, reserved; } otg_bam_sink_opts;
int  otg_bam_sink_open(const char* bam_path, const otg_bam_sink_opts* opts, otg_bam_sink** out);
int  otg_bam_sink_write(void* sink, const char* data, uint64_t len);
int  otg_bam_sink_close(otg_bam_sink* sink, uint64_t* n_records);
void otg_bam_sink_abort(otg_bam_sink* sink);
const char* otg_bam_sink_error(const otg_bam_sink* sink);
/* The `samtools merge -pco` step: coordinate-sorted BAMs with identical target lists (per-sample allele BAMs) into one BAM + BAI.  Header:
 * the @HD line above, the first input's @SQ lines, then every other header line of the inputs in input order, a line already present
 * verbatim dropped.  Records are copied unchanged in a k-way merge by (target, position): ties go to the earlier input and keep file order
 * within an input.  OTG_ERR_ARG with the offending file in otg_last_error(NULL): two @RG lines with the same ID (a sample given twice), two
 * @PG ID:otter lines whose OF: differ, different target lists, an unsorted, damaged or truncated input (a file
 * that does not end with the BGZF EOF block included); a refused merge leaves no <out_path> and no <out_path>.bai, stale ones included.  Every
 * input stays open during the merge: n is bounded by the process's limit on open files.  *n_records (nullable) = records written. */
int  otg_bam_merge(const char* const* bam_paths, uint32_t n, const char* out_path, int32_t threads, int32_t level, uint64_t* n_records);

/* The dispatcher keeps its per-device contexts (and their HBM workspaces) for the next job of the process; this frees them. */
void otg_assemble_files_release(void);

/* The batch sizes otg_assemble_files cuts a shard of `n_regions` regions into (batch_regions as in the job; 0 = the library's plan).
 * Writes at most `capacity` sizes, *n_batches = how many there are; OTG_ERR_CAPACITY when they do not fit. */
int otg_assemble_batch_plan(uint32_t n_regions, uint32_t batch_regions, uint32_t* sizes, uint32_t capacity, uint32_t* n_batches);

#ifdef __cplusplus
}
#endif
#endif /* OTTER_GPU_H */

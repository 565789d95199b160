// otg_common.hpp — shared host-side plumbing of libotter_gpu.so (HIP runtime only, no torch).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/otter_gpu.h"

#define OTG_NULL_OFF (-(1 << 30))

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// The rows of an allele operator on the device: row i is arena[off[i] .. + len[i]).  A caller's rows come through otg_rows_check and
// otg_rows_upload into the operator's own slot pair (64 zero bytes behind the arena: the kernels read past a row's end); a cohort's lie
// in its staging area (cohort.hip).  Kernels and their argument structs take it whole.
struct OtgRows { const uint8_t* arena; const uint64_t* off; const uint32_t* len; };

// What an operator with segments leaves on the context: n summaries and n + 1 offsets in its RES slot, `total` segments in its SEGS slot
// (otg_seg_collect, otg_seg_device_results) and its two HIP-event times.  valid: such a call with n > 0 has succeeded since the last one began.
struct OtgSegLast {
  uint32_t n = 0; uint64_t total = 0; bool valid = false;
  double ms[2] = {0.0, 0.0};
};

struct otg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop;
  std::string err;
  int exp_variant = 1;
  long long exp_probe_mismatches = 0;             // of the chosen variant against the host libm over the probe set of otg_create (otg_api.hip)
  int n_cu = 256;
  uint32_t max_seq_len = 65536;   // longest sequence of the current batch (sizes the tier-3 edit workspace)
  // grow-only device scratch, keyed by purpose
  std::vector<DevBuf> pool;
  // resident batch of the L3 pipeline
  struct Pipeline* pipe = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // side streams of the gap-affine chain: on small batches the register tiers run next to each other (wfa_affine.hip); created on first use
  hipStream_t tier_stream[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // Which of the two optional bit-parallel edit tiers run (wfa_edit.hip): decided per KIND of pass (0 = distance matrix / operator-level call,
  // 1 = reassignment; set around the call) from the tier loads the previous pass of that kind left behind (a job's batches are alike), copied to
  // pinned host memory behind the chain — no host synchronisation; without history, from the number of task slots.
  int edit_pass_kind = 0;
  uint32_t* edit_hist = nullptr;                  // pinned: [kind][16] = tier input counts of the last pass
  hipEvent_t edit_hist_ev[2] = {nullptr, nullptr};
  uint32_t edit_hist_mask[2] = {0u, 0u};          // the mask that pass ran with (0: no history)
  double last_score_ms = 0.0, last_prov_ms = 0.0;  // HIP-event times of the two device passes of the latest otg_edit_align_batch (otg_edit_align_last_ms)
  uint32_t last_align_tiers[2] = {0u, 0u};         // tasks the LDS / the global-row tier of the latest adaptive otg_edit_align_heur_batch finished (otg_edit_align_last_tiers)
  double last_kmer_count_ms = 0.0, last_kmer_epi_ms = 0.0;  // HIP-event times of the latest otg_kmer_usage_batch (otg_kmer_usage_last_ms)
  hipEvent_t ev2 = nullptr;                       // third timing event, created on first use (kmer_usage.hip, motif.hip)
  double last_motif_count_ms = 0.0, last_motif_reduce_ms = 0.0;   // HIP-event times of the latest otg_motif_batch / otg_motif_cohort (otg_motif_last_ms)
  uint32_t last_motif_n = 0, last_motif_stride = 0;               // the shape of the results in SLOT_MOTIF_OUT (otg_motif_device_results)
  OtgSegLast last_repeat;                                         // the latest otg_repeat_batch / otg_repeat_cohort: SLOT_REPEAT_RES / SLOT_REPEAT_SEGS, ms = runs, select
  OtgRows last_repeat_rows = {nullptr, nullptr, nullptr};         // where that repeat call read its alleles (n = last_repeat.n): otg_unitset_repeats reads them in place
  uint64_t repeat_serial = 0;                                     // counts the repeat calls on the context: a discovery remembers which one it read
  OtgRows last_motif_rows = {nullptr, nullptr, nullptr};                                  // where the latest motif call read its alleles (n = last_motif_n): otg_unitalign_motifs aligns them in place
  double last_unitalign_ms = 0.0;                                 // HIP-event time of the latest unit alignment (otg_unitalign_last_ms)
  uint32_t last_unitalign_n = 0;                                  // the records in SLOT_UNITALIGN_OUT (otg_unitalign_device_results); 0: none
  double last_tract_ms = 0.0, last_tract_local_ms = 0.0;          // HIP-event times of the latest tract call: both passes, the local pass alone (otg_tract_last_ms)
  uint32_t last_tract_n = 0;                                      // the records in SLOT_TRACT_OUT (otg_tract_device_results); 0: none
  OtgSegLast last_unitparse;                                      // the latest unit parse: SLOT_UNITPARSE_RES / SLOT_UNITPARSE_SEGS, ms = forward, traceback
  OtgSegLast last_locus;                                          // the latest locus call: SLOT_LOCUS_OUT / SLOT_UNITPARSE_SEGS, ms = both passes, the local pass; a later unit parse ends it
  // the latest otg_unitset_repeats: SLOT_UNITSET_RES (sets, set_first) / SLOT_UNITSET_UNITS (unit records, unit_off, unit_len, bytes)
  struct UnitsetLast {
    uint32_t n_groups = 0, n_alleles = 0; uint64_t n_units = 0, unit_bytes = 0, repeat_serial = 0; bool valid = false;
    double ms[2] = {0.0, 0.0};                                    // candidates and vote, pair alignments and select
    std::vector<uint32_t> group_first;                            // the caller's grouping (otg_unitset_locus maps alleles to sets by it)
  } last_unitset;
  // the latest otg_assemble_spread: SLOT_SPREAD_OUT (records, unit_off, unit records) / SLOT_SPREAD_READS; ms = total, the reads' locus call,
  // the consensus locus call, the stats kernel
  struct SpreadLast {
    uint32_t n_alleles = 0, n_reads = 0; uint64_t n_units = 0; bool valid = false;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
  } last_spread;
  uint32_t last_locus_tiers[2] = {0u, 0u};                        // tasks the narrow / the wide tier of that call's local pass took (otg_locus_last_tiers)
  double last_kernel_ms = 0.0;                    // HIP-event time of the kernels of the latest operator-level call that reports one (otg_last_kernel_ms)
  // the latest genotype clustering with a metric (genotype_edit.hip): times of its two parts (otg_genotype_metric_last_ms), whether the edit
  // matrix was built, and where its counters lie in SLOT_GTE_CLS
  double last_gt_align_ms = 0.0, last_gt_cluster_ms = 0.0;
  bool gt_edit_ran = false;
  size_t gt_edit_cnt_off = 0;
  // aligner heuristic of the L1 calls and of the running pipeline (otg_set_heuristic / otg_params.heuristic; wfa_adaptive.hip)
  int heur_strategy = OTG_HEURISTIC_NONE, heur_min_wf_len = 10, heur_max_dist = 50, heur_steps = 1;
  // What the latest tier chain on this context left behind, for otg_affine_last_routing: which chain it was (the byte offset of its group in
  // OtgCounters, set by otg_counters; -1: none yet) and, recorded by otg_launch_affine_todo once a launch is enqueued whole (n_tasks = 0 until then), the shape of the exact gap-affine launch whose
  // counters, lists (SLOT_TODO) and bounds (SLOT_BT_POOL) are still on the device.
  int last_chain = -1;
  struct AffineLast {
    uint32_t n_tasks = 0;
    bool hbm_tiers = false;         // tiers A and B ran (false: the generic kernel alone)
    bool bounded = false;           // the score-bound pass ran
    bool sublist = false;           // the launch worked on a list of task slots, not on all of them
    int reg_mask = 0;               // register tiers that ran (0: no sort either)
    const void* scores_at = nullptr;   // where the launch wrote its scores; compared with SLOT_SCORES before that slot is read, never dereferenced
  } affine_last;
  // cohort staging area of otg_cohort_begin .. otg_cohort_end (cohort.hip); created on first use
  struct Cohort* cohort = nullptr;
};

extern thread_local std::string g_otg_err;

int otg_fail(otg_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, call)                                                                      \
  do {                                                                                          \
    hipError_t e__ = (call);                                                                    \
    if (e__ != hipSuccess)                                                                      \
      return otg_fail(ctx, OTG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                      __FILE__, __LINE__);                                                      \
  } while (0)

// Grow-only device allocation slot; returns nullptr on failure (error recorded).
void* otg_slot(otg_ctx* ctx, int slot, size_t bytes);
// A caller's rows (host arrays): the NULL and range refusals under the entry's name `who` (max_len, nullable: the longest row), and the
// copy into the slot pair slot_seq (arena_bytes + 64, the tail zeroed) / slot_meta (off | len), enqueued on ctx->stream.
int otg_rows_check(otg_ctx* ctx, const char* who, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* off, const uint32_t* len, uint32_t n,
                   uint32_t* max_len);
int otg_rows_upload(otg_ctx* ctx, int slot_seq, int slot_meta, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* off, const uint32_t* len,
                    uint32_t n, OtgRows* out);
// The segments of the latest call behind the context's member `which` into the caller's buffer, and where its results lie on the device; who = the exported
// entry, noun = what the refusal calls the results ("repeat", "unit parse"), sum_bytes / seg_bytes = the sizes of a summary and a segment.
int otg_seg_collect(otg_ctx* ctx, const char* who, const char* noun, OtgSegLast otg_ctx::*which, int slot_segs, size_t seg_bytes, void* segs, uint64_t capacity);
int otg_seg_device_results(otg_ctx* ctx, const char* who, const char* noun, OtgSegLast otg_ctx::*which, int slot_res, int slot_segs, size_t sum_bytes, uint32_t* n,
                           const void** sums, const uint64_t** seg_off, const void** segs, uint64_t* total);
// The tail of an emit entry: the size into *out_len, the text into the caller's buffer, or OTG_ERR_CAPACITY
int otg_text_out(const char* who, const std::string& text, char* out, uint64_t capacity, uint64_t* out_len);

// The refusals otg_unitalign_check and otg_unitparse_check share, in their order: the NULL test (lists_null: one of the caller's own lists is
// missing), per unit the caller's length rule (unit_rule(k, length) -> its refusal or OTG_OK) and the range, the caller's own lists
// (lists() -> likewise), the task cap.
template <typename UnitRule, typename Lists>
int otg_unit_lists_check(otg_ctx* ctx, const char* who, bool lists_null, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                         const uint32_t* unit_len, uint32_t n_units, uint32_t n_tasks, UnitRule unit_rule, Lists lists)
{
  if ((n_units && (!unit_off || !unit_len || (unit_bytes && !unit_arena))) || lists_null) return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL argument", who);
  for (uint32_t k = 0; k < n_units; ++k) {
    if (int rc = unit_rule(k, unit_len[k])) return rc;
    if (unit_off[k] > unit_bytes || unit_len[k] > unit_bytes - unit_off[k])
      return otg_fail(ctx, OTG_ERR_ARG, "%s: unit %u (offset %llu, length %u) lies outside the %llu-byte unit arena", who, k, (unsigned long long)unit_off[k],
                      unit_len[k], (unsigned long long)unit_bytes);
  }
  if (int rc = lists()) return rc;
  if (n_tasks > (1u << 24)) return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: %u tasks in one call, at most %u", who, n_tasks, 1u << 24);
  return OTG_OK;
}

// cluster.hip: regions of up to this many valid reads (assemble) / alleles (genotype) keep their clustering scratch in LDS; the callers of
// otg_launch_cluster / otg_launch_genotype list the regions above it, which run on the wide kernels
constexpr uint32_t OTG_CLUSTER_NMAX = 256;
enum {
  SLOT_ARENA = 0, SLOT_TASKS, SLOT_SCORES, SLOT_CELLS, SLOT_COUNTERS /* OtgCounters, otg_chain.hpp */, SLOT_WF_WS, SLOT_CIG_OFF, SLOT_CIG_LEN,
  SLOT_CIG_ARENA, SLOT_BT_POOL, SLOT_ROWTAB, SLOT_REVOPS, SLOT_TASKSTATE, SLOT_TODO, SLOT_AUX0, SLOT_AUX1,
  SLOT_AUX2, SLOT_AUX3, SLOT_AUX4, SLOT_AUX5, SLOT_AUX6, SLOT_AUX7, SLOT_AUX8, SLOT_AUX9,
  SLOT_P0, SLOT_P1, SLOT_P2, SLOT_P3, SLOT_P4, SLOT_P5, SLOT_P6, SLOT_P7, SLOT_P8, SLOT_P9,
  SLOT_P10, SLOT_P11, SLOT_P12, SLOT_P13, SLOT_P14, SLOT_P15, SLOT_P16, SLOT_P17, SLOT_P18, SLOT_P19,
  SLOT_P20, SLOT_P21, SLOT_P22, SLOT_P23, SLOT_P24, SLOT_P25, SLOT_P26, SLOT_P27, SLOT_P28, SLOT_P29,
  SLOT_KMER_SEQ, SLOT_KMER_META, SLOT_KMER_HIST, SLOT_KMER_OUT,     // otg_kmer_usage_batch (kmer_usage.hip); OUT stays valid for the device results
  SLOT_KMER_BLK,                                                    // tier L of otg_kmer_usage_resident: gc counts and the workgroup prefix
  SLOT_GTE_CLS, SLOT_GTE_TASKS, SLOT_GTE_SCORES, SLOT_GTE_DEN, SLOT_GTE_TODO,   // the edit metric of the genotype clustering (genotype_edit.hip)
  SLOT_MOTIF_SEQ, SLOT_MOTIF_META, SLOT_MOTIF_OFF, SLOT_MOTIF_M, SLOT_MOTIF_PLANES, SLOT_MOTIF_OUT,   // otg_motif_batch (motif.hip); OUT stays valid for the device results
  SLOT_REPEAT_SEQ, SLOT_REPEAT_META, SLOT_REPEAT_OFF, SLOT_REPEAT_CNT, SLOT_REPEAT_PLANES, SLOT_REPEAT_RUNS, SLOT_REPEAT_STACK, SLOT_REPEAT_SCRATCH,   // otg_repeat_batch (repeat.hip)
  SLOT_REPEAT_RES, SLOT_REPEAT_SEGS,                                // its summaries and offsets / its segments: they stay valid for the device results
  SLOT_UNITALIGN_SEQ, SLOT_UNITALIGN_META, SLOT_UNITALIGN_UNITS, SLOT_UNITALIGN_BINS, SLOT_UNITALIGN_ORDER,   // otg_unitalign_batch (unitalign.hip)
  SLOT_UNITALIGN_OUT,                                               // its records: they stay valid for the device results
  SLOT_UNITPARSE_SEQ, SLOT_UNITPARSE_META, SLOT_UNITPARSE_UNITS, SLOT_UNITPARSE_PLAN, SLOT_UNITPARSE_TRACE,   // otg_unitparse_batch (unitparse.hip)
  SLOT_UNITPARSE_RES, SLOT_UNITPARSE_SEGS,                          // its summaries and offsets / its segments: they stay valid for the device results
  SLOT_TRACT_SEQ, SLOT_TRACT_META, SLOT_TRACT_UNITS, SLOT_TRACT_BINS, SLOT_TRACT_ORDER, SLOT_TRACT_SUB,   // otg_tract_batch (tract.hip); SUB: the sub-rows of the second pass
  SLOT_TRACT_OUT,                                                   // its records: they stay valid for the device results
  SLOT_LOCUS_SEQ, SLOT_LOCUS_META, SLOT_LOCUS_UNITS, SLOT_LOCUS_SUB,   // otg_locus_batch (locus.hip); SUB: the sub-rows of the second pass and the task order
  SLOT_LOCUS_OUT,                                                   // its records and segment offsets: they stay valid for the device results
  SLOT_UNITSET_CAND, SLOT_UNITSET_WORK, SLOT_UNITSET_TASKS, SLOT_UNITSET_PAIRS,   // otg_unitset_repeats (unitset.hip): candidates, ranked classes and offsets, pair tasks, pair records
  SLOT_UNITSET_RES, SLOT_UNITSET_UNITS,                             // its sets and offsets / its units: they stay valid for the device results
  SLOT_UNITSET_LOCUS,                                               // otg_unitset_locus: the task records before they are spread over the alleles
  SLOT_SPREAD_META,                                                 // otg_assemble_spread (spread.hip): the rows of the reads and of the consensus alleles, their task lists
  SLOT_SPREAD_READS, SLOT_SPREAD_OUT,                               // its read records / its records, unit offsets and unit records: they stay valid for the device results
  SLOT_COUNT
};

// The region string of a BED record as the VCF writer prints it in the ID column (BED::toScString, src/anbed.cpp:17-20: coordinates unsigned);
// appended to o.  otg_emit_vcf_lines writes it, otg_copies_files looks VCF records up by it.
inline void otg_region_name(std::string& o, const char* chr, uint32_t chr_len, int32_t start, int32_t end)
{
  o.append(chr, chr_len);
  o += ':'; o += std::to_string((uint32_t)start); o += '-'; o += std::to_string((uint32_t)end);
}

void otg_pipeline_free(otg_ctx* ctx);
int64_t otg_pipeline_run_regions(otg_ctx* ctx);
// pipeline.hip: the batch of the latest completed otg_assemble_run where it lies on the device, valid until the next submit on the context:
// the reads' arena (64 zero bytes behind it), the read descriptors as the run left them, the regions, the final labels, the region results,
// the consensus records and their arena (16 bytes behind it, not zeroed: exactly what the sixteen-byte loads of the locus kernels need, which
// read at most 15 bytes past a row and never use them; the 64 zero bytes of a caller's rows are not promised here); h_regions = the submitted regions on the host.  results is NULL for a batch
// without regions or reads, alleles and seqs without alleles.
struct OtgAssembleView {
  uint32_t n_reads, n_regions, n_alleles;
  const otg_region* h_regions;
  const uint8_t* arena; const otg_read* reads; const otg_region* regions; const int32_t* labels;
  const otg_region_result* results; const otg_allele* alleles; const uint8_t* seqs;
};
bool otg_pipeline_view(otg_ctx* ctx, OtgAssembleView* view);
void otg_cohort_free(otg_ctx* ctx);
// ingest.hip: gives a BAM handle the sample list of a cohort job (what otg_bam_sample_index reads from an allele BAM's header)
void otg_bam_set_samples(otg_bam* b, const char* const* names, uint32_t n, int32_t offset_l, int32_t offset_r);

// Contexts that share a device (the dispatcher runs 2-4 per GPU) size their multi-gigabyte workspaces from hipMemGetInfo; two of them doing so
// at the same moment would both claim the same free bytes.  Every "measure free memory, then allocate" section holds this lock.
std::mutex& otg_device_mutex(int device);

#if defined(__HIPCC__)
// One atomic add per WAVE, issued with exec forced to lane 0 and no divergent branch in the HIP source.
// (A source-level `if (lane == 0) atomicAdd(..)` + readfirstlane at the head of a persistent-wave loop was
// structurized by hipcc 7.2 so that lanes 1..63 re-entered the loop with lane 0 masked: an endless loop.)
// Call only from wave-uniform control flow.
__device__ __forceinline__ uint32_t otg_wave_atomic_add(uint32_t* ctr, uint32_t val)
{
  uint32_t r;
  uint64_t saved;
  asm volatile(
      "s_mov_b64 %1, exec\n\t"
      "s_mov_b64 exec, 1\n\t"
      "global_atomic_add %0, %2, %3, off sc0\n\t"
      "s_waitcnt vmcnt(0)\n\t"
      "s_mov_b64 exec, %1"
      : "=&v"(r), "=&s"(saved)
      : "v"(ctr), "v"(val)
      : "memory");
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
}

__device__ __forceinline__ int otg_imax(int a, int b) { return a > b ? a : b; }
// Maximum over the 64 lanes (DPP row shifts + row broadcasts), returned wave-uniform.
__device__ __forceinline__ int otg_wave_max_i32(int v)
{
  constexpr int NEG = -2147483647 - 1;
  v = otg_imax(v, __builtin_amdgcn_update_dpp(NEG, v, 0x111, 0xf, 0xf, false));   // row_shr:1
  v = otg_imax(v, __builtin_amdgcn_update_dpp(NEG, v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = otg_imax(v, __builtin_amdgcn_update_dpp(NEG, v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = otg_imax(v, __builtin_amdgcn_update_dpp(NEG, v, 0x118, 0xf, 0xf, false));   // row_shr:8  -> lane 15 of each row = row max
  v = otg_imax(v, __builtin_amdgcn_update_dpp(NEG, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1, 3
  v = otg_imax(v, __builtin_amdgcn_update_dpp(NEG, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2, 3
  return __builtin_amdgcn_readlane(v, 63);
}

// Band of the bit-parallel edit tiers (myers_edit.hip) for a cost threshold K.  Rows i (pattern), columns j (text),
// d = m - n >= 0; the alignment starts on a diagonal e0 in [0, pbf] and ends on e1 in [d - pef, d].  A path of cost
// <= K that visits diagonal e pays at least |e - e0| + |e - e1| indels and needs |e0 - e1| <= K, hence
//   e <= KU = min((K + d + pbf) / 2, K + pbf)      and      e >= -KL,
//   KL = min((K - d + pef) / 2, K) while the alignment may start on diagonal 0 (K >= d - pef), and beyond that — a start on diagonal 0 would
//   cost more than K, so e0 >= d - pef - K and the lowest diagonal any path can visit is that one — KL = K - (d - pef) < 0: the band's
//   lower edge lies ABOVE diagonal 0.  (A read that covers only the end of its pattern, d = pbf = 1500, K = 300: 450 diagonals instead of
//   1650 — the reassignment pass of a batch with clipped reads ran on tiers four times as wide as its alignments needed.)
__device__ __forceinline__ void otg_myers_band(int K, int d, int pbf, int pef, int* KL, int* KU)
{
  const int u1 = (K + d + pbf + 1) / 2, u2 = K + pbf;
  *KU = u1 < u2 ? u1 : u2;
  int l = (K - d + pef + 1) / 2;
  if (l > K) l = K;
  if (K - d + pef < 0) l = K - d + pef;
  *KL = l;
}
// Largest threshold K whose band fits R rows of lane schedule (KL + KU <= R, monotone in K).
// W_p of SURVEY.md §8d in closed form: wavefront cells an edit-distance WFA evaluates up to score s when the wavefront of score t spans
// the diagonals [max(-pbf - t, -m), min(tbf + t, n)] (pbf / tbf = free pattern / text prefix, 0 for a global alignment).
__device__ __forceinline__ unsigned long long otg_edit_wfa_cells(int s, int m, int n, int pbf, int tbf)
{
  if (s < 0) return 0ull;
  if (pbf > m) pbf = m;
  if (tbf > n) tbf = n;
  const long long kh = s < n - tbf ? s : n - tbf, kl = s < m - pbf ? s : m - pbf;
  const long long sum_hi = (kh + 1) * tbf + kh * (kh + 1) / 2 + ((long long)s - kh) * n;
  const long long sum_lo = (kl + 1) * pbf + kl * (kl + 1) / 2 + ((long long)s - kl) * m;
  return (unsigned long long)(sum_hi + sum_lo + (long long)s + 1);
}

__device__ __forceinline__ int otg_myers_threshold(int R, int d, int pbf, int pef)
{
  int lo = 0, hi = R;            // invariant: band(lo) fits (K = 0: KL + KU <= pbf + small), band(hi + 1) unknown
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    int kl, ku;
    otg_myers_band(mid, d, pbf, pef, &kl, &ku);
    if (kl + ku <= R) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- match-run extension helpers shared by the wavefront kernels -------------------------------------
__device__ __forceinline__ uint64_t otg_load8(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

// Lane shifts across the whole wave (GFX9 DPP wave_shr:1 / wave_shl:1; the lane at the open end keeps its own value).
__device__ __forceinline__ int otg_dpp_shr1(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }   // lane i <- lane i-1
__device__ __forceinline__ int otg_dpp_shl1(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x130, 0xf, 0xf, false); }   // lane i <- lane i+1

// Ends-free end test of a fully extended cell (text offset h, pattern offset v): one sequence is consumed and what is left of the other is free.
__device__ __forceinline__ bool otg_ends_free_done(int h, int v, int pl, int tl, int pef, int tef)
{
  return (h >= tl && pl - v <= pef) || (v >= pl && tl - h <= tef);
}

// Lane-private: number of equal leading bytes of P+v.. and T+h.., looking at most 16 bytes ahead and at most `rem`.
__device__ __forceinline__ int otg_match16(const uint8_t* P, const uint8_t* T, int v, int h, int rem)
{
  const uint64_t xl = otg_load8(P + v) ^ otg_load8(T + h), xh = otg_load8(P + v + 8) ^ otg_load8(T + h + 8);
  const int m = xl ? (__builtin_ctzll(xl) >> 3) : (xh ? 8 + (__builtin_ctzll(xh) >> 3) : 16);
  return m < rem ? m : rem;
}

// Lane-private: number of equal leading bytes of P+v.. and T+h.., looking at most 64 bytes ahead and at most `rem`.
// Eight independent 8-byte loads per operand are issued back to back (one latency, not eight).
__device__ __forceinline__ int otg_match64(const uint8_t* P, const uint8_t* T, int v, int h, int rem)
{
  uint64_t x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = (8 * i < rem) ? (otg_load8(P + v + 8 * i) ^ otg_load8(T + h + 8 * i)) : ~0ull;
  int m = 64;
#pragma unroll
  for (int i = 7; i >= 0; --i) if (x[i]) m = 8 * i + (__builtin_ctzll(x[i]) >> 3);
  return m < rem ? m : rem;
}

// Wave-cooperative (all arguments wave-uniform): extends ONE diagonal, 64 lanes x 8 bytes = 512 bytes per iteration.
__device__ __forceinline__ int otg_wave_match(const uint8_t* P, const uint8_t* T, int v, int h, int rem, int lane)
{
  int total = 0;
  while (total < rem) {
    const int off = total + lane * 8;
    const bool in = off < rem;
    uint64_t x = ~0ull;
    if (in) x = otg_load8(P + v + off) ^ otg_load8(T + h + off);
    const int m = x ? (int)(__builtin_ctzll(x) >> 3) : 8;
    const unsigned long long stop = __ballot(m < 8);          // lanes beyond `rem` report a mismatch at byte 0
    if (stop) {
      const int first = (int)__builtin_ctzll(stop);
      total += first * 8 + __builtin_amdgcn_readlane(m, first);
      break;
    }
    total += 512;
  }
  return total < rem ? total : rem;
}
#endif

// ---- device-resident launch helpers implemented in the .hip files -------------------------------------
// All take device pointers; they enqueue on ctx->stream and do not synchronise unless stated.

// wfa_edit.hip
int otg_launch_edit(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, uint32_t n_tasks,
                    int32_t* d_scores, uint64_t* d_cells, float* kernel_ms, uint64_t* launches);

// edit_align.hip: scores (the chain above), then the diamond provenance pass and the op strings (host arrays in, host arrays out).  Tasks with
// free ends take the ends-free region and kernels.  finished (nullable): as below, the tasks given to the LDS tier / the global-row tier
int otg_launch_edit_align(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const otg_align_task* h_tasks, uint32_t n_tasks,
                          int32_t* scores_out, uint32_t* len_out, uint8_t* d_cig_base, const uint64_t* cig_slot, double* score_ms, double* prov_ms,
                          uint32_t* finished = nullptr);
// the same under wfadaptive (the caller has set ctx's heuristic): the adaptive score chain, then the provenance pass under the cut; also fills
// cells_out (host) and adds the tasks each of its two tiers finished to finished[0] (LDS window) / finished[1] (global row)
int otg_launch_edit_align_adaptive(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const otg_align_task* h_tasks, uint32_t n_tasks,
                                   int32_t* scores_out, uint64_t* cells_out, uint32_t* len_out, uint8_t* d_cig_base, const uint64_t* cig_slot,
                                   double* score_ms, double* prov_ms, uint32_t finished[2]);

// bit-parallel edit tiers (myers_edit.hip), narrowest first: <blocks per lane, lanes per pair> = <1,8> <2,8> <3,8> <2,16> <3,16> <2,32> <2,64> <4,64>
constexpr int OTG_MYERS_TIERS = 8;
// register-resident gap-affine tiers (wfa_affine_reg.hpp)
constexpr int OTG_REG_TIERS = 5;
// d_pblk / d_masks (both or neither): the per-read plane table of the batch (otg_launch_read_masks) and, per task slot, the first table block of
// the task's pattern or 0xffffffff — the bit-parallel tiers then take such a pattern's match masks from the table (myers_masks.hpp).
// d_codes (nullable, only with the table): one row code per arena byte, written by otg_launch_read_masks for every read it covers; a task with
// table blocks then reads its text from there
namespace otg_myers { struct PlaneBlock; }
int otg_launch_myers(otg_ctx* ctx, int tier, const uint8_t* d_arena, const otg_align_task* d_tasks, const uint32_t* d_todo,
                     const uint32_t* d_n_todo, uint32_t n_tasks, int32_t* d_scores, uint64_t* d_cells,
                     uint32_t* ticket, uint32_t* n_overflow, uint32_t* overflow_list,
                     const uint32_t* d_pblk = nullptr, const otg_myers::PlaneBlock* d_masks = nullptr, const uint8_t* d_codes = nullptr);
int otg_launch_edit_todo(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const uint32_t* d_todo,
                         const uint32_t* d_n_todo, uint32_t n_task_slots, int32_t* d_scores, uint64_t* d_cells,
                         float* kernel_ms, uint64_t* launches,
                         const uint32_t* d_pblk = nullptr, const otg_myers::PlaneBlock* d_masks = nullptr, const uint8_t* d_codes = nullptr);
int otg_launch_read_masks(otg_ctx* ctx, const uint8_t* d_arena, const otg_read* d_reads, const uint32_t* d_read_region, uint32_t n_reads,
                          const uint32_t* d_first_blk, otg_myers::PlaneBlock* d_masks, uint32_t* d_read_blk, uint8_t* d_codes = nullptr);
int otg_launch_affine_todo(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const uint32_t* d_todo,
                           const uint32_t* d_n_todo, uint32_t n_task_slots, int x, int o, int e, int32_t* d_scores,
                           const uint64_t* d_cig_off, uint32_t* d_cig_len, uint8_t* d_cig_arena, uint64_t* d_cells,
                           float* kernel_ms = nullptr, uint64_t* launches = nullptr);

// wfa_affine.hip — forward + backtrace + unpack; CIGARs land in d_cig_arena at d_cig_off (precomputed
// exclusive prefix of pattern_len+text_len per task), lengths in d_cig_len.  Synchronises internally
// (multi-round when the backtrace pool is smaller than the batch needs).
int otg_launch_affine(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, uint32_t n_tasks,
                      int x, int o, int e, int32_t* d_scores, const uint64_t* d_cig_off, uint32_t* d_cig_len,
                      uint8_t* d_cig_arena, uint64_t* d_cells);

// wfa_adaptive.hip — the same two chains under wfadaptive(min_wf_len, max_dist, steps); otg_launch_edit_todo / otg_launch_affine_todo hand
// over to them when ctx->heur_strategy says so
int otg_launch_edit_adaptive_todo(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const uint32_t* d_todo,
                                  const uint32_t* d_n_todo, uint32_t n_task_slots, int32_t* d_scores, uint64_t* d_cells,
                                  float* kernel_ms, uint64_t* launches);
int otg_launch_affine_adaptive_todo(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const uint32_t* d_todo,
                                    const uint32_t* d_n_todo, uint32_t n_task_slots, int x, int o, int e, int32_t* d_scores,
                                    const uint64_t* d_cig_off, uint32_t* d_cig_len, uint8_t* d_cig_arena, uint64_t* d_cells,
                                    float* kernel_ms, uint64_t* launches);

// cluster.hip
int otg_launch_cluster(otg_ctx* ctx, const otg_params* P, const double* d_dist, const uint64_t* d_dist_off,
                       const uint32_t* d_read_len, const uint64_t* d_len_off, const uint32_t* d_n_valid,
                       uint32_t n_regions, uint32_t n_max, const uint32_t* h_wide, uint32_t n_wide, int32_t* d_labels, int32_t* d_ic,
                       int32_t* d_fc, double* d_bounds, int32_t* d_err, const otg_cluster_trace* d_trace = nullptr, int exp_variant = -1);
// out[i] = otg_exp<variant>(d_x[i]) in place: the function cluster_kernel calls, on its own (otg_exp_device)
int otg_launch_exp(otg_ctx* ctx, double* d_x, uint64_t n, int variant);

// poa.hip
int otg_launch_poa(otg_ctx* ctx, const uint8_t* d_seq_arena, const uint8_t* d_cig_arena,
                   const otg_poa_member* d_members, uint32_t n_members, const otg_poa_graph* d_graphs,
                   const otg_poa_graph* h_graphs, uint32_t n_graphs, uint32_t* d_out_len,
                   std::vector<uint64_t>& node_off);
// the same for graphs and members that are on the device only: planned on the device, no host copy of the graphs (see the definition)
int otg_launch_poa_resident(otg_ctx* ctx, const uint8_t* d_seq_arena, const uint8_t* d_cig_arena,
                            const otg_poa_member* d_members, uint32_t n_members, const otg_poa_graph* d_graphs, uint32_t n_graphs, uint32_t* d_out_len);

// otg_api.hip: anallele_cluster on device-resident inputs (memset of the outputs, ev0, the kernels below, ev1); see its definition
int otg_genotype_resident(otg_ctx* ctx, const otg_params* params, const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len,
                          const uint32_t* d_first, const uint32_t* d_n, const uint32_t* h_n_alleles, uint32_t n_regions, const uint64_t* d_poff,
                          uint64_t n_pairs, uint64_t na, int32_t* d_gt, double* d_hsd, int32_t* d_ngt, double* d_height = nullptr,
                          int metric = OTG_GT_METRIC_LENGTH, uint32_t max_len = 0);

// genotype_edit.hip — the first matrix of anallele_cluster under OTG_GT_METRIC_EDIT, see the definitions: the argument check of the metric
// entry points (unknown metric: OTG_ERR_ARG; pair slots beyond 2^32: OTG_ERR_CAPACITY, nothing allocated), the longest of n lengths on the
// device (synchronises), the launch (allele classes, pair tasks, the exact edit chain, the fan-out into SLOT_P20) and what the host reads
// once the stream has been waited for (times, alignments run, OTG_ERR_CAPACITY when the chain gave a pair up)
int otg_genotype_metric_fits(otg_ctx* ctx, const char* who, int metric, uint64_t n_pairs);
int otg_device_max_u32(otg_ctx* ctx, const uint32_t* d_v, uint64_t n, uint32_t* out);
int otg_launch_genotype_edit_matrix(otg_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_first,
                                    const uint32_t* d_n, uint32_t n_regions, const uint64_t* d_poff, uint64_t n_pairs, uint64_t na, uint32_t max_len);
int otg_genotype_metric_finish(otg_ctx* ctx, int metric, uint64_t* n_aligned);

// kmer_usage.hip: the workspace refusal of otg_kmer_usage_batch (OTG_ERR_CAPACITY, nothing allocated) and its launch part on device-resident
// rows; see the definitions
int otg_kmer_usage_fits(otg_ctx* ctx, const char* who, uint32_t n, int32_t k);
int otg_kmer_usage_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const uint32_t* h_blk,
                            uint32_t n, int32_t k, double* usage_out, double* gc_out, double* hsd_out);

// motif.hip: the argument refusals of otg_motif_batch (max_period, slack; unit_stride against the longest row) and its launch part on
// device-resident rows; see the definitions
int otg_motif_args(otg_ctx* ctx, const char* who, uint32_t max_period, uint32_t slack);
int otg_motif_stride_fits(otg_ctx* ctx, const char* who, uint32_t max_len, uint32_t max_period, uint32_t unit_stride);
int otg_motif_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, uint32_t n,
                       uint32_t max_period, uint32_t slack, otg_motif* out, uint8_t* unit_out, uint32_t unit_stride);
// motif.hip: the HBM plane tier, shared with repeat.hip.  The longest allele of the LDS tier (0 under OTG_MOTIF_WIDE); the scan of the plane
// words per allele into d_ploff (n + 1; an allele of the LDS tier or without a period has none) and *d_total; the pack kernel on those offsets.
uint32_t otg_motif_lds_len();
void otg_motif_plane_scan(otg_ctx* ctx, const uint32_t* d_len, uint32_t n, uint32_t max_period, uint32_t lds_len, uint64_t* d_ploff, uint64_t* d_total);
void otg_motif_pack_planes(otg_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len, uint32_t n, const uint64_t* d_ploff,
                           uint32_t* d_planes);
// unitalign.hip: the launch part of the unit alignment on device-resident alleles and units.  Allele a is rows.arena[rows.off[a] .. + rows.len[a]) (the
// arena extends 15 bytes past every row).  Unit k is d_units[d_unit_off[k] .. + d_unit_len[k]), or with d_unit_off == NULL the slot
// d_units + k * unit_stride whose length is d_motifs[k].period.  Task t aligns allele d_task_seq[t] to unit d_task_unit[t]; NULL lists: t.
struct OtgUnitSource {
  const uint8_t* d_units; const uint64_t* d_unit_off; const uint32_t* d_unit_len; const otg_motif* d_motifs; uint32_t unit_stride;
};
int otg_unitalign_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const OtgUnitSource& units,
                           const uint32_t* d_task_seq, const uint32_t* d_task_unit, uint32_t n_tasks, otg_unitalign* out);
// its refusals of a caller's units and task lists (host arrays), and the upload of both into the context's slots
int otg_unitalign_check(otg_ctx* ctx, const char* who, uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                        const uint32_t* unit_len, uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks);
int otg_unitalign_upload(otg_ctx* ctx, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units,
                         const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks, OtgUnitSource* units, const uint32_t** d_task_seq,
                         const uint32_t** d_task_unit, int slot = SLOT_UNITALIGN_UNITS);
// tract.hip: the launch part of the tract mode on device-resident alleles and units, arguments as otg_unitalign_resident.  The local pass,
// then otg_unitalign_resident on the tracts as sub-rows of the same arena, then the merge into SLOT_TRACT_OUT; params has been checked.
int otg_tract_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const OtgUnitSource& units, const uint32_t* d_task_seq,
                       const uint32_t* d_task_unit, uint32_t n_tasks, const otg_tract_params& params, otg_tract* out);
// the params of a tract entry: NULL gives the defaults, scores out of range are OTG_ERR_ARG
int otg_tract_args(otg_ctx* ctx, const char* who, const otg_tract_params* params, otg_tract_params* out);
// What the kernels over unit sets read (unitparse.hip, locus.hip): the alleles, the units (unit k = d_unit_len[k] bytes at units + unit_off[k]), set q = units
// set_first[q] .. set_first[q + 1), task t = allele task_seq[t] against set task_set[t]; all device pointers.  otg_unit_sets_upload copies
// the caller's host arrays into `slot` (enqueued on ctx->stream) and fills the view.
struct OtgSetTasks {
  OtgRows rows;
  const uint8_t* units; const uint64_t* unit_off; const uint32_t* unit_len; const uint64_t* set_first;
  const uint32_t* task_seq; const uint32_t* task_set;
};
int otg_unit_sets_upload(otg_ctx* ctx, int slot, const OtgRows& rows, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                         uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set, uint32_t n_tasks, OtgSetTasks* out);
// unitparse.hip: the refusals of a caller's unit sets and task lists (host arrays), and the launch part of the joint unit parse on
// device-resident alleles (the arena extends 15 bytes past every row).  The units, sets and task lists are host arrays and are uploaded here;
// h_len = the allele lengths on the host, NULL: they are read back from rows.len.
int otg_unitparse_check(otg_ctx* ctx, const char* who, uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                        const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                        const uint32_t* task_set, uint32_t n_tasks);
int otg_unitparse_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const uint32_t* h_len,
                           uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                           uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set, uint32_t n_tasks,
                           otg_unitparse_sum* sums, uint64_t* seg_off, uint64_t* n_segments);
// locus.hip: the launch part of the locus mode, arguments as otg_unitparse_resident.  The local pass over the unit sets, then
// otg_unitparse_resident on the tracts as sub-rows of the same arena, then the merge into SLOT_LOCUS_OUT; params has been checked.
int otg_locus_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const uint32_t* h_len, uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes,
                       const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                       const uint32_t* task_set, uint32_t n_tasks, const otg_tract_params& params, otg_locus* out, uint64_t* seg_off, uint64_t* n_segments);
// repeat.hip: the argument refusals of otg_repeat_batch and its launch part on device-resident rows (cohort.hip), as the motif pair above
int otg_repeat_args(otg_ctx* ctx, const char* who, uint32_t max_period, uint32_t min_copies, uint32_t min_span);
int otg_repeat_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, uint32_t n,
                        uint32_t max_period, uint32_t min_copies, uint32_t min_span, otg_repeat_sum* sums, uint64_t* seg_off, uint64_t* n_segments);

// cluster.hip (genotype_kernel)
int otg_launch_genotype(otg_ctx* ctx, const otg_params* P, const uint8_t* d_arena, const uint64_t* d_seq_off,
                        const uint32_t* d_seq_len, const uint32_t* d_first, const uint32_t* d_n, uint32_t n_regions,
                        const uint64_t* d_pair_off, uint64_t n_pairs_total, uint64_t n_alleles_total, uint32_t a_max,
                        const uint32_t* h_wide, uint32_t n_wide,
                        int32_t* d_gt, int32_t* d_gtl, int32_t* d_gtk, double* d_hsd, int32_t* d_ngt, int32_t* d_reps,
                        int32_t* d_err, double* d_height_l = nullptr, double* d_height_k = nullptr, bool dl_given = false);

// tract.hip — the tract mode of the copy numbers (otg_tract_batch / _motifs / _cohort): where the repeat lies inside a flanked allele, and
// the unit alignment of exactly that stretch.  The reference has no counterpart; include/otter_gpu.h states the rule.
//
// First pass, tr_align: the local wraparound alignment.  The layout is ua_align's (unitalign.hip): one task is a pair (allele, unit), the
// row lives in registers, unit positions across the S = 4 .. 64 lanes of a segment, then 2 and 4 positions per lane; sixteen allele bytes
// per load; a task that has consumed its allele keeps its state while its neighbours go on.  The key is score * 2^SHIFT + begin, ordered by
// one unsigned maximum.  Per row (otg_tract_core.hpp):
//   rotate   position j takes the cell of j - 1, position 0 that of p - 1;
//   cell     the diagonal step and the base outside the unit, each a saturating subtract, and the fresh start i + 1;
//   closure  the skipped unit bases around the cycle: a segmented prefix maximum of the cells biased by j * indel in the score field, and
//            the wrap term from position p - 1, no candidate when its score would not stay positive;
//   best     per position, replaced only by a strictly larger score (the smallest end wins) and only on rows the task still has.
// Tasks are binned as the unit alignment bins them (ua_class, ua_bucket, the scatter of otg_unit_tasks.hpp); the tier is decided per task from
// the call's scores and the unit length (tr_narrow_len).
// Second pass: tr_subrows writes the tracts as rows (off + begin, end - begin; length 0 without a tract) over the SAME arena, indexed by
// task; otg_unitalign_resident aligns them with identity task lists against the call's units (its sixteen-byte loads stay inside the parent
// row's arena); tr_merge joins both results into otg_tract records at the task's own index.
#include "otg_common.hpp"
#include "otg_lane.hpp"
#include "otg_scan.hpp"
#include "otg_tract_core.hpp"
#include "otg_unit_tasks.hpp"
#include <algorithm>
#include <cstdlib>

// cohort.hip: do the alleles of the open cohort batch still lie at d_arena (regrouped, clustered, rows built)?
bool otg_cohort_holds_rows(otg_ctx* ctx, const uint8_t* d_arena);

namespace {

using namespace otg_tract_core;
using namespace otg_lane;

__global__ __launch_bounds__(UA_T) void tr_classify(UaIn in, uint32_t n, otg_tract_params q, bool wide, bool seg64, uint32_t* __restrict__ task_bin,
                                                   uint32_t* __restrict__ hist, otg_tract* __restrict__ out)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t >= n) return;
  const uint32_t L = in.rows.len[in.seq(t)], p = in.unit_len(in.unit(t));
  const uint32_t refusal = tr_refusal(L, p);
  if (refusal || L == 0u) {                                       // nothing to align: the record is final
    otg_tract rec;
    rec.score = rec.begin = rec.end = rec.edits = rec.unit_bases = rec.end_phase = rec.start_phase = 0u;
    rec.flags = refusal ? refusal : OTG_TRACT_NONE;
    out[t] = rec;
    task_bin[t] = UA_NO_BIN;
    return;
  }
  const uint32_t tier = (wide || L > tr_narrow_len(q, p)) ? 1u : 0u;
  const uint32_t bin = (tier * UA_CLASSES + ua_class(p, seg64)) * UA_BUCKETS + (UA_BUCKETS - 1u - ua_bucket(L));      // the longest first
  task_bin[t] = bin;
  atomicAdd(&hist[bin], 1u);
}

// ---- the local alignment: tasks order[first .. first + count), 64 / S to a wave
template <typename K, int S, int R>
__global__ __launch_bounds__(UA_T) void tr_align(UaIn in, otg_tract_params q, const uint32_t* __restrict__ order, uint32_t first, uint32_t count,
                                                otg_tract* __restrict__ out)
{
  constexpr uint32_t TPW = 64 / S;
  const uint32_t lane = threadIdx.x & 63u, jl = lane % S, seg_base = lane - jl;
  const uint32_t slot = (blockIdx.x * (UA_T / 64u) + (threadIdx.x >> 6)) * TPW + lane / S;
  const bool live = slot < count;
  uint32_t t = 0, L = 0, p = 1;                                   // a segment without a task walks no base
  const uint8_t* s = nullptr;
  const uint8_t* u = nullptr;
  if (live) {
    t = order[first + slot];
    const uint32_t a = in.seq(t), k = in.unit(t);
    L = in.rows.len[a]; s = in.rows.arena + in.rows.off[a];
    p = in.unit_len(k); u = in.unit_at(k);
  }
  const K km = tr_pen<K>(q.match), kx = tr_pen<K>(q.mismatch), kg = tr_pen<K>(q.indel);
  // position j = R jl + r of the unit: its base (ua_unit_key), its bias, its row cell, its best cell and the row that one was reached in
  uint32_t um[R], bend[R];
  bool valid[R];
  K bias[R], V[R], best[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t j = jl * R + r;
    valid[r] = j < p;
    um[r] = (live && valid[r]) ? ua_unit_key(u[j]) : 0xffu;
    bias[r] = valid[r] ? tr_bias<K>(j, kg) : (K)0;
    V[r] = (K)0; best[r] = (K)0; bend[r] = 0u;
  }
  // the rotate: position 0 takes position p - 1, every other lane's first position the last one of the lane below
  const uint32_t last_lane = seg_base + (p - 1u) / R, last_reg = (p - 1u) % R;
  const uint32_t below = jl ? lane - 1u : last_lane;
  const bool is_last = lane == last_lane;
  uint32_t um_prev[R];
  {
    const uint32_t send = is_last ? pick<uint32_t, R>(um, last_reg) : um[R - 1];
    um_prev[0] = from_lane(send, below);
#pragma unroll
    for (int r = 1; r < R; ++r) um_prev[r] = um[r - 1];
  }
  for (uint32_t i0 = 0; __any(i0 < L); i0 += 16u) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (i0 < L) __builtin_memcpy(w, s + i0, 16);                  // up to 15 bytes past the allele (the arenas extend past every row)
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] &= 0xdfdfdfdfu;              // ua_fold of the sixteen bases at once
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t sc = (w[k >> 2] >> (8 * (k & 3))) & 255u;     // the folded base of this row
      const uint32_t row = i0 + (uint32_t)k + 1u;                  // i + 1: the row being built, and the key of its fresh start
      const bool act = row <= L;
      const K send = (R > 1 && is_last) ? pick<K, R>(V, last_reg) : V[R - 1];
      const K d0 = from_lane(send, below);
      K T[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const K cell = tr_cell<K>(r ? V[r - 1] : d0, V[r], um_prev[r] == sc, km, kx, kg, (K)row) + bias[r];
        T[r] = valid[r] ? cell : (K)0;
      }
      // the prefix maximum of the biased cells: inside the lane, across the lanes of the segment, and back into the lane
#pragma unroll
      for (int r = 1; r < R; ++r) T[r] = ua_scan_take<K, true>(T[r], T[r - 1], true);
      K x = T[R - 1];
      x = scan_step<K, S, 1, true>(x, lane, jl);
      x = scan_step<K, S, 2, true>(x, lane, jl);
      x = scan_step<K, S, 4, true>(x, lane, jl);
      x = scan_step<K, S, 8, true>(x, lane, jl);
      x = scan_step<K, S, 16, true>(x, lane, jl);
      x = scan_step<K, S, 32, true>(x, lane, jl);
      if constexpr (R > 1) {
        const K ex = from_lane(x, lane - 1u);
#pragma unroll
        for (int r = 0; r < R - 1; ++r) T[r] = ua_scan_take<K, true>(T[r], ex, jl > 0u);
      }
      T[R - 1] = x;
      // the closed cell of position p - 1: its scanned cell less its own bias
      const K last = from_lane(pick<K, R>(T, last_reg), last_lane) - tr_bias<K>(p - 1u, kg);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const K h = tr_close<K>(T[r], last, bias[r], kg);
        const bool on = act && valid[r];
        V[r] = on ? h : V[r];
        const bool up = on && tr_improves<K>(h, best[r]);
        best[r] = up ? h : best[r];
        bend[r] = up ? row : bend[r];
      }
    }
  }
  // the best cell of the segment, in the order of step 4
  K bk = (K)0;
  uint32_t be = 0xffffffffu, bj = 0xffffffffu;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (valid[r] && tr_better<K>(best[r], bend[r], jl * R + r, bk, be, bj)) { bk = best[r]; be = bend[r]; bj = jl * R + r; }
#pragma unroll
  for (uint32_t d = 1; d < (uint32_t)S; d <<= 1) {
    const K ok = from_lane(bk, lane ^ d);
    const uint32_t oe = from_lane(be, lane ^ d), oj = from_lane(bj, lane ^ d);
    if (tr_better<K>(ok, oe, oj, bk, be, bj)) { bk = ok; be = oe; bj = oj; }
  }
  if (live && jl == 0u) {
    otg_tract rec;
    rec.score = tr_score<K>(bk);
    const bool none = rec.score == 0u || rec.score < q.min_score;
    rec.begin = none ? 0u : tr_begin<K>(bk); rec.end = none ? 0u : be;
    rec.edits = rec.unit_bases = rec.end_phase = rec.start_phase = 0u;        // tr_merge fills them in
    rec.flags = none ? OTG_TRACT_NONE : 0u;
    out[t] = rec;
  }
}

template <typename K, int C>
void tr_launch(otg_ctx* ctx, const UaIn& in, const otg_tract_params& q, const uint32_t* d_order, uint32_t first, uint32_t count, otg_tract* d_out)
{
  constexpr int S = ua_class_lanes(C), R = ua_class_regs(C);
  const uint32_t per_block = (UA_T / 64u) * (64u / S);
  hipLaunchKernelGGL((tr_align<K, S, R>), dim3((count + per_block - 1) / per_block), dim3(UA_T), 0, ctx->stream, in, q, d_order, first, count, d_out);
}
template <typename K>
void tr_launch_class(otg_ctx* ctx, uint32_t c, const UaIn& in, const otg_tract_params& q, const uint32_t* d_order, uint32_t first, uint32_t count, otg_tract* d_out)
{
  switch (c) {
    case 0: tr_launch<K, 0>(ctx, in, q, d_order, first, count, d_out); break;
    case 1: tr_launch<K, 1>(ctx, in, q, d_order, first, count, d_out); break;
    case 2: tr_launch<K, 2>(ctx, in, q, d_order, first, count, d_out); break;
    case 3: tr_launch<K, 3>(ctx, in, q, d_order, first, count, d_out); break;
    case 4: tr_launch<K, 4>(ctx, in, q, d_order, first, count, d_out); break;
    case 5: tr_launch<K, 5>(ctx, in, q, d_order, first, count, d_out); break;
    default: tr_launch<K, 6>(ctx, in, q, d_order, first, count, d_out); break;
  }
}

// ---- the second pass: the tracts as rows of the same arena, one per task
__global__ __launch_bounds__(UA_T) void tr_subrows(UaIn in, uint32_t n, const otg_tract* __restrict__ tracts, uint64_t* __restrict__ sub_off, uint32_t* __restrict__ sub_len)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t >= n) return;
  const otg_tract rec = tracts[t];
  const bool has = rec.flags == 0u;                               // begin < end <= the row's length
  sub_off[t] = in.rows.off[in.seq(t)] + (has ? rec.begin : 0u);
  sub_len[t] = has ? rec.end - rec.begin : 0u;
}

__global__ __launch_bounds__(UA_T) void tr_merge(UaIn in, uint32_t n, const otg_unitalign* __restrict__ aligned, otg_tract* __restrict__ tracts)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t >= n) return;
  if (tracts[t].flags != 0u) return;
  const otg_unitalign a = aligned[t];
  const uint32_t p = in.unit_len(in.unit(t));                     // 1 .. OTG_UNITALIGN_MAX_UNIT: the task has no flag
  tracts[t].edits = a.edits; tracts[t].unit_bases = a.unit_bases; tracts[t].end_phase = a.end_phase;
  tracts[t].start_phase = (a.end_phase + p - a.unit_bases % p) % p;
}

bool tr_force_wide() { static const bool on = ua_env("OTG_TRACT_WIDE"); return on; }
bool tr_force_seg64() { static const bool on = ua_env("OTG_TRACT_SEG64"); return on; }

} // namespace

int otg_tract_args(otg_ctx* ctx, const char* who, const otg_tract_params* params, otg_tract_params* out)
{
  if (params) *out = *params;
  else otg_tract_params_default(out);
  if (!tr_params_ok(*out))
    return otg_fail(ctx, OTG_ERR_ARG, "%s: scores (match %u, mismatch %u, indel %u, min_score %u) outside 1..16, 1..64, 1..64, 0..%u", who, out->match, out->mismatch,
                    out->indel, out->min_score, 1u << 24);
  return OTG_OK;
}

int otg_tract_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const OtgUnitSource& units, const uint32_t* d_task_seq,
                       const uint32_t* d_task_unit, uint32_t n, const otg_tract_params& q, otg_tract* out)
{
  ctx->last_tract_ms = ctx->last_tract_local_ms = 0.0; ctx->last_tract_n = 0;
  if (n == 0) return OTG_OK;
  if (n > (1u << 24)) return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: %u tasks in one call, at most %u", who, n, 1u << 24);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // start (u32, NBINS + 1) | hist (u32, NBINS) | cursor (u32, NBINS) | task_bin (u32, n)
  uint32_t* d_start = (uint32_t*)otg_slot(ctx, SLOT_TRACT_BINS, ((size_t)3 * UA_NBINS + 1 + n) * 4);
  uint32_t* d_order = (uint32_t*)otg_slot(ctx, SLOT_TRACT_ORDER, (size_t)n * 4);
  uint64_t* d_sub_off = (uint64_t*)otg_slot(ctx, SLOT_TRACT_SUB, (size_t)n * 12);      // sub_off (u64, n) | sub_len (u32, n)
  otg_tract* d_out = (otg_tract*)otg_slot(ctx, SLOT_TRACT_OUT, (size_t)n * sizeof(otg_tract));
  if (!d_start || !d_order || !d_sub_off || !d_out) return OTG_ERR_HIP;
  uint32_t* d_hist = d_start + UA_NBINS + 1;
  uint32_t* d_cursor = d_hist + UA_NBINS;
  uint32_t* d_bin = d_cursor + UA_NBINS;
  uint32_t* d_sub_len = (uint32_t*)(d_sub_off + n);
  const UaIn in{rows, units, d_task_seq, d_task_unit};
  const uint32_t grid = (n + UA_T - 1) / UA_T;
  HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t)2 * UA_NBINS * 4, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(tr_classify, dim3(grid), dim3(UA_T), 0, ctx->stream, in, n, q, tr_force_wide(), tr_force_seg64(), d_bin, d_hist, d_out);
  hipLaunchKernelGGL((otg_scan_kernel<uint32_t, uint32_t, OtgScanPtr<uint32_t>>), dim3(1), dim3(1024), 0, ctx->stream, OtgScanPtr<uint32_t>{d_hist}, UA_NBINS, d_start,
                     (uint32_t*)nullptr);
  hipLaunchKernelGGL(ua_scatter, dim3(grid), dim3(UA_T), 0, ctx->stream, n, d_bin, d_start, d_cursor, d_order);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<uint32_t> start(UA_NBINS + 1);
  HIP_TRY(ctx, hipMemcpyAsync(start.data(), d_start, start.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t tc = 0; tc < 2u * UA_CLASSES; ++tc) {
    const uint32_t first = start[tc * UA_BUCKETS], count = start[(tc + 1) * UA_BUCKETS] - first;
    if (count == 0) continue;
    if (tc < (uint32_t)UA_CLASSES) tr_launch_class<uint32_t>(ctx, tc, in, q, d_order, first, count, d_out);
    else tr_launch_class<uint64_t>(ctx, tc - UA_CLASSES, in, q, d_order, first, count, d_out);
  }
  hipLaunchKernelGGL(tr_subrows, dim3(grid), dim3(UA_T), 0, ctx->stream, in, n, d_out, d_sub_off, d_sub_len);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float local_ms = 0.f, merge_ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&local_ms, ctx->ev0, ctx->ev1));
  // the global unit alignment of the tracts: task t = sub-row t against the task's unit
  if (int rc = otg_unitalign_resident(ctx, who, OtgRows{rows.arena, d_sub_off, d_sub_len}, units, nullptr, d_task_unit, n, nullptr)) return rc;
  const double second_ms = ctx->last_unitalign_ms;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(tr_merge, dim3(grid), dim3(UA_T), 0, ctx->stream, in, n, (const otg_unitalign*)ctx->pool[SLOT_UNITALIGN_OUT].p, d_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  if (out) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)n * sizeof(otg_tract), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&merge_ms, ctx->ev0, ctx->ev1));
  ctx->last_tract_local_ms = local_ms; ctx->last_tract_ms = (double)local_ms + second_ms + (double)merge_ms; ctx->last_tract_n = n;
  return OTG_OK;
}

extern "C" void otg_tract_params_default(otg_tract_params* params)
{
  if (!params) return;
  params->match = 2u; params->mismatch = 7u; params->indel = 7u; params->min_score = 24u;
}

extern "C" int otg_tract_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len, uint32_t n_seqs,
                               const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units,
                               const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks, const otg_tract_params* params, otg_tract* out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_tract_batch: no context (no HIP device?)");
  otg_tract_params q;
  if (int rc = otg_tract_args(ctx, "otg_tract_batch", params, &q)) return rc;
  if (int rc = otg_rows_check(ctx, "otg_tract_batch", seq_arena, arena_bytes, seq_off, seq_len, n_seqs, nullptr)) return rc;
  if (int rc = otg_unitalign_check(ctx, "otg_tract_batch", n_seqs, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks)) return rc;
  ctx->last_tract_ms = ctx->last_tract_local_ms = 0.0; ctx->last_tract_n = 0;
  if (n_tasks == 0) return OTG_OK;
  OtgRows rows;
  if (int rc = otg_rows_upload(ctx, SLOT_TRACT_SEQ, SLOT_TRACT_META, seq_arena, arena_bytes, seq_off, seq_len, n_seqs, &rows)) return rc;
  OtgUnitSource units;
  const uint32_t *d_ts = nullptr, *d_tu = nullptr;
  if (int rc = otg_unitalign_upload(ctx, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks, &units, &d_ts, &d_tu, SLOT_TRACT_UNITS)) return rc;
  return otg_tract_resident(ctx, "otg_tract_batch", rows, units, d_ts, d_tu, n_tasks, q, out);
}

extern "C" int otg_tract_motifs(otg_ctx* ctx, const otg_tract_params* params, otg_tract* out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_tract_motifs: no context (no HIP device?)");
  otg_tract_params q;
  if (int rc = otg_tract_args(ctx, "otg_tract_motifs", params, &q)) return rc;
  const DevBuf& b = ctx->pool[SLOT_MOTIF_OUT];
  if (!b.p || ctx->last_motif_n == 0) return otg_fail(ctx, OTG_ERR_ARG, "otg_tract_motifs: no motif results on this context");
  // the alleles of that call must still lie where it read them: the context's own copy, or the rows of the cohort batch
  if (ctx->last_motif_rows.arena != (const uint8_t*)ctx->pool[SLOT_MOTIF_SEQ].p && !otg_cohort_holds_rows(ctx, ctx->last_motif_rows.arena))
    return otg_fail(ctx, OTG_ERR_ARG, "otg_tract_motifs: the alleles of the latest motif call are no longer on the device");
  const uint32_t n = ctx->last_motif_n;
  const OtgUnitSource units{(const uint8_t*)b.p + (size_t)n * sizeof(otg_motif), nullptr, nullptr, (const otg_motif*)b.p, ctx->last_motif_stride};
  return otg_tract_resident(ctx, "otg_tract_motifs", ctx->last_motif_rows, units, nullptr, nullptr, n, q, out);
}

extern "C" int otg_tract_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_tract** records)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_tract_device_results: NULL context");
  if (ctx->last_tract_n == 0) return otg_fail(ctx, OTG_ERR_ARG, "otg_tract_device_results: no tract results on this context");
  if (n_tasks) *n_tasks = ctx->last_tract_n;
  if (records) *records = (const otg_tract*)ctx->pool[SLOT_TRACT_OUT].p;
  return OTG_OK;
}

extern "C" int otg_tract_last_ms(otg_ctx* ctx, double* ms, double* local_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_tract_last_ms: NULL context");
  if (ms) *ms = ctx->last_tract_ms;
  if (local_ms) *local_ms = ctx->last_tract_local_ms;
  return OTG_OK;
}

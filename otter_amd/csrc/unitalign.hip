// unitalign.hip — an allele aligned to a cyclic repeat unit (otg_unitalign_batch / _motifs / _cohort): the edit count and the unit bases
// spanned, whatever indels lie in between.  The reference has no counterpart; include/otter_gpu.h states the rule.
//
// One task is a pair (allele, unit).  The row of the wraparound DP lives in registers, unit positions across lanes, and the kernel walks the
// bases of the allele.  A task takes a segment of S = 4 .. 64 lanes, the smallest power of two that holds its unit, so a wave carries 16 .. 1
// tasks; units of 65 .. 128 and 129 .. 256 bases take 2 and 4 positions per lane at S = 64.  Per row (otg_unitalign_core.hpp):
//   rotate   position j takes the cell of j - 1, position 0 that of p - 1: one lane exchange (otg_lane.hpp) with a source lane fixed per task;
//   cell     the diagonal step and the base outside the unit, a compare and a minimum;
//   closure  the skipped unit bases around the cycle: a prefix minimum of the biased cells, segmented (DPP row shifts inside 16 lanes,
//            lane exchanges above), and a broadcast of position p - 1 for the paths that wrap.
// The unit's bases are read once, one register per position (not LDS: no row needs another lane's base); the allele is read
// 16 bytes at a time, every lane of a segment the same 16.  A task that has consumed its allele keeps its row while its neighbours go on.
// The key is edits and unit_bases packed for one unsigned minimum: 32 bits up to OTG_UNITALIGN_NARROW_LEN, 64 bits above.
//
// Tasks are binned on the device (the motif chain's unit lengths exist only there): class = (tier, segment width), then length buckets in
// descending order, by a histogram, a scan and a scatter; every class is one launch over its stretch of the order.  Results land at the
// task's own index, so the order inside a bucket (atomics) does not show.
#include "otg_common.hpp"
#include "otg_lane.hpp"
#include "otg_scan.hpp"
#include "otg_unitalign_core.hpp"
#include "otg_unit_tasks.hpp"
#include <algorithm>
#include <cstdlib>

// cohort.hip: do the alleles of the open cohort batch still lie at d_arena (regrouped, clustered, rows built)?
bool otg_cohort_holds_rows(otg_ctx* ctx, const uint8_t* d_arena);

namespace {

using namespace otg_unitalign_core;
using namespace otg_lane;

// ---- binning (the scatter is otg_unit_tasks.hpp's)
__global__ __launch_bounds__(UA_T) void ua_classify(UaIn in, uint32_t n, bool wide, bool seg64, uint32_t* __restrict__ task_bin, uint32_t* __restrict__ hist,
                                                   otg_unitalign* __restrict__ out)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t >= n) return;
  const uint32_t L = in.rows.len[in.seq(t)], p = in.unit_len(in.unit(t));
  const uint32_t refusal = ua_refusal(L, p);
  if (refusal || L == 0u) {                                       // nothing to align: the record is final
    otg_unitalign rec;
    rec.edits = rec.unit_bases = rec.end_phase = 0u; rec.flags = refusal;
    out[t] = rec;
    task_bin[t] = UA_NO_BIN;
    return;
  }
  const uint32_t tier = (wide || L > OTG_UNITALIGN_NARROW_LEN) ? 1u : 0u;
  const uint32_t bin = (tier * UA_CLASSES + ua_class(p, seg64)) * UA_BUCKETS + (UA_BUCKETS - 1u - ua_bucket(L));      // the longest first
  task_bin[t] = bin;
  atomicAdd(&hist[bin], 1u);
}

// ---- the alignment: tasks order[first .. first + count), 64 / S to a wave
template <typename K, int S, int R>
__global__ __launch_bounds__(UA_T) void ua_align(UaIn in, const uint32_t* __restrict__ order, uint32_t first, uint32_t count, otg_unitalign* __restrict__ out)
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
  // position j = R jl + r of the unit: its base (ua_unit_key), its bias, its row cell
  uint32_t um[R];
  bool valid[R];
  K bias[R], V[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t j = jl * R + r;
    valid[r] = j < p;
    um[r] = (live && valid[r]) ? ua_unit_key(u[j]) : 0xffu;
    bias[r] = valid[r] ? ua_bias<K>(j, p) : (K)0;
    V[r] = (K)0;
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
    for (int q = 0; q < 4; ++q) w[q] &= 0xdfdfdfdfu;              // ua_fold of the sixteen bases at once
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t sc = (w[k >> 2] >> (8 * (k & 3))) & 255u;     // the folded base of this row
      const bool act = i0 + (uint32_t)k < L;
      const K send = (R > 1 && is_last) ? pick<K, R>(V, last_reg) : V[R - 1];
      const K d0 = from_lane(send, below);
      K T[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const K cell = ua_cell<K>(r ? V[r - 1] : d0, V[r], um_prev[r] == sc) + bias[r];
        T[r] = valid[r] ? cell : ua_inf<K>();
      }
      // the prefix minimum of the biased cells: inside the lane, across the lanes of the segment, and back into the lane
#pragma unroll
      for (int r = 1; r < R; ++r) T[r] = ua_scan_take<K>(T[r], T[r - 1], true);
      K x = T[R - 1];
      x = scan_step<K, S, 1>(x, lane, jl);
      x = scan_step<K, S, 2>(x, lane, jl);
      x = scan_step<K, S, 4>(x, lane, jl);
      x = scan_step<K, S, 8>(x, lane, jl);
      x = scan_step<K, S, 16>(x, lane, jl);
      x = scan_step<K, S, 32>(x, lane, jl);
      if constexpr (R > 1) {
        const K ex = from_lane(x, lane - 1u);
#pragma unroll
        for (int r = 0; r < R - 1; ++r) T[r] = ua_scan_take<K>(T[r], ex, jl > 0u);
      }
      T[R - 1] = x;
      const K last = from_lane(pick<K, R>(T, last_reg), last_lane);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const K h = ua_close<K>(T[r], last, jl * R + r, p);
        V[r] = (act && valid[r]) ? h : V[r];
      }
    }
  }
  // the smallest key, ties to the smallest position
  K best = ua_inf<K>();
  uint32_t bj = 0xffffffffu;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (valid[r] && ua_better<K>(V[r], jl * R + r, best, bj)) { best = V[r]; bj = jl * R + r; }
#pragma unroll
  for (uint32_t d = 1; d < (uint32_t)S; d <<= 1) {
    const K ob = from_lane(best, lane ^ d);
    const uint32_t oj = from_lane(bj, lane ^ d);
    if (ua_better<K>(ob, oj, best, bj)) { best = ob; bj = oj; }
  }
  if (live && jl == 0u) {
    otg_unitalign rec;
    rec.edits = ua_edits<K>(best); rec.unit_bases = ua_unit_bases<K>(best); rec.end_phase = bj; rec.flags = 0u;
    out[t] = rec;
  }
}

template <typename K, int C>
void ua_launch(otg_ctx* ctx, const UaIn& in, const uint32_t* d_order, uint32_t first, uint32_t count, otg_unitalign* d_out)
{
  constexpr int S = ua_class_lanes(C), R = ua_class_regs(C);
  const uint32_t per_block = (UA_T / 64u) * (64u / S);
  hipLaunchKernelGGL((ua_align<K, S, R>), dim3((count + per_block - 1) / per_block), dim3(UA_T), 0, ctx->stream, in, d_order, first, count, d_out);
}
template <typename K>
void ua_launch_class(otg_ctx* ctx, uint32_t c, const UaIn& in, const uint32_t* d_order, uint32_t first, uint32_t count, otg_unitalign* d_out)
{
  switch (c) {
    case 0: ua_launch<K, 0>(ctx, in, d_order, first, count, d_out); break;
    case 1: ua_launch<K, 1>(ctx, in, d_order, first, count, d_out); break;
    case 2: ua_launch<K, 2>(ctx, in, d_order, first, count, d_out); break;
    case 3: ua_launch<K, 3>(ctx, in, d_order, first, count, d_out); break;
    case 4: ua_launch<K, 4>(ctx, in, d_order, first, count, d_out); break;
    case 5: ua_launch<K, 5>(ctx, in, d_order, first, count, d_out); break;
    default: ua_launch<K, 6>(ctx, in, d_order, first, count, d_out); break;
  }
}

bool ua_force_wide() { static const bool on = ua_env("OTG_UNITALIGN_WIDE"); return on; }
bool ua_force_seg64() { static const bool on = ua_env("OTG_UNITALIGN_SEG64"); return on; }

} // namespace

int otg_unitalign_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const OtgUnitSource& units, const uint32_t* d_task_seq,
                           const uint32_t* d_task_unit, uint32_t n, otg_unitalign* out)
{
  ctx->last_unitalign_ms = 0.0; ctx->last_unitalign_n = 0;
  if (n == 0) return OTG_OK;
  if (n > (1u << 24)) return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: %u tasks in one call, at most %u", who, n, 1u << 24);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // start (u32, NBINS + 1) | hist (u32, NBINS) | cursor (u32, NBINS) | task_bin (u32, n)
  uint32_t* d_start = (uint32_t*)otg_slot(ctx, SLOT_UNITALIGN_BINS, ((size_t)3 * UA_NBINS + 1 + n) * 4);
  uint32_t* d_order = (uint32_t*)otg_slot(ctx, SLOT_UNITALIGN_ORDER, (size_t)n * 4);
  otg_unitalign* d_out = (otg_unitalign*)otg_slot(ctx, SLOT_UNITALIGN_OUT, (size_t)n * sizeof(otg_unitalign));
  if (!d_start || !d_order || !d_out) return OTG_ERR_HIP;
  uint32_t* d_hist = d_start + UA_NBINS + 1;
  uint32_t* d_cursor = d_hist + UA_NBINS;
  uint32_t* d_bin = d_cursor + UA_NBINS;
  const UaIn in{rows, units, d_task_seq, d_task_unit};
  const uint32_t grid = (n + UA_T - 1) / UA_T;
  HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t)2 * UA_NBINS * 4, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(ua_classify, dim3(grid), dim3(UA_T), 0, ctx->stream, in, n, ua_force_wide(), ua_force_seg64(), d_bin, d_hist, d_out);
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
    if (tc < (uint32_t)UA_CLASSES) ua_launch_class<uint32_t>(ctx, tc, in, d_order, first, count, d_out);
    else ua_launch_class<uint64_t>(ctx, tc - UA_CLASSES, in, d_order, first, count, d_out);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  if (out) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)n * sizeof(otg_unitalign), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  ctx->last_unitalign_ms = ms; ctx->last_unitalign_n = n;
  return OTG_OK;
}

int otg_unitalign_check(otg_ctx* ctx, const char* who, uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                        const uint32_t* unit_len, uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks)
{
  return otg_unit_lists_check(
      ctx, who, n_tasks && (!task_seq || !task_unit), unit_arena, unit_bytes, unit_off, unit_len, n_units, n_tasks,
      [&](uint32_t k, uint32_t len) {
        return len > OTG_UNITALIGN_MAX_UNIT ? otg_fail(ctx, OTG_ERR_ARG, "%s: unit %u has %u bytes, at most %d", who, k, len, OTG_UNITALIGN_MAX_UNIT) : (int)OTG_OK;
      },
      [&] {
        for (uint32_t t = 0; t < n_tasks; ++t)
          if (task_seq[t] >= n_seqs || task_unit[t] >= n_units)
            return otg_fail(ctx, OTG_ERR_ARG, "%s: task %u names allele %u of %u and unit %u of %u", who, t, task_seq[t], n_seqs, task_unit[t], n_units);
        return (int)OTG_OK;
      });
}

int otg_unitalign_upload(otg_ctx* ctx, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units,
                         const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks, OtgUnitSource* units, const uint32_t** d_task_seq,
                         const uint32_t** d_task_unit, int slot)
{
  // unit_off (u64, n_units) | unit_len (u32, n_units) | task_seq, task_unit (u32, n_tasks) | the unit bytes
  const size_t meta = (size_t)n_units * 12 + (size_t)n_tasks * 8;
  uint8_t* d = (uint8_t*)otg_slot(ctx, slot, meta + unit_bytes + 16);
  if (!d) return OTG_ERR_HIP;
  uint64_t* d_uoff = (uint64_t*)d;
  uint32_t* d_ulen = (uint32_t*)(d + (size_t)n_units * 8);
  uint32_t* d_ts = d_ulen + n_units;
  uint32_t* d_tu = d_ts + n_tasks;
  uint8_t* d_ub = d + meta;
  if (n_units) {
    HIP_TRY(ctx, hipMemcpyAsync(d_uoff, unit_off, (size_t)n_units * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_ulen, unit_len, (size_t)n_units * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  if (n_tasks) {
    HIP_TRY(ctx, hipMemcpyAsync(d_ts, task_seq, (size_t)n_tasks * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_tu, task_unit, (size_t)n_tasks * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  if (unit_bytes) HIP_TRY(ctx, hipMemcpyAsync(d_ub, unit_arena, unit_bytes, hipMemcpyHostToDevice, ctx->stream));
  *units = OtgUnitSource{d_ub, d_uoff, d_ulen, nullptr, 0u};
  *d_task_seq = d_ts; *d_task_unit = d_tu;
  return OTG_OK;
}

extern "C" int otg_unitalign_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                                   uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                                   uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks, otg_unitalign* out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_unitalign_batch: no context (no HIP device?)");
  if (int rc = otg_rows_check(ctx, "otg_unitalign_batch", seq_arena, arena_bytes, seq_off, seq_len, n_seqs, nullptr)) return rc;
  if (int rc = otg_unitalign_check(ctx, "otg_unitalign_batch", n_seqs, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks)) return rc;
  ctx->last_unitalign_ms = 0.0; ctx->last_unitalign_n = 0;
  if (n_tasks == 0) return OTG_OK;
  OtgRows rows;
  if (int rc = otg_rows_upload(ctx, SLOT_UNITALIGN_SEQ, SLOT_UNITALIGN_META, seq_arena, arena_bytes, seq_off, seq_len, n_seqs, &rows)) return rc;
  OtgUnitSource units;
  const uint32_t *d_ts = nullptr, *d_tu = nullptr;
  if (int rc = otg_unitalign_upload(ctx, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks, &units, &d_ts, &d_tu)) return rc;
  return otg_unitalign_resident(ctx, "otg_unitalign_batch", rows, units, d_ts, d_tu, n_tasks, out);
}

extern "C" int otg_unitalign_motifs(otg_ctx* ctx, otg_unitalign* out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_unitalign_motifs: no context (no HIP device?)");
  const DevBuf& b = ctx->pool[SLOT_MOTIF_OUT];
  if (!b.p || ctx->last_motif_n == 0) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitalign_motifs: no motif results on this context");
  // the alleles of that call must still lie where it read them: the context's own copy, or the rows of the cohort batch
  if (ctx->last_motif_rows.arena != (const uint8_t*)ctx->pool[SLOT_MOTIF_SEQ].p && !otg_cohort_holds_rows(ctx, ctx->last_motif_rows.arena))
    return otg_fail(ctx, OTG_ERR_ARG, "otg_unitalign_motifs: the alleles of the latest motif call are no longer on the device");
  const uint32_t n = ctx->last_motif_n;
  const OtgUnitSource units{(const uint8_t*)b.p + (size_t)n * sizeof(otg_motif), nullptr, nullptr, (const otg_motif*)b.p, ctx->last_motif_stride};
  return otg_unitalign_resident(ctx, "otg_unitalign_motifs", ctx->last_motif_rows, units, nullptr, nullptr, n, out);
}

extern "C" int otg_unitalign_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_unitalign** records)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitalign_device_results: NULL context");
  if (ctx->last_unitalign_n == 0) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitalign_device_results: no unit alignment results on this context");
  if (n_tasks) *n_tasks = ctx->last_unitalign_n;
  if (records) *records = (const otg_unitalign*)ctx->pool[SLOT_UNITALIGN_OUT].p;
  return OTG_OK;
}

extern "C" int otg_unitalign_last_ms(otg_ctx* ctx, double* ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitalign_last_ms: NULL context");
  if (ms) *ms = ctx->last_unitalign_ms;
  return OTG_OK;
}

// locus.hip — the locus mode (otg_locus_batch / _cohort): where the repeat of a unit set lies inside a flanked allele, and the joint parse of
// exactly that stretch.  The reference has no counterpart; include/otter_gpu.h states the rule.
//
// First pass, lc_align: the local wraparound alignment over a unit set.  The lanes are up_forward's (unitparse.hip): the cycles of all units
// of the set side by side in registers, every unit starting at a lane boundary, 4 .. 64 lanes per task at 1, 2 or 4 positions per lane,
// sixteen allele bytes per load; a task that has consumed its allele keeps its state while its neighbours go on.  The arithmetic is
// tr_align's (tract.hip): the key score * 2^SHIFT + begin ordered by one unsigned maximum, the cell step, the biased prefix maximum inside
// each unit, the running best per position.  Between them the join of otg_locus_core.hpp: per unit its last position, one maximum of the
// phase-0 candidates over the task's lanes, the entry and the way on.  No traceback store: the second pass has its own.
// The tasks are ordered on the host as the joint parse orders them (the unit sets come from there, and of the alleles only the lengths are
// needed): by tier and class, the longest first.
// Second pass: lc_subrows writes the tracts as rows (off + begin, end - begin; length 0 without a tract) over the SAME arena, indexed by
// task; otg_unitparse_resident parses them with identity task lists against the call's sets (its sixteen-byte loads stay inside the parent
// row's arena); lc_merge joins both results into otg_locus records at the task's own index and shifts the segments by the tract's begin.
#include "otg_common.hpp"
#include "otg_lane.hpp"
#include "otg_locus_core.hpp"
#include "otg_unit_tasks.hpp"
#include <algorithm>
#include <numeric>

namespace {

using namespace otg_locus_core;
using namespace otg_lane;

constexpr uint32_t LC_NONE = 0xffffffffu;

using LcIn = OtgSetTasks;

// every record before the alignment: a task that is not aligned keeps it
__global__ __launch_bounds__(UA_T) void lc_init(LcIn in, uint32_t n, otg_locus* __restrict__ out)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t >= n) return;
  otg_locus rec;
  rec.score = rec.begin = rec.end = rec.edits = rec.switches = rec.unit_bases = rec.n_segments = 0u;
  rec.flags = in.rows.len[in.task_seq[t]] > OTG_LOCUS_MAX_LEN ? OTG_LOCUS_TOO_LONG : OTG_LOCUS_NONE;
  out[t] = rec;
}

// ---- the local alignment: tasks order[first .. first + count), 64 / S to a wave
template <typename K, int S, int R>
__global__ __launch_bounds__(UA_T) void lc_align(LcIn in, otg_tract_params q, const uint32_t* __restrict__ order, uint32_t first, uint32_t count,
                                                otg_locus* __restrict__ out)
{
  constexpr uint32_t TPW = 64 / S;
  const uint32_t lane = threadIdx.x & 63u, jl = lane % S, seg_base = lane - jl;
  const uint32_t slot = (blockIdx.x * (UA_T / 64u) + (threadIdx.x >> 6)) * TPW + lane / S;
  const bool live = slot < count;
  uint32_t t = 0, L = 0, NU = 0;                                  // a segment without a task walks no base
  uint64_t uf = 0;
  const uint8_t* s = nullptr;
  if (live) {
    t = order[first + slot];
    const uint32_t a = in.task_seq[t], sq = in.task_set[t];
    L = in.rows.len[a]; s = in.rows.arena + in.rows.off[a];
    uf = in.set_first[sq]; NU = (uint32_t)(in.set_first[sq + 1] - uf);
  }
  // the lane's unit: k, its length p, the lane's place ul inside it and the unit's first lane
  uint32_t k = LC_NONE, ul = 0, p = 1, ufirst = lane;
  const uint8_t* u = nullptr;
  for (uint32_t c = 0, acc = 0; c < NU; ++c) {
    const uint32_t pc = in.unit_len[uf + c], nl = (pc + R - 1u) / R;
    if (jl >= acc && jl - acc < nl) { k = c; ul = jl - acc; p = pc; ufirst = seg_base + acc; u = in.units + in.unit_off[uf + c]; }
    acc += nl;
  }
  const K km = tr_pen<K>(q.match), kx = tr_pen<K>(q.mismatch), kg = tr_pen<K>(q.indel);
  // position j = R ul + r of the unit: its base, its bias (also the way on from phase 0), its row cell, its best cell and that one's row
  uint32_t um[R], bend[R];
  bool valid[R];
  K bias[R], V[R], best[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t j = ul * R + r;
    valid[r] = k != LC_NONE && j < p;
    um[r] = valid[r] ? ua_unit_key(u[j]) : 0xffu;
    bias[r] = valid[r] ? tr_bias<K>(j, kg) : (K)0;
    V[r] = (K)0; best[r] = (K)0; bend[r] = 0u;
  }
  // the rotate: position 0 takes position p - 1, every other lane's first position the last one of the lane below
  const uint32_t last_lane = ufirst + (p - 1u) / R, last_reg = (p - 1u) % R;
  const uint32_t below = ul ? lane - 1u : last_lane;
  const bool is_last = lane == last_lane, is_first = ul == 0u && valid[0];
  const K last_bias = tr_bias<K>(p - 1u, kg);
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
    for (int kk = 0; kk < 16; ++kk) {
      const uint32_t sc = (w[kk >> 2] >> (8 * (kk & 3))) & 255u;   // the folded base of this row
      const uint32_t row = i0 + (uint32_t)kk + 1u;                 // i + 1: the row being built, and the key of its fresh start
      const bool act = row <= L;
      const K send = (R > 1 && is_last) ? pick<K, R>(V, last_reg) : V[R - 1];
      const K d0 = from_lane(send, below);
      K T[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const K cell = tr_cell<K>(r ? V[r - 1] : d0, V[r], um_prev[r] == sc, km, kx, kg, (K)row) + bias[r];
        T[r] = valid[r] ? cell : (K)0;
      }
      const K h0 = T[0];                                           // H1[0] at a unit's first lane: bias 0, nothing below it
      // the prefix maximum of the biased cells: inside the lane, across the lanes of the unit, and back into the lane
#pragma unroll
      for (int r = 1; r < R; ++r) T[r] = ua_scan_take<K, true>(T[r], T[r - 1], true);
      K x = T[R - 1];
      x = scan_step<K, S, 1, true>(x, lane, ul);
      x = scan_step<K, S, 2, true>(x, lane, ul);
      x = scan_step<K, S, 4, true>(x, lane, ul);
      x = scan_step<K, S, 8, true>(x, lane, ul);
      x = scan_step<K, S, 16, true>(x, lane, ul);
      x = scan_step<K, S, 32, true>(x, lane, ul);
      if constexpr (R > 1) {
        const K ex = from_lane(x, lane - 1u);
#pragma unroll
        for (int r = 0; r < R - 1; ++r) T[r] = ua_scan_take<K, true>(T[r], ex, ul > 0u);
      }
      T[R - 1] = x;
      // the closed cell of the unit's position p - 1: its scanned cell less its own bias
      const K last = from_lane(pick<K, R>(T, last_reg), last_lane) - last_bias;
      // phase 0: the unit's candidate at its first lane, the largest of the task, and what enters every unit from behind
      K best0 = is_first ? lc_cand0<K>(h0, last, kg) : (K)0;
#pragma unroll
      for (uint32_t d = 1; d < (uint32_t)S; d <<= 1) best0 = tr_max<K>(best0, from_lane(best0, lane ^ d));
      const K entry = lc_entry<K>(last, best0, kg);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const K h = lc_close<K>(T[r], bias[r], entry);
        const bool on = act && valid[r];
        V[r] = on ? h : V[r];
        const bool up = on && tr_improves<K>(h, best[r]);
        best[r] = up ? h : best[r];
        bend[r] = up ? row : bend[r];
      }
    }
  }
  // the best cell of the task, in the order of step 4: the lanes lie in (unit, position) order
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
    otg_locus rec;
    rec.score = tr_score<K>(bk);
    const bool none = rec.score == 0u || rec.score < q.min_score;
    rec.begin = none ? 0u : tr_begin<K>(bk); rec.end = none ? 0u : be;
    rec.edits = rec.switches = rec.unit_bases = rec.n_segments = 0u;      // lc_merge fills them in
    rec.flags = none ? OTG_LOCUS_NONE : 0u;
    out[t] = rec;
  }
}

template <typename K, int C>
void lc_launch(otg_ctx* ctx, const LcIn& in, const otg_tract_params& q, const uint32_t* d_order, uint32_t first, uint32_t count, otg_locus* d_out)
{
  constexpr int S = ua_class_lanes(C), R = ua_class_regs(C);
  const uint32_t per_block = (UA_T / 64u) * (64u / S);
  hipLaunchKernelGGL((lc_align<K, S, R>), dim3((count + per_block - 1) / per_block), dim3(UA_T), 0, ctx->stream, in, q, d_order, first, count, d_out);
}
template <typename K>
void lc_launch_class(otg_ctx* ctx, uint32_t c, const LcIn& in, const otg_tract_params& q, const uint32_t* d_order, uint32_t first, uint32_t count, otg_locus* d_out)
{
  switch (c) {
    case 0: lc_launch<K, 0>(ctx, in, q, d_order, first, count, d_out); break;
    case 1: lc_launch<K, 1>(ctx, in, q, d_order, first, count, d_out); break;
    case 2: lc_launch<K, 2>(ctx, in, q, d_order, first, count, d_out); break;
    case 3: lc_launch<K, 3>(ctx, in, q, d_order, first, count, d_out); break;
    case 4: lc_launch<K, 4>(ctx, in, q, d_order, first, count, d_out); break;
    case 5: lc_launch<K, 5>(ctx, in, q, d_order, first, count, d_out); break;
    default: lc_launch<K, 6>(ctx, in, q, d_order, first, count, d_out); break;
  }
}

// ---- the second pass: the tracts as rows of the same arena, one per task
__global__ __launch_bounds__(UA_T) void lc_subrows(LcIn in, uint32_t n, const otg_locus* __restrict__ loci, uint64_t* __restrict__ sub_off, uint32_t* __restrict__ sub_len)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t >= n) return;
  const otg_locus rec = loci[t];
  const bool has = rec.flags == 0u;                               // begin < end <= the row's length
  sub_off[t] = in.rows.off[in.task_seq[t]] + (has ? rec.begin : 0u);
  sub_len[t] = has ? rec.end - rec.begin : 0u;
}

// the parse of the sub-rows into the records; the segments of a task with a tract move to allele positions; the offsets behind the records
__global__ __launch_bounds__(UA_T) void lc_merge(uint32_t n, const otg_unitparse_sum* __restrict__ sums, const uint64_t* __restrict__ seg_off,
                                                otg_unitparse_seg* __restrict__ segs, otg_locus* __restrict__ loci, uint64_t* __restrict__ off_out)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t > n) return;
  off_out[t] = seg_off[t];
  if (t == n || loci[t].flags != 0u) return;                      // (a task without a tract had an empty sub-row: no segments)
  const otg_unitparse_sum a = sums[t];
  const uint32_t begin = loci[t].begin;
  loci[t].edits = a.edits; loci[t].switches = a.switches; loci[t].unit_bases = a.unit_bases; loci[t].n_segments = a.n_segments;
  for (uint64_t g = seg_off[t]; g < seg_off[t + 1]; ++g) { segs[g].begin += begin; segs[g].end += begin; }
}

bool lc_force_wide() { static const bool on = ua_env("OTG_LOCUS_WIDE"); return on; }
bool lc_force_seg64() { static const bool on = ua_env("OTG_LOCUS_SEG64"); return on; }

} // namespace

int otg_locus_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const uint32_t* h_len, uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes,
                       const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                       const uint32_t* task_set, uint32_t n, const otg_tract_params& q, otg_locus* out, uint64_t* seg_off, uint64_t* n_segments)
{
  ctx->last_locus = OtgSegLast{};
  ctx->last_locus_tiers[0] = ctx->last_locus_tiers[1] = 0u;
  if (n_segments) *n_segments = 0;
  if (n == 0) {
    if (seg_off) seg_off[0] = 0;
    return OTG_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> lens;
  if (!h_len) {                                                    // the rows of a cohort: only their lengths come to the host
    lens.resize(n_seqs);
    HIP_TRY(ctx, hipMemcpyAsync(lens.data(), rows.len, (size_t)n_seqs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h_len = lens.data();
  }
  // ---- the plan: the tasks by (tier, class), the longest first
  const bool wide = lc_force_wide(), seg64 = lc_force_seg64();
  std::vector<uint32_t> set_class(n_sets), set_narrow(n_sets);
  for (uint32_t s = 0; s < n_sets; ++s) {
    const uint32_t K = (uint32_t)(set_first[s + 1] - set_first[s]);
    set_class[s] = lc_class(unit_len + set_first[s], K, seg64);
    set_narrow[s] = lc_narrow_len(q, unit_len + set_first[s], K);
  }
  std::vector<uint32_t> by_bin[2 * UP_CLASSES];
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t L = h_len[task_seq[t]], s = task_set[t];
    if (L == 0u || L > OTG_LOCUS_MAX_LEN) continue;
    by_bin[((wide || L > set_narrow[s]) ? UP_CLASSES : 0) + set_class[s]].push_back(t);
  }
  std::vector<uint32_t> order, bin_first(2 * UP_CLASSES + 1, 0u);
  for (uint32_t b = 0; b < 2u * UP_CLASSES; ++b) {
    std::vector<uint32_t>& v = by_bin[b];
    std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t c) {
      const uint32_t la = h_len[task_seq[a]], lb = h_len[task_seq[c]];
      return la != lb ? la > lb : a < c;
    });
    order.insert(order.end(), v.begin(), v.end());
    bin_first[b + 1] = (uint32_t)order.size();
  }
  // ---- the device copies
  LcIn in;
  if (int rc = otg_unit_sets_upload(ctx, SLOT_LOCUS_UNITS, rows, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set, n, &in)) return rc;
  uint64_t* d_sub_off = (uint64_t*)otg_slot(ctx, SLOT_LOCUS_SUB, (size_t)n * 16);      // sub_off (u64, n) | sub_len (u32, n) | order (u32, n)
  // OUT: the records | the segment offsets (u64, n + 1)
  uint8_t* d_res = (uint8_t*)otg_slot(ctx, SLOT_LOCUS_OUT, (size_t)n * sizeof(otg_locus) + ((size_t)n + 1) * 8);
  if (!d_sub_off || !d_res) return OTG_ERR_HIP;
  uint32_t* d_sub_len = (uint32_t*)(d_sub_off + n);
  uint32_t* d_order = d_sub_len + n;
  otg_locus* d_out = (otg_locus*)d_res;
  uint64_t* d_off_out = (uint64_t*)(d_res + (size_t)n * sizeof(otg_locus));
  if (!order.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  const uint32_t grid = (n + UA_T - 1) / UA_T;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(lc_init, dim3(grid), dim3(UA_T), 0, ctx->stream, in, n, d_out);
  for (uint32_t b = 0; b < 2u * UP_CLASSES; ++b) {
    const uint32_t first = bin_first[b], count = bin_first[b + 1] - first;
    if (count == 0) continue;
    if (b < (uint32_t)UP_CLASSES) lc_launch_class<uint32_t>(ctx, b, in, q, d_order, first, count, d_out);
    else lc_launch_class<uint64_t>(ctx, b - UP_CLASSES, in, q, d_order, first, count, d_out);
  }
  hipLaunchKernelGGL(lc_subrows, dim3(grid), dim3(UA_T), 0, ctx->stream, in, n, d_out, d_sub_off, d_sub_len);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float local_ms = 0.f, merge_ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&local_ms, ctx->ev0, ctx->ev1));
  // the joint parse of the tracts: task t = sub-row t against the task's set
  std::vector<uint32_t> identity(n);
  std::iota(identity.begin(), identity.end(), 0u);
  uint64_t total = 0;
  if (int rc = otg_unitparse_resident(ctx, who, OtgRows{rows.arena, d_sub_off, d_sub_len}, nullptr, n, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets,
                                      identity.data(), task_set, n, nullptr, seg_off, &total))
    return rc;
  const double second_ms = ctx->last_unitparse.ms[0] + ctx->last_unitparse.ms[1];
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  const uint8_t* up_res = (const uint8_t*)ctx->pool[SLOT_UNITPARSE_RES].p;
  hipLaunchKernelGGL(lc_merge, dim3((n + 1 + UA_T - 1) / UA_T), dim3(UA_T), 0, ctx->stream, n, (const otg_unitparse_sum*)up_res,
                     (const uint64_t*)(up_res + (size_t)n * sizeof(otg_unitparse_sum)), (otg_unitparse_seg*)ctx->pool[SLOT_UNITPARSE_SEGS].p, d_out, d_off_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  if (out) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)n * sizeof(otg_locus), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&merge_ms, ctx->ev0, ctx->ev1));
  if (n_segments) *n_segments = total;
  ctx->last_locus_tiers[0] = bin_first[UP_CLASSES]; ctx->last_locus_tiers[1] = (uint32_t)order.size() - bin_first[UP_CLASSES];
  ctx->last_locus = OtgSegLast{n, total, true, {(double)local_ms + second_ms + (double)merge_ms, (double)local_ms}};
  return OTG_OK;
}

extern "C" int otg_locus_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len, uint32_t n_seqs,
                               const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units,
                               const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set, uint32_t n_tasks,
                               const otg_tract_params* params, otg_locus* out, uint64_t* seg_off, uint64_t* n_segments)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_locus_batch: no context (no HIP device?)");
  otg_tract_params q;
  if (int rc = otg_tract_args(ctx, "otg_locus_batch", params, &q)) return rc;
  if (int rc = otg_rows_check(ctx, "otg_locus_batch", seq_arena, arena_bytes, seq_off, seq_len, n_seqs, nullptr)) return rc;
  if (int rc = otg_unitparse_check(ctx, "otg_locus_batch", n_seqs, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set, n_tasks))
    return rc;
  ctx->last_locus.valid = false;
  OtgRows rows = {nullptr, nullptr, nullptr};
  if (n_tasks != 0)                                                // (without tasks the launch part answers before it reads a row)
    if (int rc = otg_rows_upload(ctx, SLOT_LOCUS_SEQ, SLOT_LOCUS_META, seq_arena, arena_bytes, seq_off, seq_len, n_seqs, &rows)) return rc;
  return otg_locus_resident(ctx, "otg_locus_batch", rows, seq_len, n_seqs, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set,
                            n_tasks, q, out, seg_off, n_segments);
}

extern "C" int otg_locus_collect(otg_ctx* ctx, otg_unitparse_seg* segs, uint64_t capacity)
{
  return otg_seg_collect(ctx, "otg_locus_collect", "locus", &otg_ctx::last_locus, SLOT_UNITPARSE_SEGS, sizeof(otg_unitparse_seg), segs, capacity);
}

extern "C" int otg_locus_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_locus** records, const uint64_t** seg_off, const otg_unitparse_seg** segs,
                                        uint64_t* total)
{
  return otg_seg_device_results(ctx, "otg_locus_device_results", "locus", &otg_ctx::last_locus, SLOT_LOCUS_OUT, SLOT_UNITPARSE_SEGS, sizeof(otg_locus), n_tasks,
                                (const void**)records, seg_off, (const void**)segs, total);
}

extern "C" int otg_locus_last_ms(otg_ctx* ctx, double* ms, double* local_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_locus_last_ms: NULL context");
  if (ms) *ms = ctx->last_locus.ms[0];
  if (local_ms) *local_ms = ctx->last_locus.ms[1];
  return OTG_OK;
}

extern "C" int otg_locus_last_tiers(otg_ctx* ctx, uint32_t* narrow, uint32_t* wide)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_locus_last_tiers: NULL context");
  if (narrow) *narrow = ctx->last_locus_tiers[0];
  if (wide) *wide = ctx->last_locus_tiers[1];
  return OTG_OK;
}

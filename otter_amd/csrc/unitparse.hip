// unitparse.hip — an allele parsed against a set of repeat units (otg_unitparse_batch / _cohort): edits, switches and unit bases of the
// joint alignment, and its segments by a traceback.  The reference has no counterpart; include/otter_gpu.h states the rule.
//
// The forward pass is the unit alignment's (unitalign.hip): the row of the wraparound DP in registers, positions across lanes, the kernel
// walking the bases of the allele.  Here the row holds the cycles of all units of the set side by side, every unit starting at a lane
// boundary, so "position inside its unit" is a per-lane constant and the scan guards and the rotate's source lane are fixed per task.  A
// task takes the smallest power of two of 4 .. 64 lanes that holds its set, at 1, 2 or 4 positions per lane.  Per row
// (otg_unitparse_core.hpp):
//   rotate   inside each unit, one lane exchange (otg_lane.hpp);
//   cell     the diagonal step and the base outside the unit, kept apart: the traceback wants to know which one won;
//   scan     the biased prefix minimum, segmented by unit (DPP row shifts where the task lies inside 16 lanes, lane exchanges above);
//   phase 0  per unit the candidate from inside it, one minimum of those over the task's lanes, plus one switch where that is smaller;
//   close    the way on from phase 0 around every unit.
// It stores decisions, not keys: two bits per cell (diagonal, outside base, skip, switch) and per row the units that hold the smallest
// phase-0 candidate, as wave ballots: 2 R + 1 words of 64 bits per row and wave, written by as many lanes in one store.  The backward pass
// walks one task per lane from its end cell over those words and writes the segments from the last to the first; the forward pass has
// already counted them (switches + 1), so the order is count, scan, write.  The walk is a chain of dependent loads, so only every
// UP_WALK_SPREAD-th lane of a wave takes a task: more waves for the same tasks, and a load of one hides behind the others'.
//
// The tasks are ordered on the host (the unit sets come from there, and of the alleles only the lengths are needed): by class, then the
// longest first, so the tasks of a wave end close to each other and a wave's store is as long as its first task.  A call is cut into
// chunks of waves whose store fits the budget (OTG_UNITPARSE_TRACE_MB); with more than one chunk the forward pass first runs without the
// store to count the segments, then once more chunk by chunk with the walk behind it.
#include "otg_common.hpp"
#include "otg_lane.hpp"
#include "otg_scan.hpp"
#include "otg_unitparse_core.hpp"
#include <algorithm>
#include <cstdlib>

namespace {

using namespace otg_unitparse_core;
using namespace otg_lane;

constexpr uint32_t UP_T = 256;                                   // threads of a forward workgroup
constexpr uint32_t UP_WALK_T = 64;                               // threads of a walk workgroup: the walk is latency-bound, so the waves are spread
constexpr uint32_t UP_WALK_SPREAD = 8;                           // and only every eighth lane walks a task: eight times the waves to hide a load behind
constexpr uint32_t UP_NONE = 0xffffffffu;
constexpr size_t UP_TRACE_MB = 1024;                             // the default budget of the traceback store

using UpIn = OtgSetTasks;

__global__ __launch_bounds__(UP_T) void up_init(UpIn in, uint32_t n, otg_unitparse_sum* __restrict__ sums)
{
  const uint32_t t = blockIdx.x * UP_T + threadIdx.x;
  if (t >= n) return;
  otg_unitparse_sum rec;
  rec.edits = rec.switches = rec.unit_bases = rec.n_segments = rec.end_unit = rec.end_phase = rec.reserved = 0u;
  rec.flags = in.rows.len[in.task_seq[t]] > OTG_UNITPARSE_MAX_LEN ? OTG_UNITPARSE_TOO_LONG : 0u;
  sums[t] = rec;
}

// ---- the forward pass: tasks order[first .. first + count), 64 / S to a wave; wave w of the launch is wave wave0 + w of the plan
template <int S, int R, bool TR>
__global__ __launch_bounds__(UP_T) void up_forward(UpIn in, const uint32_t* __restrict__ order, uint32_t first, uint32_t count, uint32_t wave0,
                                                  const uint64_t* __restrict__ wave_off, const uint32_t* __restrict__ wave_rows,
                                                  uint64_t* __restrict__ trace, otg_unitparse_sum* __restrict__ sums)
{
  constexpr uint32_t TPW = 64 / S, WORDS = up_words(R);
  const uint32_t lane = threadIdx.x & 63u, jl = lane % S, seg_base = lane - jl;
  const uint32_t wave = blockIdx.x * (UP_T / 64u) + (threadIdx.x >> 6);
  const uint32_t slot = wave * TPW + lane / S;
  const bool live = slot < count;
  uint32_t t = 0, L = 0, K = 0;                                   // a segment without a task walks no base
  uint64_t uf = 0;
  const uint8_t* s = nullptr;
  if (live) {
    t = order[first + slot];
    const uint32_t a = in.task_seq[t], q = in.task_set[t];
    L = in.rows.len[a]; s = in.rows.arena + in.rows.off[a];
    uf = in.set_first[q]; K = (uint32_t)(in.set_first[q + 1] - uf);
  }
  // the lane's unit: k, its length p, the lane's place ul inside it and the unit's first lane
  uint32_t k = UP_NONE, ul = 0, p = 1, ufirst = lane;
  const uint8_t* u = nullptr;
  for (uint32_t q = 0, acc = 0; q < K; ++q) {
    const uint32_t pq = in.unit_len[uf + q], nl = (pq + R - 1u) / R;
    if (jl >= acc && jl - acc < nl) { k = q; ul = jl - acc; p = pq; ufirst = seg_base + acc; u = in.units + in.unit_off[uf + q]; }
    acc += nl;
  }
  // position j = R ul + r of the unit: its base, its bias, the way on from phase 0, its row cell
  uint32_t um[R];
  bool valid[R];
  uint64_t bias[R], onward[R], V[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t j = ul * R + r;
    valid[r] = k != UP_NONE && j < p;
    um[r] = valid[r] ? ua_unit_key(u[j]) : 0xffu;
    bias[r] = valid[r] ? up_bias(j, p) : 0u;
    onward[r] = up_onward(j);
    V[r] = 0u;
  }
  // the rotate: position 0 takes position p - 1, every other lane's first position the last one of the lane below
  const uint32_t last_lane = ufirst + (p - 1u) / R, last_reg = (p - 1u) % R;
  const uint32_t below = ul ? lane - 1u : last_lane;
  const bool is_last = lane == last_lane, is_first = ul == 0u && valid[0];
  uint32_t um_prev[R];
  {
    const uint32_t send = is_last ? pick<uint32_t, R>(um, last_reg) : um[R - 1];
    um_prev[0] = from_lane(send, below);
#pragma unroll
    for (int r = 1; r < R; ++r) um_prev[r] = um[r - 1];
  }
  // the wave's stretch of the store (wave-uniform)
  uint32_t rows_w = 0;
  uint64_t* tr = nullptr;
  if constexpr (TR) {
    if (wave * TPW < count) { rows_w = wave_rows[wave0 + wave]; tr = trace + wave_off[wave0 + wave]; }
  }
  for (uint32_t i0 = 0; __any(i0 < L); i0 += 16u) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (i0 < L) __builtin_memcpy(w, s + i0, 16);                  // up to 15 bytes past the allele (the arenas extend past every row)
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] &= 0xdfdfdfdfu;              // ua_fold of the sixteen bases at once
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const uint32_t sc = (w[kk >> 2] >> (8 * (kk & 3))) & 255u;   // the folded base of this row
      const bool act = i0 + (uint32_t)kk < L;
      const uint64_t send = (R > 1 && is_last) ? pick<uint64_t, R>(V, last_reg) : V[R - 1];
      const uint64_t d0 = from_lane(send, below);
      uint64_t d[R], v[R], T[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        d[r] = up_diag(r ? V[r - 1] : d0, um_prev[r] == sc);
        v[r] = up_vert(V[r]);
        T[r] = valid[r] ? up_min(d[r], v[r]) + bias[r] : up_inf();
      }
      const uint64_t cell0 = up_min(d[0], v[0]);
      // the prefix minimum of the biased cells: inside the lane, across the lanes of the unit, and back into the lane
#pragma unroll
      for (int r = 1; r < R; ++r) T[r] = ua_scan_take<uint64_t>(T[r], T[r - 1], true);
      uint64_t x = T[R - 1];
      x = scan_step<uint64_t, S, 1>(x, lane, ul);
      x = scan_step<uint64_t, S, 2>(x, lane, ul);
      x = scan_step<uint64_t, S, 4>(x, lane, ul);
      x = scan_step<uint64_t, S, 8>(x, lane, ul);
      x = scan_step<uint64_t, S, 16>(x, lane, ul);
      x = scan_step<uint64_t, S, 32>(x, lane, ul);
      if constexpr (R > 1) {
        const uint64_t ex = from_lane(x, lane - 1u);
#pragma unroll
        for (int r = 0; r < R - 1; ++r) T[r] = ua_scan_take<uint64_t>(T[r], ex, ul > 0u);
      }
      T[R - 1] = x;
      const uint64_t last = from_lane(pick<uint64_t, R>(T, last_reg), last_lane);
      // phase 0: the unit's candidate at its first lane, the smallest of the task, and what enters every unit from behind
      const uint64_t cand = is_first ? up_phase0(cell0, last) : up_inf();
      uint64_t best0 = cand;
#pragma unroll
      for (uint32_t dd = 1; dd < (uint32_t)S; dd <<= 1) best0 = up_min(best0, from_lane(best0, lane ^ dd));
      const uint64_t entry = up_entry(last, best0);
      uint32_t code[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t h = up_close(T[r], bias[r], entry, onward[r]);
        code[r] = up_code(h, d[r], v[r], ul * R + r, last);
        V[r] = (act && valid[r]) ? h : V[r];
      }
      if constexpr (TR) {
        uint64_t mine = __ballot(is_first && cand == best0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint64_t b0 = __ballot((code[r] & 1u) != 0u), b1 = __ballot((code[r] & 2u) != 0u);
          mine = lane == 2u * r ? b0 : lane == 2u * r + 1u ? b1 : mine;
        }
        const uint32_t row = i0 + (uint32_t)kk;
        if (row < rows_w && lane < WORDS) tr[(uint64_t)row * WORDS + lane] = mine;      // rows_w rows of WORDS words were planned for this wave
      }
    }
  }
  // the smallest key, ties to the smallest (unit, position): the lanes lie in that order
  uint64_t best = up_inf();
  uint32_t bg = UP_NONE;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (valid[r] && (V[r] < best || (V[r] == best && lane * R + r < bg))) { best = V[r]; bg = lane * R + r; }
#pragma unroll
  for (uint32_t dd = 1; dd < (uint32_t)S; dd <<= 1) {
    const uint64_t ob = from_lane(best, lane ^ dd);
    const uint32_t og = from_lane(bg, lane ^ dd);
    if (ob < best || (ob == best && og < bg)) { best = ob; bg = og; }
  }
  if (live && bg != UP_NONE && bg / R == lane) {
    otg_unitparse_sum rec;
    rec.edits = up_edits(best); rec.switches = up_switches(best); rec.unit_bases = up_unit_bases(best);
    rec.n_segments = rec.switches + 1u; rec.end_unit = k; rec.end_phase = ul * R + bg % R; rec.flags = 0u; rec.reserved = 0u;
    sums[t] = rec;
  }
}

// ---- the backward pass: one task per lane
struct UpSegCount {
  const otg_unitparse_sum* sums;
  __device__ __forceinline__ uint64_t operator()(uint32_t i) const { return sums[i].n_segments; }
};

__global__ __launch_bounds__(UP_WALK_T) void up_walk_kernel(UpIn in, const uint32_t* __restrict__ order, uint32_t first, uint32_t count, uint32_t wave0,
                                                           const uint64_t* __restrict__ wave_off, uint32_t S, uint32_t R, const uint64_t* __restrict__ trace,
                                                           const otg_unitparse_sum* __restrict__ sums, const uint64_t* __restrict__ seg_off,
                                                           otg_unitparse_seg* __restrict__ segs, uint32_t* __restrict__ defect)
{
  const uint32_t thread = blockIdx.x * UP_WALK_T + threadIdx.x, slot = thread / UP_WALK_SPREAD;
  if (thread % UP_WALK_SPREAD != 0u || slot >= count) return;
  const uint32_t tpw = 64u / S, wave = slot / tpw, lane0 = (slot % tpw) * S;
  const uint32_t t = order[first + slot], a = in.task_seq[t], q = in.task_set[t];
  const uint64_t uf = in.set_first[q];
  const otg_unitparse_sum rec = sums[t];
  const uint64_t so = seg_off[t];
  const uint32_t room = (uint32_t)(seg_off[t + 1] - so);
  const uint32_t bad = room != rec.n_segments ? 7u
                                              : up_walk(trace + wave_off[wave0 + wave], R, lane0, S, in.rows.arena + in.rows.off[a], in.rows.len[a], in.units, in.unit_off + uf,
                                                        in.unit_len + uf, (uint32_t)(in.set_first[q + 1] - uf), rec.end_unit, rec.end_phase, segs + so, room);
  if (bad) atomicMax(defect, bad);
}

template <int C, bool TR>
void up_launch(otg_ctx* ctx, const UpIn& in, const uint32_t* d_order, uint32_t first, uint32_t count, uint32_t wave0, const uint64_t* d_wave_off,
               const uint32_t* d_wave_rows, uint64_t* d_trace, otg_unitparse_sum* d_sums)
{
  constexpr int S = ua_class_lanes(C), R = ua_class_regs(C);
  const uint32_t per_block = (UP_T / 64u) * (64u / S);
  hipLaunchKernelGGL((up_forward<S, R, TR>), dim3((count + per_block - 1) / per_block), dim3(UP_T), 0, ctx->stream, in, d_order, first, count, wave0, d_wave_off,
                     d_wave_rows, d_trace, d_sums);
}
template <bool TR>
void up_launch_class(otg_ctx* ctx, uint32_t c, const UpIn& in, const uint32_t* d_order, uint32_t first, uint32_t count, uint32_t wave0,
                     const uint64_t* d_wave_off, const uint32_t* d_wave_rows, uint64_t* d_trace, otg_unitparse_sum* d_sums)
{
  switch (c) {
    case 0: up_launch<0, TR>(ctx, in, d_order, first, count, wave0, d_wave_off, d_wave_rows, d_trace, d_sums); break;
    case 1: up_launch<1, TR>(ctx, in, d_order, first, count, wave0, d_wave_off, d_wave_rows, d_trace, d_sums); break;
    case 2: up_launch<2, TR>(ctx, in, d_order, first, count, wave0, d_wave_off, d_wave_rows, d_trace, d_sums); break;
    case 3: up_launch<3, TR>(ctx, in, d_order, first, count, wave0, d_wave_off, d_wave_rows, d_trace, d_sums); break;
    case 4: up_launch<4, TR>(ctx, in, d_order, first, count, wave0, d_wave_off, d_wave_rows, d_trace, d_sums); break;
    case 5: up_launch<5, TR>(ctx, in, d_order, first, count, wave0, d_wave_off, d_wave_rows, d_trace, d_sums); break;
    default: up_launch<6, TR>(ctx, in, d_order, first, count, wave0, d_wave_off, d_wave_rows, d_trace, d_sums); break;
  }
}

// the budget of the traceback store in bytes: OTG_UNITPARSE_TRACE_MB, read once
size_t up_budget()
{
  static const size_t bytes = [] {
    const char* e = getenv("OTG_UNITPARSE_TRACE_MB");
    const long long mb = e && *e ? atoll(e) : 0;
    return (size_t)(mb > 0 ? (size_t)mb : UP_TRACE_MB) << 20;
  }();
  return bytes;
}

// a stretch of whole waves of one class: slots [first, first + count) of the order, the first of them wave wave0 of the plan
struct UpPiece { uint32_t cls, first, count, wave0; };
struct UpChunk { std::vector<UpPiece> pieces; uint64_t words = 0; };

} // namespace

int otg_unitparse_check(otg_ctx* ctx, const char* who, uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                        const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                        const uint32_t* task_set, uint32_t n_tasks)
{
  return otg_unit_lists_check(
      ctx, who, !set_first || (n_tasks && (!task_seq || !task_set)), unit_arena, unit_bytes, unit_off, unit_len, n_units, n_tasks,
      [&](uint32_t k, uint32_t len) {
        return len == 0u || len > OTG_UNITALIGN_MAX_UNIT
                   ? otg_fail(ctx, OTG_ERR_ARG, "%s: unit %u has %u bytes, 1 to %d are allowed", who, k, len, OTG_UNITALIGN_MAX_UNIT)
                   : (int)OTG_OK;
      },
      [&] {
        for (uint32_t q = 0; q < n_sets; ++q) {
          if (set_first[q] > set_first[q + 1] || set_first[q + 1] > n_units)
            return otg_fail(ctx, OTG_ERR_ARG, "%s: set %u spans units %llu .. %llu of %u", who, q, (unsigned long long)set_first[q], (unsigned long long)set_first[q + 1],
                            n_units);
          const uint64_t K = set_first[q + 1] - set_first[q];
          if (K == 0) return otg_fail(ctx, OTG_ERR_ARG, "%s: set %u is empty", who, q);
          if (K > OTG_UNITPARSE_MAX_UNITS) return otg_fail(ctx, OTG_ERR_ARG, "%s: set %u has %llu units, at most %d", who, q, (unsigned long long)K, OTG_UNITPARSE_MAX_UNITS);
          if (otg_unitparse_core::up_class(unit_len + set_first[q], (uint32_t)K) == otg_unitparse_core::UP_NO_CLASS)
            return otg_fail(ctx, OTG_ERR_ARG, "%s: set %u does not fit one wave (its units take %u lanes at four positions each, at most %d)", who, q,
                            otg_unitparse_core::up_lanes(unit_len + set_first[q], (uint32_t)K, 4u), OTG_UNITPARSE_MAX_LANES);
        }
        for (uint32_t t = 0; t < n_tasks; ++t)
          if (task_seq[t] >= n_seqs || task_set[t] >= n_sets)
            return otg_fail(ctx, OTG_ERR_ARG, "%s: task %u names allele %u of %u and set %u of %u", who, t, task_seq[t], n_seqs, task_set[t], n_sets);
        return (int)OTG_OK;
      });
}

int otg_unit_sets_upload(otg_ctx* ctx, int slot, const OtgRows& rows, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                         uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set, uint32_t n, OtgSetTasks* out)
{
  // unit_off (u64) | set_first (u64) | unit_len, task_seq, task_set (u32) | the unit bytes
  const size_t meta = (size_t)n_units * 12 + (size_t)(n_sets + 1) * 8 + (size_t)n * 8;
  uint8_t* d_u = (uint8_t*)otg_slot(ctx, slot, meta + unit_bytes + 16);
  if (!d_u) return OTG_ERR_HIP;
  uint64_t* d_uoff = (uint64_t*)d_u;
  uint64_t* d_sf = d_uoff + n_units;
  uint32_t* d_ulen = (uint32_t*)(d_sf + n_sets + 1);
  uint32_t* d_ts = d_ulen + n_units;
  uint32_t* d_tq = d_ts + n;
  uint8_t* d_ub = d_u + meta;
  HIP_TRY(ctx, hipMemcpyAsync(d_uoff, unit_off, (size_t)n_units * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_sf, set_first, (size_t)(n_sets + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_ulen, unit_len, (size_t)n_units * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_ts, task_seq, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_tq, task_set, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  if (unit_bytes) HIP_TRY(ctx, hipMemcpyAsync(d_ub, unit_arena, unit_bytes, hipMemcpyHostToDevice, ctx->stream));
  *out = OtgSetTasks{rows, d_ub, d_uoff, d_ulen, d_sf, d_ts, d_tq};
  return OTG_OK;
}

int otg_unitparse_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const uint32_t* h_len, uint32_t n_seqs, const uint8_t* unit_arena,
                           uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set, uint32_t n,
                           otg_unitparse_sum* sums, uint64_t* seg_off, uint64_t* n_segments)
{
  ctx->last_unitparse = OtgSegLast{};
  ctx->last_locus.valid = false;                                   // (its segments lie in this operator's slot)
  if (n_segments) *n_segments = 0;
  if (n == 0) {
    if (seg_off) seg_off[0] = 0;
    return OTG_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->ev2) HIP_TRY(ctx, hipEventCreate(&ctx->ev2));
  std::vector<uint32_t> lens;
  if (!h_len) {                                                    // the rows of a cohort: only their lengths come to the host
    lens.resize(n_seqs);
    HIP_TRY(ctx, hipMemcpyAsync(lens.data(), rows.len, (size_t)n_seqs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h_len = lens.data();
  }
  // ---- the plan: the tasks by class, the longest first; the waves, their rows, the chunks
  std::vector<uint32_t> set_class(n_sets);
  for (uint32_t q = 0; q < n_sets; ++q) set_class[q] = up_class(unit_len + set_first[q], (uint32_t)(set_first[q + 1] - set_first[q]));
  std::vector<uint32_t> by_class[UP_CLASSES];
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t L = h_len[task_seq[t]];
    if (L != 0u && L <= OTG_UNITPARSE_MAX_LEN) by_class[set_class[task_set[t]]].push_back(t);
  }
  std::vector<uint32_t> order, wave_rows;
  std::vector<uint64_t> wave_off;
  std::vector<UpChunk> chunks;
  std::vector<UpPiece> classes;                                    // every class as one piece: the counting pass
  const uint64_t budget_words = up_budget() / 8;
  for (uint32_t c = 0; c < (uint32_t)UP_CLASSES; ++c) {
    std::vector<uint32_t>& v = by_class[c];
    if (v.empty()) continue;
    std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) {
      const uint32_t la = h_len[task_seq[a]], lb = h_len[task_seq[b]];
      return la != lb ? la > lb : a < b;
    });
    const uint32_t tpw = 64u / (uint32_t)ua_class_lanes((int)c), words = up_words((uint32_t)ua_class_regs((int)c));
    const uint32_t cfirst = (uint32_t)order.size();
    classes.push_back(UpPiece{c, cfirst, (uint32_t)v.size(), (uint32_t)wave_rows.size()});
    for (size_t w = 0; w * tpw < v.size(); ++w) {
      const uint32_t rows = h_len[task_seq[v[w * tpw]]];            // the longest task of the wave
      const uint64_t need = (uint64_t)rows * words;
      const uint32_t cnt = (uint32_t)std::min<size_t>(tpw, v.size() - w * tpw), slot0 = cfirst + (uint32_t)(w * tpw), wv = (uint32_t)wave_rows.size();
      if (chunks.empty() || (chunks.back().words && chunks.back().words + need > budget_words)) chunks.emplace_back();
      UpChunk& ch = chunks.back();
      if (!ch.pieces.empty() && ch.pieces.back().cls == c) ch.pieces.back().count += cnt;
      else ch.pieces.push_back(UpPiece{c, slot0, cnt, wv});
      wave_rows.push_back(rows);
      wave_off.push_back(ch.words);
      ch.words += need;
    }
    order.insert(order.end(), v.begin(), v.end());
  }
  uint64_t trace_words = 0;
  for (const UpChunk& ch : chunks) trace_words = std::max(trace_words, ch.words);
  // ---- the device copies
  const size_t n_waves = wave_rows.size();
  UpIn in;
  if (int rc = otg_unit_sets_upload(ctx, SLOT_UNITPARSE_UNITS, rows, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set, n, &in)) return rc;
  // PLAN: wave_off (u64) | order, wave_rows, defect (u32)
  uint8_t* d_p = (uint8_t*)otg_slot(ctx, SLOT_UNITPARSE_PLAN, n_waves * 12 + order.size() * 4 + 16);
  uint8_t* d_res = (uint8_t*)otg_slot(ctx, SLOT_UNITPARSE_RES, (size_t)n * sizeof(otg_unitparse_sum) + ((size_t)n + 1) * 8);
  uint64_t* d_trace = (uint64_t*)otg_slot(ctx, SLOT_UNITPARSE_TRACE, (size_t)trace_words * 8 + 16);
  if (!d_p || !d_res || !d_trace) return OTG_ERR_HIP;
  uint64_t* d_woff = (uint64_t*)d_p;
  uint32_t* d_order = (uint32_t*)(d_woff + n_waves);
  uint32_t* d_wrows = d_order + order.size();
  uint32_t* d_defect = d_wrows + n_waves;
  otg_unitparse_sum* d_sums = (otg_unitparse_sum*)d_res;
  uint64_t* d_segoff = (uint64_t*)(d_res + (size_t)n * sizeof(otg_unitparse_sum));
  if (n_waves) {
    HIP_TRY(ctx, hipMemcpyAsync(d_woff, wave_off.data(), n_waves * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_wrows, wave_rows.data(), n_waves * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(ctx, hipMemsetAsync(d_defect, 0, 4, ctx->stream));
  const bool one = chunks.size() <= 1;
  double forward_ms = 0.0, trace_ms = 0.0;
  float ms = 0.f;
  // ---- the forward pass that counts the segments (with a single chunk it fills the store as well)
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(up_init, dim3((n + UP_T - 1) / UP_T), dim3(UP_T), 0, ctx->stream, in, n, d_sums);
  for (const UpPiece& pc : classes) {
    if (one) up_launch_class<true>(ctx, pc.cls, in, d_order, pc.first, pc.count, pc.wave0, d_woff, d_wrows, d_trace, d_sums);
    else up_launch_class<false>(ctx, pc.cls, in, d_order, pc.first, pc.count, pc.wave0, d_woff, d_wrows, d_trace, d_sums);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, UpSegCount>), dim3(1), dim3(1024), 0, ctx->stream, UpSegCount{d_sums}, n, d_segoff, (uint64_t*)nullptr);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t total = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&total, d_segoff + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  otg_unitparse_seg* d_segs = (otg_unitparse_seg*)otg_slot(ctx, SLOT_UNITPARSE_SEGS, (size_t)total * sizeof(otg_unitparse_seg) + 16);
  if (!d_segs) return OTG_ERR_HIP;
  // ---- the walk, chunk by chunk
  auto walk = [&](const UpChunk& ch) {
    for (const UpPiece& pc : ch.pieces)
      hipLaunchKernelGGL(up_walk_kernel, dim3((uint32_t)(((uint64_t)pc.count * UP_WALK_SPREAD + UP_WALK_T - 1) / UP_WALK_T)), dim3(UP_WALK_T), 0, ctx->stream, in, d_order, pc.first, pc.count, pc.wave0,
                         d_woff, (uint32_t)ua_class_lanes((int)pc.cls), (uint32_t)ua_class_regs((int)pc.cls), d_trace, d_sums, d_segoff, d_segs, d_defect);
  };
  if (one) {
    if (!chunks.empty()) walk(chunks[0]);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    forward_ms = ms;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2));
    trace_ms = ms;
  } else {
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    forward_ms = ms;
    for (const UpChunk& ch : chunks) {
      HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
      for (const UpPiece& pc : ch.pieces) up_launch_class<true>(ctx, pc.cls, in, d_order, pc.first, pc.count, pc.wave0, d_woff, d_wrows, d_trace, d_sums);
      HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
      walk(ch);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      forward_ms += ms;
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2));
      trace_ms += ms;
    }
  }
  uint32_t defect = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&defect, d_defect, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (sums) HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, (size_t)n * sizeof(otg_unitparse_sum), hipMemcpyDeviceToHost, ctx->stream));
  if (seg_off) HIP_TRY(ctx, hipMemcpyAsync(seg_off, d_segoff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (defect) return otg_fail(ctx, OTG_ERR_FATAL, "%s: the traceback store contradicts the forward pass (code %u)", who, defect);
  if (n_segments) *n_segments = total;
  ctx->last_unitparse = OtgSegLast{n, total, true, {forward_ms, trace_ms}};
  return OTG_OK;
}

extern "C" int otg_unitparse_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                                   uint32_t n_seqs, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len,
                                   uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq, const uint32_t* task_set,
                                   uint32_t n_tasks, otg_unitparse_sum* sums, uint64_t* seg_off, uint64_t* n_segments)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_unitparse_batch: no context (no HIP device?)");
  if (int rc = otg_rows_check(ctx, "otg_unitparse_batch", seq_arena, arena_bytes, seq_off, seq_len, n_seqs, nullptr)) return rc;
  if (int rc = otg_unitparse_check(ctx, "otg_unitparse_batch", n_seqs, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set,
                                   n_tasks))
    return rc;
  ctx->last_unitparse.valid = false;
  OtgRows rows = {nullptr, nullptr, nullptr};
  if (n_tasks != 0)                                                // (without tasks the launch part answers before it reads a row)
    if (int rc = otg_rows_upload(ctx, SLOT_UNITPARSE_SEQ, SLOT_UNITPARSE_META, seq_arena, arena_bytes, seq_off, seq_len, n_seqs, &rows)) return rc;
  return otg_unitparse_resident(ctx, "otg_unitparse_batch", rows, seq_len, n_seqs, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq,
                                task_set, n_tasks, sums, seg_off, n_segments);
}

extern "C" int otg_unitparse_collect(otg_ctx* ctx, otg_unitparse_seg* segs, uint64_t capacity)
{
  return otg_seg_collect(ctx, "otg_unitparse_collect", "unit parse", &otg_ctx::last_unitparse, SLOT_UNITPARSE_SEGS, sizeof(otg_unitparse_seg), segs, capacity);
}

extern "C" int otg_unitparse_device_results(otg_ctx* ctx, uint32_t* n_tasks, const otg_unitparse_sum** sums, const uint64_t** seg_off,
                                            const otg_unitparse_seg** segs, uint64_t* total)
{
  return otg_seg_device_results(ctx, "otg_unitparse_device_results", "unit parse", &otg_ctx::last_unitparse, SLOT_UNITPARSE_RES, SLOT_UNITPARSE_SEGS,
                                sizeof(otg_unitparse_sum), n_tasks, (const void**)sums, seg_off, (const void**)segs, total);
}

extern "C" int otg_unitparse_last_ms(otg_ctx* ctx, double* forward_ms, double* trace_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitparse_last_ms: NULL context");
  if (forward_ms) *forward_ms = ctx->last_unitparse.ms[0];
  if (trace_ms) *trace_ms = ctx->last_unitparse.ms[1];
  return OTG_OK;
}

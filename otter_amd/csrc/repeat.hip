// repeat.hip — the repeat structure of alleles (otg_repeat_batch / otg_repeat_cohort): every allele as a left-to-right sequence of exact
// tandem repeats and literals, (CAG)20(CCG)20.  The reference has no counterpart; include/otter_gpu.h states the rule.
//
// The planes, their two tiers and the shifted compare are those of motif.hip (otg_motif_core.hpp); the per-word walk, the candidate order
// and the unit compare are otg_repeat_core.hpp.  Two phases:
//   runs    lanes own periods and sweep the words of the match bits e_p, carrying the open run across words.  A counting pass gives the kept
//           runs per (allele, period); a workgroup scan per allele and a scan over the alleles turn the counts into offsets; a second pass
//           (only the periods that keep a run) writes (p, a, e) at those positions, in (p, a) order within an allele.  No atomics.
//   select  one workgroup per allele runs the parse: every best() is a strided scan of the allele's runs and a tree under rp_better (a total
//           order), the unit compare of a placement runs over t across lanes.  The horizon stack (at most one entry per run) and the
//           segments (at most 2 K + 1 for K runs) lie in workspace sized from the run counts; the segments are then compacted to CSR by a
//           scan of the actual counts.
#include "otg_common.hpp"
#include "otg_scan.hpp"
#include "otg_repeat_core.hpp"
#include <algorithm>

static_assert(OTG_REPEAT_MAX_LEN == OTG_MOTIF_MAX_LEN && OTG_REPEAT_MAX_PERIOD == OTG_MOTIF_MAX_PERIOD, "the plane tiers of motif.hip are shared");

namespace {

using namespace otg_repeat_core;
constexpr uint32_t REPEAT_LDS_WORDS = OTG_MOTIF_LDS_LEN / 32 + 2;

struct RpPeriods {
  const uint32_t* len; uint32_t max_period;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return rp_period_range(len[i], max_period); }
};
struct RpSegCap {                                                // the segments K runs can give
  const uint32_t* k;
  __device__ __forceinline__ uint64_t operator()(uint32_t i) const { return 2ull * k[i] + 1ull; }
};
struct RpSegCount {
  const otg_repeat_sum* sums;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return sums[i].n_segments; }
};

// One period of one allele in either pass: count the kept runs (WRITE = false) or write them where the scans put them (only a period that keeps one).
template <bool WRITE>
__device__ __forceinline__ void repeat_period(const uint32_t* LO, const uint32_t* HI, const uint32_t* V, uint32_t L, uint32_t p, uint32_t min_copies,
                                              uint32_t min_span, uint32_t* cnt, const uint32_t* pre, RpRun* runs)
{
  const uint32_t min_len = rp_min_len(p, min_copies, min_span);
  if (!WRITE) cnt[p - 1u] = L >= min_len ? rp_runs(LO, HI, V, L, p, min_len, nullptr) : 0u;
  else if (cnt[p - 1u]) rp_runs(LO, HI, V, L, p, min_len, runs + pre[p - 1u]);
}

// ---- LDS tier: pack and sweep, one workgroup per allele (the write pass skips an allele without a kept run)
template <bool WRITE>
__global__ __launch_bounds__(REPEAT_T) void repeat_runs_lds(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                           const uint32_t* __restrict__ seq_len, uint32_t n, uint32_t max_period, uint32_t lds_len,
                                                           uint32_t min_copies, uint32_t min_span, const uint64_t* __restrict__ m_off,
                                                           uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pre,
                                                           const uint64_t* __restrict__ run_off, RpRun* __restrict__ runs)
{
  __shared__ uint32_t LO[REPEAT_LDS_WORDS], HI[REPEAT_LDS_WORDS], V[REPEAT_LDS_WORDS];
  const uint32_t tid = threadIdx.x;
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint32_t L = seq_len[a], P = rp_period_range(L, max_period);
    if (P == 0u || L > lds_len) continue;                       // (block-uniform)
    if (WRITE && run_off[a + 1] == run_off[a]) continue;
    const uint8_t* s = arena + seq_off[a];
    const uint32_t W = (L + 31u) >> 5;
    for (uint32_t w = tid; w < W + 2u; w += REPEAT_T) {
      uint32_t l = 0, h = 0, v = 0;
      if (w < W) mo_pack_word(s, L, w, &l, &h, &v);
      LO[w] = l; HI[w] = h; V[w] = v;
    }
    __syncthreads();
    for (uint32_t p = 1u + tid; p <= P; p += REPEAT_T)
      repeat_period<WRITE>(LO, HI, V, L, p, min_copies, min_span, cnt + m_off[a], WRITE ? pre + m_off[a] : nullptr, WRITE ? runs + run_off[a] : nullptr);
    __syncthreads();
  }
}

// ---- HBM tier: the planes of motif.hip's pack kernel, one workgroup per allele and 256 periods
template <bool WRITE>
__global__ __launch_bounds__(REPEAT_T) void repeat_runs_hbm(const uint32_t* __restrict__ seq_len, uint32_t n, uint32_t max_period, uint32_t min_copies,
                                                           uint32_t min_span, const uint64_t* __restrict__ pl_off, const uint32_t* __restrict__ planes,
                                                           const uint64_t* __restrict__ m_off, uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pre,
                                                           const uint64_t* __restrict__ run_off, RpRun* __restrict__ runs)
{
  const uint32_t a = blockIdx.x;
  if (a >= n || pl_off[a + 1] == pl_off[a]) return;
  if (WRITE && run_off[a + 1] == run_off[a]) return;
  const uint32_t L = seq_len[a], P = rp_period_range(L, max_period), PW = ((L + 31u) >> 5) + 2u;
  const uint32_t p = 1u + blockIdx.y * REPEAT_T + threadIdx.x;
  if (p > P) return;
  const uint32_t* LO = planes + 3u * pl_off[a];
  const uint32_t* HI = LO + PW;
  const uint32_t* V = HI + PW;
  repeat_period<WRITE>(LO, HI, V, L, p, min_copies, min_span, cnt + m_off[a], WRITE ? pre + m_off[a] : nullptr, WRITE ? runs + run_off[a] : nullptr);
}

// ---- per allele the exclusive scan of its period counts (pre) and their sum K, one workgroup per allele
__global__ __launch_bounds__(REPEAT_T) void repeat_scan_periods(const uint32_t* __restrict__ seq_len, uint32_t n, uint32_t max_period,
                                                               const uint64_t* __restrict__ m_off, const uint32_t* __restrict__ cnt,
                                                               uint32_t* __restrict__ pre, uint32_t* __restrict__ k_out)
{
  __shared__ uint32_t part[REPEAT_T];
  const uint32_t tid = threadIdx.x;
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint32_t P = rp_period_range(seq_len[a], max_period);
    const uint32_t* c = cnt + m_off[a];
    uint32_t* o = pre + m_off[a];
    uint32_t carry = 0;                                         // (the same in every thread)
    for (uint32_t base = 0; base < P; base += REPEAT_T) {
      const uint32_t i = base + tid, v = i < P ? c[i] : 0u;
      part[tid] = v;
      __syncthreads();
      for (uint32_t d = 1; d < REPEAT_T; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
      }
      if (i < P) o[i] = carry + part[tid] - v;
      carry += part[REPEAT_T - 1];
      __syncthreads();
    }
    if (tid == 0) k_out[a] = carry;
  }
}

// ---- the parse, one workgroup per allele.  The parse state (x, H, depth, prev, the pending literal, the counts) is computed by every thread
// from the reductions' results, so it is the same in all of them; thread 0 writes the stack and the segments.
__global__ __launch_bounds__(REPEAT_T) void repeat_select(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                         const uint32_t* __restrict__ seq_len, uint32_t n, uint32_t min_copies, uint32_t min_span,
                                                         const uint64_t* __restrict__ run_off, const RpRun* __restrict__ runs, uint2* __restrict__ stack,
                                                         const uint64_t* __restrict__ sc_off, otg_repeat_seg* __restrict__ scratch,
                                                         otg_repeat_sum* __restrict__ sums, uint32_t* __restrict__ overflow)
{
  __shared__ RpCand red[REPEAT_T];
  __shared__ uint32_t red_t[REPEAT_T];
  const uint32_t tid = threadIdx.x;
  for (uint32_t al = blockIdx.x; al < n; al += gridDim.x) {
    const uint32_t L = seq_len[al], K = (uint32_t)(run_off[al + 1] - run_off[al]), cap = (uint32_t)(sc_off[al + 1] - sc_off[al]);
    const uint8_t* s = arena + seq_off[al];
    const RpRun* R = runs + run_off[al];
    uint2* ST = stack + run_off[al];
    otg_repeat_seg* SG = scratch + sc_off[al];
    uint32_t x = 0, H = L, depth = 0, prev_p = 0, prev_b = 0, lit_b = 0, lit_len = 0, nseg = 0, nrep = 0, covered = 0;
    bool over = false;
    // a segment goes to SG[nseg]; adjacent literals have been merged into the pending one (lit_b, lit_len) before they get here
    auto emit = [&](uint32_t begin, uint32_t period, uint32_t copies, uint32_t length) {
      if (nseg >= cap) { over = true; return; }
      if (tid == 0) { otg_repeat_seg g; g.begin = begin; g.period = period; g.copies = copies; g.length = length; SG[nseg] = g; }
      ++nseg;
    };
    while (L != 0u && !over) {
      RpCand c = {0u, 0u, 0u, 0u, 0u};
      for (uint32_t i = tid; i < K; i += REPEAT_T) {
        const RpCand cc = rp_cand(R[i], i, x, H, min_copies, min_span);
        if (rp_better(cc, c)) c = cc;
      }
      red[tid] = c;
      __syncthreads();
      for (uint32_t d = REPEAT_T / 2; d > 0; d >>= 1) {
        if (tid < d && rp_better(red[tid + d], red[tid])) red[tid] = red[tid + d];
        __syncthreads();
      }
      const RpCand b = red[0];
      __syncthreads();
      uint32_t ri;
      if (b.w == 0u) {                                          // nothing under this horizon: the rest of it is a literal
        if (H > x) { if (lit_len == 0u) lit_b = x; lit_len += H - x; }
        x = H;
        if (depth == 0u) break;
        --depth;
        const uint2 top = ST[depth];                            // written by thread 0 in front of a barrier
        ri = top.x; H = top.y;
      } else if (b.st > x) {                                    // the gap in front of the run is parsed first, under the run's start
        if (depth >= K) { over = true; break; }
        if (tid == 0) ST[depth] = make_uint2(b.idx, H);
        ++depth;
        H = b.st;
        continue;
      } else ri = b.idx;
      // place run ri at x under H
      const RpRun run = R[ri];
      const uint32_t p = run.p, en = run.e < H ? run.e : H;
      uint32_t st = x;
      if (prev_p == p) {                                        // keep the unit's phase: the smallest t whose unit is the previous one's
        const uint32_t t_end = x + p < en - p + 1u ? x + p : en - p + 1u;
        uint32_t found = 0xffffffffu;
        for (uint32_t t = x + tid; t < t_end; t += REPEAT_T)
          if (rp_unit_equal(s, t, prev_b, p)) { found = t; break; }
        red_t[tid] = found;
        __syncthreads();
        for (uint32_t d = REPEAT_T / 2; d > 0; d >>= 1) {
          if (tid < d && red_t[tid + d] < red_t[tid]) red_t[tid] = red_t[tid + d];
          __syncthreads();
        }
        found = red_t[0];
        __syncthreads();
        if (found != 0xffffffffu && rp_enough((en - found) / p, p, min_copies, min_span)) st = found;
      }
      if (st > x) { if (lit_len == 0u) lit_b = x; lit_len += st - x; }
      if (lit_len) { emit(lit_b, 0u, 0u, lit_len); lit_len = 0u; }
      const uint32_t k = (en - st) / p;
      emit(st, p, k, k * p);
      ++nrep; covered += k * p;
      prev_p = p; prev_b = st;
      x = st + k * p;
    }
    if (lit_len && !over) emit(lit_b, 0u, 0u, lit_len);
    if (tid == 0) {
      otg_repeat_sum sm;
      sm.n_segments = nseg; sm.n_repeats = nrep; sm.covered = covered; sm.flags = L > OTG_REPEAT_MAX_LEN ? OTG_REPEAT_TOO_LONG : 0u;
      sums[al] = sm;
      if (over) *overflow = 1u;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(REPEAT_T) void repeat_compact(uint32_t n, const otg_repeat_sum* __restrict__ sums, const uint64_t* __restrict__ sc_off,
                                                          const otg_repeat_seg* __restrict__ scratch, const uint64_t* __restrict__ seg_off,
                                                          otg_repeat_seg* __restrict__ segs)
{
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint32_t ns = sums[a].n_segments;
    for (uint32_t i = threadIdx.x; i < ns; i += REPEAT_T) segs[seg_off[a] + i] = scratch[sc_off[a] + i];
  }
}

} // namespace

int otg_repeat_args(otg_ctx* ctx, const char* who, uint32_t max_period, uint32_t min_copies, uint32_t min_span)
{
  if (max_period < 1 || max_period > OTG_REPEAT_MAX_PERIOD)
    return otg_fail(ctx, OTG_ERR_ARG, "%s: max_period = %u outside 1..%d", who, max_period, OTG_REPEAT_MAX_PERIOD);
  if (min_copies < 2 || min_copies > 1024) return otg_fail(ctx, OTG_ERR_ARG, "%s: min_copies = %u outside 2..1024", who, min_copies);
  if (min_span < 2 || min_span > 65535) return otg_fail(ctx, OTG_ERR_ARG, "%s: min_span = %u outside 2..65535", who, min_span);
  return OTG_OK;
}

// The launch part of otg_repeat_batch on device-resident rows, as otg_motif_resident: row i is rows.arena[rows.off[i] .. + rows.len[i]), the arena
// extends 31 bytes past every row.  The results land in SLOT_REPEAT_RES (n summaries, then n + 1 offsets) and SLOT_REPEAT_SEGS.
int otg_repeat_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, uint32_t n, uint32_t max_period, uint32_t min_copies, uint32_t min_span,
                        otg_repeat_sum* sums, uint64_t* seg_off, uint64_t* n_segments)
{
  ctx->last_repeat = OtgSegLast{};
  ctx->last_repeat_rows = OtgRows{nullptr, nullptr, nullptr};
  ++ctx->repeat_serial;
  if (n_segments) *n_segments = 0;
  if (n == 0) {
    if (seg_off) seg_off[0] = 0;
    return OTG_OK;
  }
  if (n > (1u << 24)) return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: %u alleles in one call, at most %u", who, n, 1u << 24);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->ev2) HIP_TRY(ctx, hipEventCreate(&ctx->ev2));
  const uint32_t lds_len = otg_motif_lds_len();
  // offsets: m_off | pl_off | run_off | sc_off (u64, n + 1 each) | four totals and the overflow word | K (u32, n)
  uint64_t* d_moff = (uint64_t*)otg_slot(ctx, SLOT_REPEAT_OFF, ((size_t)4 * (n + 1) + 5) * 8 + (size_t)n * 4);
  uint8_t* d_res = (uint8_t*)otg_slot(ctx, SLOT_REPEAT_RES, (size_t)n * sizeof(otg_repeat_sum) + ((size_t)n + 1) * 8);
  if (!d_moff || !d_res) return OTG_ERR_HIP;
  uint64_t* d_ploff = d_moff + (n + 1);
  uint64_t* d_runoff = d_ploff + (n + 1);
  uint64_t* d_scoff = d_runoff + (n + 1);
  uint64_t* d_tot = d_scoff + (n + 1);
  uint32_t* d_over = (uint32_t*)(d_tot + 4);
  uint32_t* d_k = (uint32_t*)(d_tot + 5);
  otg_repeat_sum* d_sums = (otg_repeat_sum*)d_res;
  uint64_t* d_segoff = (uint64_t*)(d_res + (size_t)n * sizeof(otg_repeat_sum));
  HIP_TRY(ctx, hipMemsetAsync(d_tot, 0, 40, ctx->stream));
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, RpPeriods>), dim3(1), dim3(1024), 0, ctx->stream, RpPeriods{rows.len, max_period}, n, d_moff, d_tot);
  otg_motif_plane_scan(ctx, rows.len, n, max_period, lds_len, d_ploff, d_tot + 1);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t tot[4] = {0, 0, 0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // per (allele, period): the count of kept runs | its exclusive scan within the allele
  uint32_t* d_cnt = (uint32_t*)otg_slot(ctx, SLOT_REPEAT_CNT, (size_t)tot[0] * 8 + 8);
  uint32_t* d_planes = tot[1] ? (uint32_t*)otg_slot(ctx, SLOT_REPEAT_PLANES, (size_t)tot[1] * 12) : nullptr;
  if (!d_cnt || (tot[1] && !d_planes)) return OTG_ERR_HIP;
  uint32_t* d_pre = d_cnt + tot[0];
  const uint32_t grid = std::min<uint32_t>(n, 1u << 20);
  const dim3 hbm_grid(n, (max_period + REPEAT_T - 1) / REPEAT_T);
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (lds_len)
    hipLaunchKernelGGL(repeat_runs_lds<false>, dim3(grid), dim3(REPEAT_T), 0, ctx->stream, rows.arena, rows.off, rows.len, n, max_period, lds_len, min_copies, min_span,
                       d_moff, d_cnt, nullptr, nullptr, nullptr);
  if (tot[1]) {
    otg_motif_pack_planes(ctx, rows.arena, rows.off, rows.len, n, d_ploff, d_planes);
    hipLaunchKernelGGL(repeat_runs_hbm<false>, hbm_grid, dim3(REPEAT_T), 0, ctx->stream, rows.len, n, max_period, min_copies, min_span, d_ploff, d_planes, d_moff,
                       d_cnt, nullptr, nullptr, nullptr);
  }
  hipLaunchKernelGGL(repeat_scan_periods, dim3(grid), dim3(REPEAT_T), 0, ctx->stream, rows.len, n, max_period, d_moff, d_cnt, d_pre, d_k);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, OtgScanPtr<uint32_t>>), dim3(1), dim3(1024), 0, ctx->stream, OtgScanPtr<uint32_t>{d_k}, n, d_runoff, d_tot + 2);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, RpSegCap>), dim3(1), dim3(1024), 0, ctx->stream, RpSegCap{d_k}, n, d_scoff, d_tot + 3);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(tot + 2, d_tot + 2, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // the runs, the horizon stacks (one entry per run) and the segment scratch
  RpRun* d_runs = (RpRun*)otg_slot(ctx, SLOT_REPEAT_RUNS, (size_t)tot[2] * sizeof(RpRun) + 16);
  uint2* d_stack = (uint2*)otg_slot(ctx, SLOT_REPEAT_STACK, (size_t)tot[2] * sizeof(uint2) + 16);
  otg_repeat_seg* d_scratch = (otg_repeat_seg*)otg_slot(ctx, SLOT_REPEAT_SCRATCH, (size_t)tot[3] * sizeof(otg_repeat_seg));
  if (!d_runs || !d_stack || !d_scratch) return OTG_ERR_HIP;
  if (tot[2]) {
    if (lds_len)
      hipLaunchKernelGGL(repeat_runs_lds<true>, dim3(grid), dim3(REPEAT_T), 0, ctx->stream, rows.arena, rows.off, rows.len, n, max_period, lds_len, min_copies, min_span,
                         d_moff, d_cnt, d_pre, d_runoff, d_runs);
    if (tot[1])
      hipLaunchKernelGGL(repeat_runs_hbm<true>, hbm_grid, dim3(REPEAT_T), 0, ctx->stream, rows.len, n, max_period, min_copies, min_span, d_ploff, d_planes, d_moff,
                         d_cnt, d_pre, d_runoff, d_runs);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  hipLaunchKernelGGL(repeat_select, dim3(grid), dim3(REPEAT_T), 0, ctx->stream, rows.arena, rows.off, rows.len, n, min_copies, min_span, d_runoff, d_runs, d_stack, d_scoff,
                     d_scratch, d_sums, d_over);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, RpSegCount>), dim3(1), dim3(1024), 0, ctx->stream, RpSegCount{d_sums}, n, d_segoff, d_tot);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t fin[5] = {0, 0, 0, 0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(fin, d_tot, 40, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if ((uint32_t)fin[4]) return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: an allele gave more segments than two per kept run and one", who);
  const uint64_t total = fin[0];
  otg_repeat_seg* d_segs = (otg_repeat_seg*)otg_slot(ctx, SLOT_REPEAT_SEGS, (size_t)total * sizeof(otg_repeat_seg) + 16);
  if (!d_segs) return OTG_ERR_HIP;
  hipLaunchKernelGGL(repeat_compact, dim3(grid), dim3(REPEAT_T), 0, ctx->stream, n, d_sums, d_scoff, d_scratch, d_segoff, d_segs);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  if (sums) HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, (size_t)n * sizeof(otg_repeat_sum), hipMemcpyDeviceToHost, ctx->stream));
  if (seg_off) HIP_TRY(ctx, hipMemcpyAsync(seg_off, d_segoff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float r_ms = 0.f, s_ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&r_ms, ctx->ev0, ctx->ev1));
  HIP_TRY(ctx, hipEventElapsedTime(&s_ms, ctx->ev1, ctx->ev2));
  ctx->last_repeat = OtgSegLast{n, total, true, {r_ms, s_ms}};
  ctx->last_repeat_rows = rows;
  if (n_segments) *n_segments = total;
  return OTG_OK;
}

extern "C" int otg_repeat_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                                uint32_t n, uint32_t max_period, uint32_t min_copies, uint32_t min_span, otg_repeat_sum* sums, uint64_t* seg_off,
                                uint64_t* n_segments)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_repeat_batch: no context (no HIP device?)");
  if (int rc = otg_repeat_args(ctx, "otg_repeat_batch", max_period, min_copies, min_span)) return rc;
  if (int rc = otg_rows_check(ctx, "otg_repeat_batch", seq_arena, arena_bytes, seq_off, seq_len, n, nullptr)) return rc;
  OtgRows rows = {nullptr, nullptr, nullptr};
  if (n != 0 && n <= (1u << 24))                                  // (otherwise the launch part answers before it reads a row)
    if (int rc = otg_rows_upload(ctx, SLOT_REPEAT_SEQ, SLOT_REPEAT_META, seq_arena, arena_bytes, seq_off, seq_len, n, &rows)) return rc;
  return otg_repeat_resident(ctx, "otg_repeat_batch", rows, n, max_period, min_copies, min_span, sums, seg_off, n_segments);
}

extern "C" int otg_repeat_collect(otg_ctx* ctx, otg_repeat_seg* segs, uint64_t capacity)
{
  return otg_seg_collect(ctx, "otg_repeat_collect", "repeat", &otg_ctx::last_repeat, SLOT_REPEAT_SEGS, sizeof(otg_repeat_seg), segs, capacity);
}

extern "C" int otg_repeat_device_results(otg_ctx* ctx, uint32_t* n, const otg_repeat_sum** sums, const uint64_t** seg_off, const otg_repeat_seg** segs,
                                         uint64_t* total)
{
  return otg_seg_device_results(ctx, "otg_repeat_device_results", "repeat", &otg_ctx::last_repeat, SLOT_REPEAT_RES, SLOT_REPEAT_SEGS, sizeof(otg_repeat_sum), n,
                                (const void**)sums, seg_off, (const void**)segs, total);
}

extern "C" int otg_repeat_last_ms(otg_ctx* ctx, double* runs_ms, double* select_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_repeat_last_ms: NULL context");
  if (runs_ms) *runs_ms = ctx->last_repeat.ms[0];
  if (select_ms) *select_ms = ctx->last_repeat.ms[1];
  return OTG_OK;
}

// motif.hip — tandem-repeat motif annotation of alleles (otg_motif_batch / otg_motif_cohort): per allele the repeat period, the unit, and
// the match counts that give copies and purity.  The reference has no counterpart; include/otter_gpu.h states the rule.
//
// An allele is packed once into three bit-planes of 32 bases per word: bit 0 and bit 1 of the base code (A/a=0 C/c=1 G/g=2 T/t=3) and `valid`
// (an ACGT byte below L).  The planes end in zero words, so a base past the end is invalid and the L - p tail of a shifted compare needs no
// mask of its own.  m(p) = #{i < L - p : s[i] == s[i+p], both ACGT} is a shifted self-comparison: lanes own periods and sweep the words, per
// word one funnel shift per plane (v_alignbit), ~((lo ^ lo') | (hi ^ hi')) & v & v', a popcount.  Two tiers by where the planes live:
//   LDS,  L <= MOTIF_LDS_LEN: one 256-thread workgroup per allele packs the planes into LDS and counts from there;
//   HBM,  L <= OTG_MOTIF_MAX_LEN (and everything under OTG_MOTIF_WIDE): a pack kernel writes the planes into the context's workspace, the count
//         kernel runs one workgroup per allele and 256 periods.
// Both write m(1..P) of an allele at its offset in one u32 array (the offsets are a device scan of P = min(max_period, L / 2)).  One
// reduce-and-unit kernel serves both: best period (exact 64-bit cross-multiplied compares; the order of a tie is fixed by the period, not
// by the lane), selected period, phase majority, smallest rotation.  Only the records and the unit bytes leave the device.
#include "otg_common.hpp"
#include "otg_scan.hpp"
#include "otg_motif_core.hpp"
#include <algorithm>
#include <cstdlib>

namespace {

constexpr uint32_t MOTIF_LDS_LEN = OTG_MOTIF_LDS_LEN;            // longest allele of the LDS tier
constexpr uint32_t MOTIF_LDS_WORDS = MOTIF_LDS_LEN / 32 + 2;    // words of one plane there, the two zero words included
using namespace otg_motif_core;

// per allele the number of periods (the slots of m) / the words of one plane in the HBM workspace (0: the LDS tier counts it)
struct MoPeriods {
  const uint32_t* len; uint32_t max_period;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return mo_period_range(len[i], max_period); }
};
struct MoPlaneWords {
  const uint32_t* len; uint32_t max_period, lds_len;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const
  {
    const uint32_t L = len[i];
    return mo_period_range(L, max_period) == 0u || L <= lds_len ? 0u : (L + 31u) / 32u + 2u;
  }
};

// ---- LDS tier: pack and count, one workgroup per allele
__global__ __launch_bounds__(MOTIF_T) void motif_count_lds(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                          const uint32_t* __restrict__ seq_len, uint32_t n, uint32_t max_period, uint32_t lds_len,
                                                          const uint64_t* __restrict__ m_off, uint32_t* __restrict__ m_out)
{
  __shared__ uint32_t LO[MOTIF_LDS_WORDS], HI[MOTIF_LDS_WORDS], V[MOTIF_LDS_WORDS];
  const uint32_t tid = threadIdx.x;
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint32_t L = seq_len[a], P = mo_period_range(L, max_period);
    if (P == 0u || L > lds_len) continue;                       // (block-uniform)
    const uint8_t* s = arena + seq_off[a];
    const uint32_t W = (L + 31u) >> 5;
    for (uint32_t w = tid; w < W + 2u; w += MOTIF_T) {
      uint32_t l = 0, h = 0, v = 0;
      if (w < W) mo_pack_word(s, L, w, &l, &h, &v);
      LO[w] = l; HI[w] = h; V[w] = v;
    }
    __syncthreads();
    uint32_t* m = m_out + m_off[a];
    for (uint32_t p = 1u + tid; p <= P; p += MOTIF_T) m[p - 1u] = mo_count(LO, HI, V, L, p);
    __syncthreads();
  }
}

// ---- HBM tier: the planes of allele a are 3 x (W + 2) words at planes + 3 pl_off[a]
__global__ __launch_bounds__(MOTIF_T) void motif_pack_hbm(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                         const uint32_t* __restrict__ seq_len, uint32_t n, const uint64_t* __restrict__ pl_off,
                                                         uint32_t* __restrict__ planes)
{
  const uint32_t a = blockIdx.x;
  if (a >= n || pl_off[a + 1] == pl_off[a]) return;
  const uint32_t L = seq_len[a], W = (L + 31u) >> 5, PW = W + 2u;
  const uint8_t* s = arena + seq_off[a];
  uint32_t* LO = planes + 3u * pl_off[a];
  uint32_t* HI = LO + PW;
  uint32_t* V = HI + PW;
  for (uint32_t w = blockIdx.y * MOTIF_T + threadIdx.x; w < PW; w += gridDim.y * MOTIF_T) {
    uint32_t l = 0, h = 0, v = 0;
    if (w < W) mo_pack_word(s, L, w, &l, &h, &v);
    LO[w] = l; HI[w] = h; V[w] = v;
  }
}

__global__ __launch_bounds__(MOTIF_T) void motif_count_hbm(const uint32_t* __restrict__ seq_len, uint32_t n, uint32_t max_period,
                                                          const uint64_t* __restrict__ pl_off, const uint32_t* __restrict__ planes,
                                                          const uint64_t* __restrict__ m_off, uint32_t* __restrict__ m_out)
{
  const uint32_t a = blockIdx.x;
  if (a >= n || pl_off[a + 1] == pl_off[a]) return;
  const uint32_t L = seq_len[a], P = mo_period_range(L, max_period), PW = ((L + 31u) >> 5) + 2u;
  const uint32_t p = 1u + blockIdx.y * MOTIF_T + threadIdx.x;
  if (p > P) return;
  const uint32_t* LO = planes + 3u * pl_off[a];
  const uint32_t* HI = LO + PW;
  const uint32_t* V = HI + PW;
  m_out[m_off[a] + (p - 1u)] = mo_count(LO, HI, V, L, p);
}

// ---- reduce and unit, one workgroup per allele
__global__ __launch_bounds__(MOTIF_T) void motif_reduce_unit(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                            const uint32_t* __restrict__ seq_len, uint32_t n, uint32_t max_period, uint32_t slack,
                                                            const uint64_t* __restrict__ m_off, const uint32_t* __restrict__ m_all,
                                                            otg_motif* __restrict__ out, uint8_t* __restrict__ unit_out, uint32_t unit_stride)
{
  __shared__ uint32_t red_p[MOTIF_T], red_m[MOTIF_T];
  __shared__ uint32_t cnt[MOTIF_T][4];
  __shared__ uint8_t unit[OTG_MOTIF_MAX_PERIOD];
  const uint32_t tid = threadIdx.x;
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint32_t L = seq_len[a], P = mo_period_range(L, max_period);
    otg_motif rec;
    rec.period = rec.matches = rec.compared = rec.best_period = rec.reserved = 0u;
    rec.flags = L > OTG_MOTIF_MAX_LEN ? OTG_MOTIF_TOO_LONG : 0u;
    if (P == 0u) {                                              // (block-uniform)
      if (tid == 0) out[a] = rec;
      continue;
    }
    const uint32_t* m = m_all + m_off[a];                        // m(p) = m[p - 1], 1 <= p <= P
    // best period: the thread's own periods in ascending order, then the tree; mo_better is a total order, so neither changes the winner
    uint32_t bp = 0, bm = 0;
    for (uint32_t p = 1u + tid; p <= P; p += MOTIF_T) {
      const uint32_t mp = m[p - 1u];
      if (mo_better(L, p, mp, bp, bm)) { bp = p; bm = mp; }
    }
    red_p[tid] = bp; red_m[tid] = bm;
    __syncthreads();
    for (uint32_t d = MOTIF_T / 2; d > 0; d >>= 1) {
      if (tid < d && mo_better(L, red_p[tid + d], red_m[tid + d], red_p[tid], red_m[tid])) { red_p[tid] = red_p[tid + d]; red_m[tid] = red_m[tid + d]; }
      __syncthreads();
    }
    const uint32_t best = red_p[0], mbest = red_m[0];
    __syncthreads();
    if (mbest == 0u) {
      if (tid == 0) out[a] = rec;
      continue;
    }
    // selected period: the smallest p <= best within the slack of the best ratio (p = best always is)
    uint32_t sel = best;
    for (uint32_t p = 1u + tid; p <= best; p += MOTIF_T)
      if (mo_within_slack(L, p, m[p - 1u], best, mbest, slack)) { sel = p; break; }
    red_p[tid] = sel;
    __syncthreads();
    for (uint32_t d = MOTIF_T / 2; d > 0; d >>= 1) {
      if (tid < d && red_p[tid + d] < red_p[tid]) red_p[tid] = red_p[tid + d];
      __syncthreads();
    }
    const uint32_t period = red_p[0];
    __syncthreads();
    // unit: the majority base of every phase (ties to the lower code, no ACGT byte: N)
    const uint8_t* s = arena + seq_off[a];
    if (period <= MOTIF_T) {
      // k = 256 / period threads share a phase; thread t takes the positions j + period (r + k i) of phase j = t % period, r = t / period
      const uint32_t k = MOTIF_T / period, j = tid % period, r = tid / period;
      cnt[tid][0] = cnt[tid][1] = cnt[tid][2] = cnt[tid][3] = 0u;
      __syncthreads();
      if (r < k) {
        uint32_t c[4] = {0u, 0u, 0u, 0u};
        for (uint64_t i = j + (uint64_t)period * r; i < L; i += (uint64_t)period * k) {
          const uint32_t code = mo_code(s[i]);
          c[0] += code == 0u; c[1] += code == 1u; c[2] += code == 2u; c[3] += code == 3u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) if (c[q]) atomicAdd(&cnt[j][q], c[q]);
      }
      __syncthreads();
      if (tid < period) unit[tid] = mo_majority(cnt[tid][0], cnt[tid][1], cnt[tid][2], cnt[tid][3]);
    } else {
      for (uint32_t j = tid; j < period; j += MOTIF_T) {
        uint32_t c[4] = {0u, 0u, 0u, 0u};
        for (uint32_t i = j; i < L; i += period) {
          const uint32_t code = mo_code(s[i]);
          c[0] += code == 0u; c[1] += code == 1u; c[2] += code == 2u; c[3] += code == 3u;
        }
        unit[j] = mo_majority(c[0], c[1], c[2], c[3]);
      }
    }
    __syncthreads();
    // smallest rotation: the thread's own offsets, then the tree (mo_rot_less is a total order)
    uint32_t rot = tid < period ? tid : 0u;
    for (uint32_t o = tid + MOTIF_T; o < period; o += MOTIF_T)
      if (mo_rot_less(unit, period, o, rot)) rot = o;
    red_p[tid] = rot;
    __syncthreads();
    for (uint32_t d = MOTIF_T / 2; d > 0; d >>= 1) {
      if (tid < d && mo_rot_less(unit, period, red_p[tid + d], red_p[tid])) red_p[tid] = red_p[tid + d];
      __syncthreads();
    }
    rot = red_p[0];
    uint8_t* u = unit_out + (size_t)a * unit_stride;
    for (uint32_t i = tid; i < period; i += MOTIF_T) { const uint32_t src = rot + i; u[i] = unit[src < period ? src : src - period]; }
    if (tid == 0) {
      rec.period = period; rec.matches = m[period - 1u]; rec.compared = L - period; rec.best_period = best;
      out[a] = rec;
    }
    __syncthreads();
  }
}

bool motif_force_wide()
{
  static const bool on = [] { const char* e = getenv("OTG_MOTIF_WIDE"); return e && *e && strcmp(e, "0") != 0; }();
  return on;
}

} // namespace

uint32_t otg_motif_lds_len() { return motif_force_wide() ? 0u : MOTIF_LDS_LEN; }

void otg_motif_plane_scan(otg_ctx* ctx, const uint32_t* d_len, uint32_t n, uint32_t max_period, uint32_t lds_len, uint64_t* d_ploff, uint64_t* d_total)
{
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, MoPlaneWords>), dim3(1), dim3(1024), 0, ctx->stream, MoPlaneWords{d_len, max_period, lds_len}, n,
                     d_ploff, d_total);
}

// a grid over every allele: the workgroups of an allele without planes in HBM (pl_off unchanged) return at once
void otg_motif_pack_planes(otg_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len, uint32_t n, const uint64_t* d_ploff,
                           uint32_t* d_planes)
{
  hipLaunchKernelGGL(motif_pack_hbm, dim3(n, 8), dim3(MOTIF_T), 0, ctx->stream, d_arena, d_off, d_len, n, d_ploff, d_planes);
}

int otg_motif_args(otg_ctx* ctx, const char* who, uint32_t max_period, uint32_t slack)
{
  if (max_period < 1 || max_period > OTG_MOTIF_MAX_PERIOD)
    return otg_fail(ctx, OTG_ERR_ARG, "%s: max_period = %u outside 1..%d", who, max_period, OTG_MOTIF_MAX_PERIOD);
  if (slack > 999) return otg_fail(ctx, OTG_ERR_ARG, "%s: slack = %u outside 0..999 (per mille)", who, slack);
  return OTG_OK;
}

// The launch part of otg_motif_batch on device-resident rows: row i is rows.arena[rows.off[i] .. + rows.len[i]), and the pack reads up to 31 bytes past
// a row, so the arena must extend that far past every row.  The caller has checked unit_stride against the longest row
// (otg_motif_stride_fits).  The results land in SLOT_MOTIF_OUT (otg_motif_device_results): n records, then n x unit_stride unit bytes (zero beyond a unit's period).
int otg_motif_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, uint32_t n, uint32_t max_period, uint32_t slack, otg_motif* out,
                       uint8_t* unit_out, uint32_t unit_stride)
{
  ctx->last_motif_count_ms = ctx->last_motif_reduce_ms = 0.0;
  ctx->last_motif_n = 0; ctx->last_motif_stride = 0;
  if (n == 0) return OTG_OK;
  if (n > (1u << 24)) return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: %u alleles in one call, at most %u", who, n, 1u << 24);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->ev2) HIP_TRY(ctx, hipEventCreate(&ctx->ev2));
  const uint32_t lds_len = otg_motif_lds_len();
  // offsets: m_off (u64, n + 1) | pl_off (u64, n + 1) | the two totals
  uint64_t* d_moff = (uint64_t*)otg_slot(ctx, SLOT_MOTIF_OFF, ((size_t)2 * n + 4) * 8);
  const size_t rec_bytes = (size_t)n * sizeof(otg_motif), unit_bytes = (size_t)n * unit_stride;
  uint8_t* d_out = (uint8_t*)otg_slot(ctx, SLOT_MOTIF_OUT, rec_bytes + unit_bytes);
  if (!d_moff || !d_out) return OTG_ERR_HIP;
  uint64_t* d_ploff = d_moff + (n + 1);
  uint64_t* d_tot = d_ploff + (n + 1);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, MoPeriods>), dim3(1), dim3(1024), 0, ctx->stream, MoPeriods{rows.len, max_period}, n, d_moff, d_tot);
  otg_motif_plane_scan(ctx, rows.len, n, max_period, lds_len, d_ploff, d_tot + 1);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t tot[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t* d_m = (uint32_t*)otg_slot(ctx, SLOT_MOTIF_M, (size_t)tot[0] * 4);
  uint32_t* d_planes = tot[1] ? (uint32_t*)otg_slot(ctx, SLOT_MOTIF_PLANES, (size_t)tot[1] * 12) : nullptr;
  if (!d_m || (tot[1] && !d_planes)) return OTG_ERR_HIP;
  otg_motif* d_rec = (otg_motif*)d_out;
  uint8_t* d_unit = d_out + rec_bytes;
  if (unit_bytes) HIP_TRY(ctx, hipMemsetAsync(d_unit, 0, unit_bytes, ctx->stream));
  const uint32_t grid = std::min<uint32_t>(n, 1u << 20);
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (lds_len) hipLaunchKernelGGL(motif_count_lds, dim3(grid), dim3(MOTIF_T), 0, ctx->stream, rows.arena, rows.off, rows.len, n, max_period, lds_len, d_moff, d_m);
  if (tot[1]) {              // grids over every allele: the workgroups of an allele without planes in HBM (pl_off unchanged) return at once
    otg_motif_pack_planes(ctx, rows.arena, rows.off, rows.len, n, d_ploff, d_planes);
    hipLaunchKernelGGL(motif_count_hbm, dim3(n, (max_period + MOTIF_T - 1) / MOTIF_T), dim3(MOTIF_T), 0, ctx->stream, rows.len, n, max_period, d_ploff, d_planes, d_moff, d_m);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  hipLaunchKernelGGL(motif_reduce_unit, dim3(grid), dim3(MOTIF_T), 0, ctx->stream, rows.arena, rows.off, rows.len, n, max_period, slack, d_moff, d_m, d_rec, d_unit, unit_stride);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  if (out) HIP_TRY(ctx, hipMemcpyAsync(out, d_rec, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (unit_out && unit_bytes) HIP_TRY(ctx, hipMemcpyAsync(unit_out, d_unit, unit_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float c_ms = 0.f, r_ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&c_ms, ctx->ev0, ctx->ev1));
  HIP_TRY(ctx, hipEventElapsedTime(&r_ms, ctx->ev1, ctx->ev2));
  ctx->last_motif_count_ms = c_ms; ctx->last_motif_reduce_ms = r_ms;
  ctx->last_motif_n = n; ctx->last_motif_stride = unit_stride;
  ctx->last_motif_rows = rows;
  return OTG_OK;
}

int otg_motif_stride_fits(otg_ctx* ctx, const char* who, uint32_t max_len, uint32_t max_period, uint32_t unit_stride)
{
  const uint32_t need = std::min<uint32_t>(max_period, max_len / 2);
  if (unit_stride < need)
    return otg_fail(ctx, OTG_ERR_ARG, "%s: unit_stride = %u, a unit may have min(max_period, longest allele / 2) = %u bytes", who, unit_stride, need);
  return OTG_OK;
}

extern "C" int otg_motif_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                               uint32_t n, uint32_t max_period, uint32_t slack, otg_motif* out, uint8_t* unit_out, uint32_t unit_stride)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_motif_batch: no context (no HIP device?)");
  if (int rc = otg_motif_args(ctx, "otg_motif_batch", max_period, slack)) return rc;
  uint32_t max_len = 0;
  if (int rc = otg_rows_check(ctx, "otg_motif_batch", seq_arena, arena_bytes, seq_off, seq_len, n, &max_len)) return rc;
  if (int rc = otg_motif_stride_fits(ctx, "otg_motif_batch", max_len, max_period, unit_stride)) return rc;
  ctx->last_motif_count_ms = ctx->last_motif_reduce_ms = 0.0;
  ctx->last_motif_n = 0; ctx->last_motif_stride = 0;
  if (n == 0) return OTG_OK;
  OtgRows rows;
  if (int rc = otg_rows_upload(ctx, SLOT_MOTIF_SEQ, SLOT_MOTIF_META, seq_arena, arena_bytes, seq_off, seq_len, n, &rows)) return rc;
  return otg_motif_resident(ctx, "otg_motif_batch", rows, n, max_period, slack, out, unit_out, unit_stride);
}

extern "C" int otg_motif_device_results(otg_ctx* ctx, uint32_t* n, const otg_motif** records, const uint8_t** units, uint32_t* unit_stride)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_motif_device_results: NULL context");
  const DevBuf& b = ctx->pool[SLOT_MOTIF_OUT];
  if (!b.p || ctx->last_motif_n == 0) return otg_fail(ctx, OTG_ERR_ARG, "otg_motif_device_results: no motif results on this context");
  if (n) *n = ctx->last_motif_n;
  if (records) *records = (const otg_motif*)b.p;
  if (units) *units = (const uint8_t*)b.p + (size_t)ctx->last_motif_n * sizeof(otg_motif);
  if (unit_stride) *unit_stride = ctx->last_motif_stride;
  return OTG_OK;
}

extern "C" int otg_motif_last_ms(otg_ctx* ctx, double* count_ms, double* reduce_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_motif_last_ms: NULL context");
  if (count_ms) *count_ms = ctx->last_motif_count_ms;
  if (reduce_ms) *reduce_ms = ctx->last_motif_reduce_ms;
  return OTG_OK;
}

// kmer_usage.hip — the per-allele work of `otter vcf2mat` (src/vcf2mat.cpp:38-46,66-72): k-mer counts (seq2kcounts,
// src/anseqs.cpp:149-166), frequencies (KUSAGE, :111-121), Hill-Shannon diversity (KUSAGE::hsdiv, :135-147) and GC fraction
// (get_gc_content), for a batch of alleles and any 1 <= k <= 12.
//
// A window of k bytes is counted once: bin = its base-4 code (A/a=0 C/c=1 G/g=2 T/t=3, first base most significant) when all k bytes are
// ACGTacgt, else the last bin 4^k.  Every window is counted, so total = L-k+1 (L >= k) or 0 without summing the bins.  Three counting tiers by
// the number of bins:
//   S, k <= 4 (<= 256 ACGT bins): one wave per allele; every lane counts into its own u16 column of an LDS histogram [bin][lane] (no atomics),
//      folded into u32 registers every 4095 tiles and at the end (a lane adds at most 16 per tile and column);
//   M, k 5..7 (<= 16 384 ACGT bins = 64 KiB of u32): one 256-thread workgroup per allele, one LDS histogram, LDS atomics;
//   L, k 8..12: per-allele u32 histograms in HBM (global atomics), up to 64 KiB of windows per workgroup, then a division pass over all
//      (allele, bin) and a per-allele diversity pass.
// In every tier the bin 4^k is a register count (summed per wave or workgroup), and a lane takes 16 consecutive window starts of a tile from
// one 16-byte load plus the k-1 bytes after them (lanes of a wave read 1 KiB contiguously; the device arena ends in 64 bytes of slack).
// Epilogue: value = count / total in double (0/0 when total == 0, as the reference), GC = (C/c/G/g bytes) / L, and the diversity summed by one
// wave in ascending bin order with the lanes' terms added one at a time (ballot over the nonzero bins, which are the only terms).
#include "otg_common.hpp"
#include "otg_scan.hpp"
#include <algorithm>
#include <vector>

namespace {

constexpr int KU_SEGS = 16;                     // window starts per lane and tile
constexpr int KU_TILE_S = 64 * KU_SEGS;         // tile of the wave tier
constexpr int KU_TILE_M = 256 * KU_SEGS;        // tile of the workgroup tiers
constexpr uint32_t KU_CHUNK_L = 16 * KU_TILE_M; // window starts per workgroup in tier L
constexpr uint64_t KU_WORKSPACE = 4ull << 30;   // device bytes of one batch: usage rows (+ tier L histograms)
constexpr double KU_E = 2.718281828459045235360287471352662498;   // M_E

__device__ __forceinline__ int ku_code(uint8_t ch)
{
  return (ch == 'A' || ch == 'a') ? 0 : (ch == 'C' || ch == 'c') ? 1 : (ch == 'G' || ch == 'g') ? 2 : (ch == 'T' || ch == 't') ? 3 : 4;
}

// The 16 window starts j0 .. j0+15 of one lane (window j counted when j < nwin) and the GC bytes among positions j0 .. j0+15 below L.
// emit(bin) for a valid window, ++*inv for one that holds a non-ACGT byte.
template <int K, class F>
__device__ __forceinline__ void ku_segment(const uint8_t* s, int64_t j0, int64_t nwin, int64_t L, uint32_t* inv, uint32_t* gc, F emit)
{
  uint8_t b[32];
  __builtin_memcpy(b, s + j0, 16);
  if (K > 1) __builtin_memcpy(b + 16, s + j0 + 16, 16);
  constexpr uint32_t MASK = (K == 16) ? 0xffffffffu : ((1u << (2 * K)) - 1u);
  uint32_t idx = 0;
  int run = 0;
#pragma unroll
  for (int p = 0; p < KU_SEGS + K - 1; ++p) {
    const uint8_t ch = b[p];
    const int c = ku_code(ch);
    if (p < KU_SEGS && j0 + p < L) *gc += (c == 1 || c == 2);
    idx = ((idx << 2) | (uint32_t)(c & 3)) & MASK;
    run = c < 4 ? run + 1 : 0;
    if (p >= K - 1) {
      const int q = p - (K - 1);
      if (j0 + q < nwin) {
        if (run >= K) emit(idx);
        else *inv += 1;
      }
    }
  }
}

__device__ __forceinline__ uint32_t ku_wave_sum(uint32_t v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// acc += v*log(v) for the lanes whose count is nonzero, one lane at a time in lane order (wave-uniform acc)
__device__ __forceinline__ double ku_wave_terms(double acc, uint32_t cnt, double dtot)
{
  const double v = (double)cnt / dtot;
  const double term = cnt ? v * log(v) : 0.0;
  uint64_t mask = __ballot(cnt != 0);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    acc += __shfl(term, l);
  }
  return acc;
}

__device__ __forceinline__ int32_t ku_total(int64_t L, int K) { return L >= K ? (int32_t)(L - K + 1) : 0; }

// ---- tier S: one wave (one workgroup of 64) per allele
template <int K>
__global__ __launch_bounds__(64) void kmer_usage_wave(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                      const uint32_t* __restrict__ seq_len, uint32_t n, double* __restrict__ usage,
                                                      double* __restrict__ gc_out, double* __restrict__ hsd_out)
{
  constexpr int NB = 1 << (2 * K);
  constexpr int PER = (NB + 63) / 64;           // bins per lane: lane l holds bins l, l+64, ...
  __shared__ uint16_t H[NB * 64];
  const int lane = threadIdx.x;
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint8_t* s = arena + seq_off[a];
    const int64_t L = seq_len[a], nwin = L >= K ? L - K + 1 : 0;
    uint32_t cnt[PER], inv = 0, gc = 0;
#pragma unroll
    for (int m = 0; m < PER; ++m) cnt[m] = 0;
    for (int q = lane; q < NB * 32; q += 64) ((uint32_t*)H)[q] = 0u;
    __syncthreads();
    auto fold = [&]() {                                   // column sums: lane walks the 64 columns of its bins, rotated (distinct banks)
      __syncthreads();
#pragma unroll
      for (int m = 0; m < PER; ++m) {
        const int bin = 64 * m + lane;
        if (bin < NB)
          for (int j = 0; j < 64; ++j) {
            uint16_t& h = H[bin * 64 + ((j + lane) & 63)];
            cnt[m] += h;
            h = 0;
          }
      }
      __syncthreads();
    };
    int tiles = 0;
    for (int64_t t0 = 0; t0 < L; t0 += KU_TILE_S) {
      const int64_t j0 = t0 + (int64_t)KU_SEGS * lane;
      if (j0 < L) ku_segment<K>(s, j0, nwin, L, &inv, &gc, [&](uint32_t idx) { H[idx * 64 + lane] += 1; });   // own column: no atomics
      if (++tiles == 4095) { fold(); tiles = 0; }
    }
    fold();
    inv = ku_wave_sum(inv);
    gc = ku_wave_sum(gc);
    const int32_t total = ku_total(L, K);
    const double dtot = (double)total;
    double* row = usage + (size_t)a * (NB + 1);
    double acc = 0;
#pragma unroll
    for (int m = 0; m < PER; ++m) {
      const int bin = 64 * m + lane;
      const uint32_t c = bin < NB ? cnt[m] : 0u;
      if (bin < NB) row[bin] = (double)c / dtot;
      acc = ku_wave_terms(acc, c, dtot);
    }
    if (inv) { const double v = (double)inv / dtot; acc += v * log(v); }
    if (lane == 0) {
      row[NB] = (double)inv / dtot;
      gc_out[a] = (double)gc / (double)L;
      acc = -1 * acc;
      hsd_out[a] = pow(KU_E, acc);
    }
    __syncthreads();
  }
}

// ---- tier M: one 256-thread workgroup per allele, one LDS histogram of 4^k u32 (64 KiB at k = 7)
template <int K>
__global__ __launch_bounds__(256) void kmer_usage_block(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                        const uint32_t* __restrict__ seq_len, uint32_t n, double* __restrict__ usage,
                                                        double* __restrict__ gc_out, double* __restrict__ hsd_out)
{
  constexpr int NB = 1 << (2 * K);
  __shared__ uint32_t H[NB];
  __shared__ uint32_t red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint8_t* s = arena + seq_off[a];
    const int64_t L = seq_len[a], nwin = L >= K ? L - K + 1 : 0;
    for (int q = tid; q < NB; q += 256) H[q] = 0u;
    __syncthreads();
    uint32_t inv = 0, gc = 0;
    for (int64_t t0 = 0; t0 < L; t0 += KU_TILE_M) {
      const int64_t j0 = t0 + (int64_t)KU_SEGS * tid;
      if (j0 < L) ku_segment<K>(s, j0, nwin, L, &inv, &gc, [&](uint32_t idx) { atomicAdd(&H[idx], 1u); });
    }
    inv = ku_wave_sum(inv);
    gc = ku_wave_sum(gc);
    if (lane == 0) { red[0][wv] = inv; red[1][wv] = gc; }
    __syncthreads();
    inv = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    gc = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const int32_t total = ku_total(L, K);
    const double dtot = (double)total;
    double* row = usage + (size_t)a * (NB + 1);
    for (int q = tid; q < NB; q += 256) row[q] = (double)H[q] / dtot;
    if (wv == 0) {
      double acc = 0;
      for (int c0 = 0; c0 < NB; c0 += 64) acc = ku_wave_terms(acc, H[c0 + lane], dtot);
      if (inv) { const double v = (double)inv / dtot; acc += v * log(v); }
      if (lane == 0) {
        row[NB] = (double)inv / dtot;
        gc_out[a] = (double)gc / (double)L;
        acc = -1 * acc;
        hsd_out[a] = pow(KU_E, acc);
      }
    }
    __syncthreads();
  }
}

// ---- tier L: HBM histograms, rows of 4^k + 1 u32 (the last one the non-ACGT windows); workgroup w counts the windows of one chunk of
// KU_CHUNK_L starts of allele a, blk_first[a] <= w < blk_first[a + 1]
template <int K>
__global__ __launch_bounds__(256) void kmer_count_global(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                         const uint32_t* __restrict__ seq_len, const uint32_t* __restrict__ blk_first, uint32_t n,
                                                         uint32_t* __restrict__ hist, uint32_t* __restrict__ gc_cnt)
{
  constexpr uint32_t NB = 1u << (2 * K);
  const uint32_t w = blockIdx.x;
  uint32_t lo = 0, hi = n;                        // last a with blk_first[a] <= w
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (blk_first[mid] <= w) lo = mid; else hi = mid; }
  const uint32_t a = lo;
  const int tid = threadIdx.x;
  const uint8_t* s = arena + seq_off[a];
  const int64_t L = seq_len[a], nwin = L >= K ? L - K + 1 : 0;
  const int64_t c0 = (int64_t)(w - blk_first[a]) * KU_CHUNK_L, c1 = c0 + KU_CHUNK_L < L ? c0 + KU_CHUNK_L : L;
  uint32_t* h = hist + (size_t)a * (NB + 1);
  uint32_t inv = 0, gc = 0;
  for (int64_t t0 = c0; t0 < c1; t0 += KU_TILE_M) {
    const int64_t j0 = t0 + (int64_t)KU_SEGS * tid;
    if (j0 < c1) ku_segment<K>(s, j0, nwin, L, &inv, &gc, [&](uint32_t idx) { atomicAdd(&h[idx], 1u); });
  }
  inv = ku_wave_sum(inv);
  gc = ku_wave_sum(gc);
  if ((tid & 63) == 0) {
    if (inv) atomicAdd(&h[NB], inv);
    if (gc) atomicAdd(&gc_cnt[a], gc);
  }
}

__global__ __launch_bounds__(256) void kmer_divide_global(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ seq_len, uint32_t n,
                                                          int k, uint32_t bins, double* __restrict__ usage)
{
  for (uint32_t a = blockIdx.y; a < n; a += gridDim.y) {
    const double dtot = (double)ku_total(seq_len[a], k);
    const uint32_t* h = hist + (size_t)a * bins;
    double* row = usage + (size_t)a * bins;
    for (uint32_t b = blockIdx.x * 256 + threadIdx.x; b < bins; b += gridDim.x * 256) row[b] = (double)h[b] / dtot;
  }
}

// one wave per allele: the diversity over the bins in ascending order (lane l takes bin c0 + l + 64 j of a 1024-bin step; j outer, lane inner)
__global__ __launch_bounds__(64) void kmer_hsd_global(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ seq_len,
                                                      const uint32_t* __restrict__ gc_cnt, uint32_t n, int k, uint32_t bins,
                                                      double* __restrict__ gc_out, double* __restrict__ hsd_out)
{
  const int lane = threadIdx.x;
  for (uint32_t a = blockIdx.x; a < n; a += gridDim.x) {
    const uint32_t* h = hist + (size_t)a * bins;
    const double dtot = (double)ku_total(seq_len[a], k);
    double acc = 0;
    for (uint32_t c0 = 0; c0 < bins; c0 += 1024) {
      uint32_t c[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) { const uint32_t b = c0 + 64 * j + lane; c[j] = b < bins ? h[b] : 0u; }
#pragma unroll
      for (int j = 0; j < 16; ++j) acc = ku_wave_terms(acc, c[j], dtot);
    }
    if (lane == 0) {
      gc_out[a] = (double)gc_cnt[a] / (double)seq_len[a];
      acc = -1 * acc;
      hsd_out[a] = pow(KU_E, acc);
    }
  }
}

template <int K>
void launch_tier(otg_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_blk, uint32_t n,
                 uint32_t n_blk, double* d_usage, uint32_t* d_hist, uint32_t* d_gc, double* d_gcv, double* d_hsd)
{
  const uint32_t grid = std::min<uint32_t>(n, 1u << 20);
  if constexpr (K <= 4) {          // tiers S and M count and finish in one kernel: the epilogue time is 0
    hipLaunchKernelGGL(kmer_usage_wave<K>, dim3(grid), dim3(64), 0, ctx->stream, d_arena, d_off, d_len, n, d_usage, d_gcv, d_hsd);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
  } else if constexpr (K <= 7) {
    hipLaunchKernelGGL(kmer_usage_block<K>, dim3(grid), dim3(256), 0, ctx->stream, d_arena, d_off, d_len, n, d_usage, d_gcv, d_hsd);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
  } else {
    const uint32_t bins = (1u << (2 * K)) + 1u;
    if (n_blk) hipLaunchKernelGGL(kmer_count_global<K>, dim3(n_blk), dim3(256), 0, ctx->stream, d_arena, d_off, d_len, d_blk, n, d_hist, d_gc);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    const dim3 g(std::min<uint32_t>((bins + 255) / 256, 4096u), std::min<uint32_t>(n, 65535u));
    hipLaunchKernelGGL(kmer_divide_global, g, dim3(256), 0, ctx->stream, d_hist, d_len, n, K, bins, d_usage);
    hipLaunchKernelGGL(kmer_hsd_global, dim3(grid), dim3(64), 0, ctx->stream, d_hist, d_len, d_gc, n, K, bins, d_gcv, d_hsd);
  }
}

using LaunchFn = void (*)(otg_ctx*, const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, double*, uint32_t*,
                          uint32_t*, double*, double*);
const LaunchFn kLaunch[13] = {nullptr, launch_tier<1>, launch_tier<2>, launch_tier<3>, launch_tier<4>, launch_tier<5>, launch_tier<6>,
                              launch_tier<7>, launch_tier<8>, launch_tier<9>, launch_tier<10>, launch_tier<11>, launch_tier<12>};

// the prefix of tier L on the device: workgroups per row from the resident lengths
struct KuChunks {
  const uint32_t* len;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (len[i] + KU_CHUNK_L - 1) / KU_CHUNK_L; }
};

} // namespace

int otg_kmer_usage_fits(otg_ctx* ctx, const char* who, uint32_t n, int32_t k)
{
  const uint64_t bins = (1ull << (2 * k)) + 1;
  const uint64_t row_bytes = bins * sizeof(double) + (k >= 8 ? bins * sizeof(uint32_t) : 0);
  if ((uint64_t)n * row_bytes > KU_WORKSPACE)
    return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: %u alleles at k = %d need %llu device bytes, the workspace holds %llu (at most %llu alleles)",
                    who, n, k, (unsigned long long)(n * row_bytes), (unsigned long long)KU_WORKSPACE, (unsigned long long)(KU_WORKSPACE / row_bytes));
  return OTG_OK;
}

// The launch part of otg_kmer_usage_batch on device-resident rows: row i is rows.arena[rows.off[i] .. + rows.len[i]), and the tiers read up to 32 bytes
// past a row's last window, so the arena must extend that far past every row.  h_blk (nullable, read for k >= 8 only) is the workgroup prefix
// of tier L (n + 1 entries) where the caller has the lengths on the host; without it the prefix is scanned on the device and only its total
// read back.  The results land in SLOT_KMER_OUT (otg_kmer_usage_device_results); the caller has checked otg_kmer_usage_fits.
int otg_kmer_usage_resident(otg_ctx* ctx, const char* who, const OtgRows& rows, const uint32_t* h_blk, uint32_t n, int32_t k, double* usage_out,
                            double* gc_out, double* hsd_out)
{
  ctx->last_kmer_count_ms = ctx->last_kmer_epi_ms = 0.0;
  if (n == 0) return OTG_OK;
  const uint64_t bins = (1ull << (2 * k)) + 1;
  const bool tier_l = k >= 8;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->ev2) HIP_TRY(ctx, hipEventCreate(&ctx->ev2));
  // tier L: gc counts (u32) | workgroup prefix (u32, n + 1) | their u64 total
  uint64_t acc = tier_l && h_blk ? h_blk[n] : 0;
  const size_t blk_words = ((size_t)2 * n + 2) & ~(size_t)1;              // the total behind them is 8-byte aligned
  const size_t usage_bytes = (size_t)n * bins * sizeof(double);
  uint8_t* d_out = (uint8_t*)otg_slot(ctx, SLOT_KMER_OUT, usage_bytes + (size_t)n * 2 * sizeof(double));   // usage rows | gc | hsd
  uint32_t* d_hist = tier_l ? (uint32_t*)otg_slot(ctx, SLOT_KMER_HIST, (size_t)n * bins * sizeof(uint32_t)) : nullptr;
  uint32_t* d_gc = tier_l ? (uint32_t*)otg_slot(ctx, SLOT_KMER_BLK, blk_words * 4 + 8) : nullptr;
  if (!d_out || (tier_l && (!d_hist || !d_gc))) return OTG_ERR_HIP;
  uint32_t* d_blk = tier_l ? d_gc + n : nullptr;
  double* d_usage = (double*)d_out;
  double* d_gcv = (double*)(d_out + usage_bytes);
  double* d_hsd = d_gcv + n;
  if (tier_l) {
    if (h_blk) HIP_TRY(ctx, hipMemcpyAsync(d_blk, h_blk, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    else {
      uint64_t* d_total = (uint64_t*)(d_gc + blk_words);
      hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint32_t, KuChunks>), dim3(1), dim3(1024), 0, ctx->stream, KuChunks{rows.len}, n, d_blk, d_total);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&acc, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      if (acc > 0x7fffffffull) return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: the batch needs %llu workgroups", who, (unsigned long long)acc);
    }
    HIP_TRY(ctx, hipMemsetAsync(d_gc, 0, (size_t)n * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t)n * bins * sizeof(uint32_t), ctx->stream));
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  kLaunch[k](ctx, rows.arena, rows.off, rows.len, d_blk, n, (uint32_t)acc, d_usage, d_hist, d_gc, d_gcv, d_hsd);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  if (usage_out) HIP_TRY(ctx, hipMemcpyAsync(usage_out, d_usage, usage_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (gc_out) HIP_TRY(ctx, hipMemcpyAsync(gc_out, d_gcv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (hsd_out) HIP_TRY(ctx, hipMemcpyAsync(hsd_out, d_hsd, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float c_ms = 0.f, e_ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&c_ms, ctx->ev0, ctx->ev1));
  HIP_TRY(ctx, hipEventElapsedTime(&e_ms, ctx->ev1, ctx->ev2));
  ctx->last_kmer_count_ms = c_ms; ctx->last_kmer_epi_ms = e_ms;
  return OTG_OK;
}

extern "C" int otg_kmer_usage_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const uint64_t* seq_off, const uint32_t* seq_len,
                                    uint32_t n, int32_t k, double* usage_out, double* gc_out, double* hsd_out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_kmer_usage_batch: no context (no HIP device?)");
  if (k < 1 || k > OTG_KMER_MAX) return otg_fail(ctx, OTG_ERR_ARG, "otg_kmer_usage_batch: k = %d outside 1..%d", k, OTG_KMER_MAX);
  if (int rc = otg_rows_check(ctx, "otg_kmer_usage_batch", seq_arena, arena_bytes, seq_off, seq_len, n, nullptr)) return rc;
  if (int rc = otg_kmer_usage_fits(ctx, "otg_kmer_usage_batch", n, k)) return rc;
  ctx->last_kmer_count_ms = ctx->last_kmer_epi_ms = 0.0;
  if (n == 0) return OTG_OK;
  // tier L: the workgroup prefix from the host lengths, refused before anything is allocated
  std::vector<uint32_t> blk(k >= 8 ? n + 1 : 0);
  if (k >= 8) {
    uint64_t acc = 0;
    for (uint32_t i = 0; i < n; ++i) { blk[i] = (uint32_t)acc; acc += (seq_len[i] + KU_CHUNK_L - 1) / KU_CHUNK_L; }
    if (acc > 0x7fffffffull) return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_kmer_usage_batch: the batch needs %llu workgroups", (unsigned long long)acc);
    blk[n] = (uint32_t)acc;
  }
  OtgRows rows;
  if (int rc = otg_rows_upload(ctx, SLOT_KMER_SEQ, SLOT_KMER_META, seq_arena, arena_bytes, seq_off, seq_len, n, &rows)) return rc;
  return otg_kmer_usage_resident(ctx, "otg_kmer_usage_batch", rows, k >= 8 ? blk.data() : nullptr, n, k, usage_out, gc_out, hsd_out);
}

extern "C" int otg_kmer_usage_device_results(otg_ctx* ctx, uint32_t n, int32_t k, const double** usage, const double** gc, const double** hsd)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_kmer_usage_device_results: NULL context");
  if (k < 1 || k > OTG_KMER_MAX) return otg_fail(ctx, OTG_ERR_ARG, "otg_kmer_usage_device_results: k = %d outside 1..%d", k, OTG_KMER_MAX);
  const size_t usage_bytes = (size_t)n * ((1ull << (2 * k)) + 1) * sizeof(double);
  const DevBuf& b = ctx->pool[SLOT_KMER_OUT];
  if (!b.p || b.cap < usage_bytes + (size_t)n * 2 * sizeof(double))
    return otg_fail(ctx, OTG_ERR_ARG, "otg_kmer_usage_device_results: no results of %u alleles at k = %d on this context", n, k);
  if (usage) *usage = (const double*)b.p;
  if (gc) *gc = (const double*)((const uint8_t*)b.p + usage_bytes);
  if (hsd) *hsd = (const double*)((const uint8_t*)b.p + usage_bytes) + n;
  return OTG_OK;
}

extern "C" int otg_kmer_usage_last_ms(otg_ctx* ctx, double* count_ms, double* epilogue_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_kmer_usage_last_ms: NULL context");
  if (count_ms) *count_ms = ctx->last_kmer_count_ms;
  if (epilogue_ms) *epilogue_ms = ctx->last_kmer_epi_ms;
  return OTG_OK;
}

// otg_scan.hpp — the one-block exclusive scan of the cohort regroup (cohort.hip) and of the resident k-mer rows (kmer_usage.hip), and the
// several-scans-in-one-launch kernel of the pipeline's compaction and of the consensus plan (pipeline.hip, poa.hip).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
// the plain input of a scan: in(i) = p[i]
template <class T>
struct OtgScanPtr {
  const T* p;
  __device__ __forceinline__ T operator()(uint32_t i) const { return p[i]; }
};

// Exclusive scan of the n values in(0) .. in(n - 1) into n + 1 (out[n] = the total), summed in Tacc and stored as Tout; *total (nullable)
// receives the unconverted sum.  One block; every thread owns ITEMS consecutive values of a tile, the thread sums are scanned in LDS.  The
// tables are a few thousand regions / some ten thousand alleles: one block is enough.
template <class Tacc, class Tout, class In>
__global__ void __launch_bounds__(1024) otg_scan_kernel(In in, uint32_t n, Tout* __restrict__ out, Tacc* __restrict__ total)
{
  constexpr uint32_t ITEMS = 8, T = 1024;
  __shared__ Tacc part[T];
  __shared__ Tacc carry_s;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += ITEMS * T) {
    Tacc v[ITEMS];
    Tacc sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; ++k) {
      const uint32_t i = base + t * ITEMS + k;
      v[k] = i < n ? (Tacc)in(i) : (Tacc)0;
      sum += v[k];
    }
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {
      const Tacc add = t >= d ? part[t - d] : (Tacc)0;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    Tacc run = carry_s + part[t] - sum;
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; ++k) {
      const uint32_t i = base + t * ITEMS + k;
      if (i < n) out[i] = (Tout)run;
      run += v[k];
    }
    __syncthreads();
    if (t == T - 1) carry_s += part[t];
    __syncthreads();
  }
  if (t == 0) {
    out[n] = (Tout)carry_s;
    if (total) *total = carry_s;
  }
}

// Several exclusive scans in ONE launch, one block per scan (pipeline.hip: the two compaction scans of a run; poa.hip: the capacity offsets of
// the consensus plan).  The values are uint32 or uint64 and are summed and stored as uint64.  With an index list the scan runs over a list:
// value k is in[idx[first + k]] and its prefix goes to out[idx[first + k]] (the running sums of a launch list, scattered to the graphs).
struct OtgScanJob {
  const void* in = nullptr;
  const uint32_t* idx = nullptr;         // nullable
  const uint32_t* first_ptr = nullptr;   // nullable: where the list begins in idx (device word)
  const uint32_t* n_ptr = nullptr;       // nullable: the count is this device word, not n
  uint64_t* out = nullptr;
  uint64_t* total = nullptr;             // nullable
  uint32_t n = 0;
  uint32_t in_u64 = 0;                   // the values are uint64
  uint32_t write_end = 0;                // out[n] = the total (plain scans only)
};
constexpr uint32_t OTG_SCAN_MAX_JOBS = 8;
struct OtgScanJobs { OtgScanJob j[OTG_SCAN_MAX_JOBS]; };

// grid = number of jobs.  A tile is 1024 threads x ITEMS consecutive values (coalesced: a wave reads 64 x ITEMS consecutive values); the thread
// sums are scanned by lane shifts inside a wave and across the 16 waves through LDS, and the block carries the prefix from tile to tile.
template <uint32_t ITEMS>
__global__ void __launch_bounds__(1024) otg_scan_jobs_kernel(OtgScanJobs J)
{
  constexpr uint32_t T = 1024;
  __shared__ uint64_t wave_sum[T / 64];
  const OtgScanJob& job = J.j[blockIdx.x];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t n = job.n_ptr ? *job.n_ptr : job.n;
  const uint32_t* idx = job.idx ? job.idx + (job.first_ptr ? *job.first_ptr : 0u) : nullptr;
  const uint32_t* in32 = (const uint32_t*)job.in;
  const uint64_t* in64 = (const uint64_t*)job.in;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < n; base += ITEMS * T) {
    uint64_t v[ITEMS];
    uint32_t at[ITEMS];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; ++k) {
      const uint32_t i = base + t * ITEMS + k;
      at[k] = i < n ? (idx ? idx[i] : i) : 0u;
      v[k] = i < n ? (job.in_u64 ? in64[at[k]] : (uint64_t)in32[at[k]]) : 0ull;
      sum += v[k];
    }
    uint64_t x = sum;                      // inclusive over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint64_t y = __shfl_up(x, d); if (lane >= d) x += y; }
    if (lane == 63) wave_sum[wv] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64; ++w) { const uint64_t s = wave_sum[w]; if (w < wv) before += s; all += s; }
    uint64_t run = carry + before + x - sum;
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; ++k) {
      const uint32_t i = base + t * ITEMS + k;
      if (i < n) job.out[at[k]] = run;
      run += v[k];
    }
    carry += all;
    __syncthreads();
  }
  if (t == 0) {
    if (job.write_end) job.out[n] = carry;
    if (job.total) *job.total = carry;
  }
}
#endif

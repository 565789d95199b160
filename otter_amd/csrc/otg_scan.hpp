// otg_scan.hpp — the one-block exclusive scan of the cohort regroup (cohort.hip) and of the resident k-mer rows (kmer_usage.hip).
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
#endif

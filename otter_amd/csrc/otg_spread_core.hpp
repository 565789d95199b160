// otg_spread_core.hpp — the order statistics of the spread operator (include/otter_gpu.h states the rule): the five quantiles of the members'
// values of one allele, found by selection, not by sorting, so that no buffer caps the depth of a region.
//
// Shared by spread.hip (device) and tests/spread_core_host.cpp (host), which runs the same functions in the kernel's schedule: a wave of 64
// lanes walks the region's reads 64 at a time ("strides"); a lane holds the value of its read of the stride, or SP_ABSENT when that read is
// no member.  The wave W supplies the one cross-lane operation that is needed:
//   W::Vec                          what a wave holds per stride: one uint32_t per lane (device: the lane's own register; host: 64 of them)
//   w.count_le(Vec v, uint32_t x)   how many lanes hold a value <= x, the same number in every lane (device: ballot and popcount)
//
// Selection.  The values are below 2^SP_BITS.  The k-th smallest (k from 0) is the smallest x with #{v <= x} > k; its bits are found from
// the highest down: with the bits above b decided as x, every value that agrees with them and has bit b clear is <= x | (2^b - 1), so bit b
// of the answer is clear exactly when #{v <= x | (2^b - 1)} > k.  SP_BITS counting passes over the strides per statistic, O(m) each; a value
// is never moved, so ties need no care, and SP_ABSENT (all ones) is above every candidate and is never counted.
//
// Two sources of the strides.  While the region has at most SP_REG_STRIDES strides the values stay in registers, one stride per register,
// and a pass is SP_REG_STRIDES compares and ballots; above that a pass asks the caller's loader for every stride again (the kernel re-reads
// the records, which are L2-resident at these sizes) and serves all five statistics from one load.  Both run the same bit loop.
#pragma once
#include <cstdint>
#include "../../include/otter_gpu.h"

#if defined(__HIPCC__)
#define OTG_SP_HD __host__ __device__ __forceinline__
#else
#define OTG_SP_HD inline
#endif

namespace otg_spread_core {

constexpr int SP_BITS = 21;                         // values are unit bases of a row of at most OTG_LOCUS_MAX_LEN bases
constexpr int SP_REG_STRIDES = 4;                   // R: regions of up to 64 R reads keep their values in registers
constexpr uint32_t SP_ABSENT = 0xffffffffu;         // the lane's read is no member
static_assert(2u * (uint32_t)OTG_LOCUS_MAX_LEN < (1u << SP_BITS), "unit_bases of a row (at most its length plus its edits) must stay below 2^SP_BITS");

// the index of quantile j of m >= 1 sorted members: floor(j (m - 1) / 4)
OTG_SP_HD uint32_t sp_rank(uint32_t j, uint32_t m) { return (uint32_t)(((uint64_t)j * (m - 1u)) >> 2); }

// the k-th smallest (k from 0, k < the number of members) of the values in v[0 .. R)
template <typename W, int R> OTG_SP_HD uint32_t sp_select_reg(const W& w, const typename W::Vec (&v)[R], uint32_t k)
{
  uint32_t x = 0u;
  for (int b = SP_BITS - 1; b >= 0; --b) {
    const uint32_t cand = x | ((1u << b) - 1u);
    uint32_t c = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 0; s < R; ++s) c += w.count_le(v[s], cand);
    if (c <= k) x |= 1u << b;
  }
  return x;
}

// the five quantiles of m members; m = 0 gives zeros
template <typename W, int R> OTG_SP_HD void sp_quantiles_reg(const W& w, const typename W::Vec (&v)[R], uint32_t m, uint32_t (&q)[5])
{
  for (uint32_t j = 0; j < 5u; ++j) q[j] = m ? sp_select_reg<W, R>(w, v, sp_rank(j, m)) : 0u;
}
// the same over n_strides strides that load(s) -> W::Vec gives anew on every pass, the five bit loops side by side: a stride is loaded once
// per bit, not once per bit and statistic
template <typename W, typename Load> OTG_SP_HD void sp_quantiles_load(const W& w, Load& load, uint32_t n_strides, uint32_t m, uint32_t (&q)[5])
{
  uint32_t k[5];
  for (int j = 0; j < 5; ++j) { q[j] = 0u; k[j] = m ? sp_rank((uint32_t)j, m) : 0u; }
  if (m == 0u) return;
  for (int b = SP_BITS - 1; b >= 0; --b) {
    uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t s = 0; s < n_strides; ++s) {
      const typename W::Vec v = load(s);
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int j = 0; j < 5; ++j) c[j] += w.count_le(v, q[j] | ((1u << b) - 1u));
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 5; ++j)
      if (c[j] <= k[j]) q[j] |= 1u << b;
  }
}

} // namespace otg_spread_core

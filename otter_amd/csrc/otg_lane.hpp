// otg_lane.hpp — the lane exchanges of the kernels that keep a DP row across the lanes of a wave (unitalign.hip, unitparse.hip, tract.hip), for keys of
// 32 and 64 bits: a value from any lane (ds_bpermute), from D lanes below inside a row of 16 (DPP), one register of a lane's few by a
// runtime index, and the step of the segmented prefix minimum built on them.  Device code only.
#pragma once
#include <cstdint>
#include "otg_unitalign_core.hpp"

namespace otg_lane {

__device__ __forceinline__ uint32_t from_lane(uint32_t x, uint32_t src) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)x); }
__device__ __forceinline__ uint64_t from_lane(uint64_t x, uint32_t src)
{
  return ((uint64_t)from_lane((uint32_t)(x >> 32), src) << 32) | from_lane((uint32_t)x, src);
}
// the value D lanes below inside a row of 16 (DPP row_shr); a lane without such a source keeps its own
template <int D> __device__ __forceinline__ uint32_t row_up(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x110 + D, 0xf, 0xf, false); }
template <int D> __device__ __forceinline__ uint64_t row_up(uint64_t x)
{
  return ((uint64_t)row_up<D>((uint32_t)(x >> 32)) << 32) | row_up<D>((uint32_t)x);
}
template <typename K, int R> __device__ __forceinline__ K pick(const K (&v)[R], uint32_t r)
{
  K x = v[0];
#pragma unroll
  for (int q = 1; q < R; ++q) x = r == (uint32_t)q ? v[q] : x;
  return x;
}
// one step of the segmented prefix minimum (MAX: maximum) over lanes, distance D < S: pos = the lane's place inside its segment of at most S lanes
template <typename K, int S, int D, bool MAX = false> __device__ __forceinline__ K scan_step(K x, uint32_t lane, uint32_t pos)
{
  if constexpr (D < S) {
    K from;
    if constexpr (S <= 16) from = row_up<D>(x);
    else from = from_lane(x, lane - D);                            // (lane < D reads a lane of the wave that `ok` discards)
    return otg_unitalign_core::ua_scan_take<K, MAX>(x, from, pos >= (uint32_t)D);
  } else {
    return x;
  }
}

} // namespace otg_lane

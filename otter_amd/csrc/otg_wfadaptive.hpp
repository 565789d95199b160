// otg_wfadaptive.hpp — the cut of WFA2-lib's adaptive wavefront reduction, wf_heuristic_wfadaptive(min_wavefront_length,
// max_distance_threshold, steps_between_cutoffs), shared by the kernels that run under it: the score chains (wfa_adaptive.hip, where the
// semantics are written out) and the provenance pass of the edit op strings (edit_align.hip).
#pragma once
#include "wfa_affine_common.hpp"

namespace otg_adaptive {

using otg_affine::imax;
using otg_affine::imin;

constexpr int BIG = 1 << 30;

struct Heur { int min_wf_len, max_dist, steps; };

// what is left to align from offset h of diagonal k (the distance the cut compares)
__device__ __forceinline__ int left_to_align(int h, int k, int pl, int tl, bool ef, int pef, int tef)
{
  if (h < 0) return BIG;
  const int lv = pl - (h - k), lh = tl - h;
  if (!ef) return imax(lv, lh);
  return imin(imax(lh, lv - pef), imax(lv, lh - tef));
}

// The cut.  [lo, hi] = range of the extended M wavefront, mind = smallest left_to_align over it, off(k) = offset of diagonal k (called
// for lo <= k <= hi only).  Wave-uniform control flow; returns the trimmed range in lo / hi.
template <class Off>
__device__ __forceinline__ void wfadaptive_cut(const Heur& H, int& steps_wait, int mind, int pl, int tl, bool ef, int pef, int tef,
                                               int& lo, int& hi, int lane, Off off)
{
  --steps_wait;
  if (steps_wait > 0) return;
  if (hi - lo + 1 < H.min_wf_len) return;
  const int kend = tl - pl;
  const int min_k = ef ? kend - tef : kend, max_k = ef ? kend + pef : kend;
  const int top_limit = imin(min_k - 1, hi);
  int nlo = lo;
  if (top_limit > lo) {
    nlo = top_limit;
    for (int c = lo; c < top_limit; c += 64) {
      const int k = c + lane;
      bool ok = false;
      if (k < top_limit) ok = left_to_align(off(k), k, pl, tl, ef, pef, tef) - mind <= H.max_dist;
      const unsigned long long b = __ballot(ok);
      if (b) { nlo = c + (int)__builtin_ctzll(b); break; }
    }
  }
  const int bottom_limit = imax(max_k + 1, nlo);
  int nhi = hi;
  if (hi > bottom_limit) {
    nhi = bottom_limit;
    for (int c = hi; c > bottom_limit; c -= 64) {
      const int k = c - 63 + lane;                      // this chunk covers [c - 63, c]
      bool ok = false;
      if (k > bottom_limit) ok = left_to_align(off(k), k, pl, tl, ef, pef, tef) - mind <= H.max_dist;
      const unsigned long long b = __ballot(ok);
      if (b) { nhi = c - (int)__builtin_clzll(b); break; }
    }
  }
  lo = nlo; hi = nhi;
  steps_wait = H.steps;
}

// The same cut with both ends looked at in ONE step (the fast tiers): lanes 0-31 hold the 32 lowest diagonals of the range, lanes 32-63 the 32
// highest; one offset read, one distance, one ballot.  A scan that would have to look further than 32 diagonals from an end — nothing in range
// among them and the limit not reached — falls back to the general form above (same result by construction: both implement "first diagonal
// from the end within the threshold, but not past the limit").
template <class Off>
__device__ __forceinline__ void wfadaptive_cut32(const Heur& H, int& steps_wait, int mind, int pl, int tl, bool ef, int pef, int tef,
                                                 int& lo, int& hi, int lane, Off off)
{
  if (steps_wait - 1 > 0 || hi - lo + 1 < H.min_wf_len) { wfadaptive_cut(H, steps_wait, mind, pl, tl, ef, pef, tef, lo, hi, lane, off); return; }
  const int kend = tl - pl;
  const int min_k = ef ? kend - tef : kend, max_k = ef ? kend + pef : kend;
  const int top_limit = imin(min_k - 1, hi);
  const bool low = lane < 32;
  const int k = low ? lo + lane : hi - 63 + lane;
  bool ok = false;
  if (k >= lo && k <= hi) ok = left_to_align(off(k), k, pl, tl, ef, pef, tef) - mind <= H.max_dist;
  const unsigned long long b = __ballot(ok);
  // low end: the first diagonal in [lo, top_limit) within the threshold, else top_limit
  int nlo = lo;
  bool fallback = false;
  if (top_limit > lo) {
    const int n = top_limit - lo;                                  // candidates lo .. top_limit - 1
    const uint32_t cand = (uint32_t)b & (n >= 32 ? 0xffffffffu : ((1u << n) - 1u));
    if (cand) nlo = lo + (int)__builtin_ctz(cand);
    else if (n <= 32) nlo = top_limit;
    else fallback = true;
  }
  int nhi = hi;
  if (!fallback) {
    const int bottom_limit = imax(max_k + 1, nlo);
    if (hi > bottom_limit) {
      const int n = hi - bottom_limit;                             // candidates bottom_limit + 1 .. hi = the top n bits
      const uint32_t hb = (uint32_t)(b >> 32);
      const uint32_t cand = hb & (n >= 32 ? 0xffffffffu : ~((1u << (32 - n)) - 1u));
      if (cand) nhi = hi - (int)__builtin_clz(cand);
      else if (n <= 32) nhi = bottom_limit;
      else fallback = true;
    }
  }
  if (fallback) { wfadaptive_cut(H, steps_wait, mind, pl, tl, ef, pef, tef, lo, hi, lane, off); return; }
  lo = nlo; hi = nhi;
  steps_wait = H.steps;
}

} // namespace otg_adaptive

// affine_score_range.hpp — which diagonals a score of the gap-affine wavefront can reach, in closed form (penalties (2,4,1) after gcd
// reduction: mismatch 2, gap open + extension 4, gap extension 1).  Shared by the register tiers (wfa_affine_reg.hip) and a host check
// (tests/affine_score_range_host.cpp), so it includes nothing of the device headers.
//
// The range of a score follows from the ranges of the scores 2 and 4 below it (mismatch, gap open: the latter widened by one diagonal per
// side) and of the score below it (gap extension, widened likewise) — no cell value enters.  Unrolled: score 0 spans the start diagonals
// [lo0, hi0]; nothing costs 1; score 2 is score 0 again (a mismatch), and from there every score widens the span by one diagonal per side,
// first through the gap of no bases that score 3 = 4 - 1 stands for in this bookkeeping, then through extensions.  The span is clamped to
// [-pl, tl] and clipped to the diamond of cells that can still end within the bound U: a cell of score s on diagonal k needs
// dist(k, [elo, ehi]) <= U - s.
#pragma once

#if defined(__HIPCC__)
#define OTG_RANGE_HD __host__ __device__ __forceinline__
#else
#define OTG_RANGE_HD inline
#endif

namespace otg_affine {

enum { RANGE_FAIL = -1, RANGE_EMPTY = 0, RANGE_OK = 1 };

// [*lo, *hi] of score s >= 0.  RANGE_OK: the range; RANGE_EMPTY: the score is unreachable (score 1, and nothing else while hi0 >= lo0 lie
// within [-pl, tl]); RANGE_FAIL: the bound is used up (U < s) or the diamond has clipped the range away — no alignment of score <= U.
OTG_RANGE_HD int affine_score_range(int s, int lo0, int hi0, int pl, int tl, int U, int elo, int ehi, int* lo, int* hi)
{
  if (s == 0) { *lo = lo0; *hi = hi0; return hi0 >= lo0 ? RANGE_OK : RANGE_FAIL; }     // (no start diagonal: affine_window refuses such a task before any tier sees it)
  if (s == 1) { *lo = 1; *hi = 0; return RANGE_EMPTY; }
  const int g = s - 2;
  int l = lo0 - g, h = hi0 + g;
  if (l < -pl) l = -pl;
  if (h > tl) h = tl;
  if (h >= l) {
    const int room = U - s;
    const int dl = elo - room, dh = ehi + room;
    if (l < dl) l = dl;
    if (h > dh) h = dh;
    if (room < 0 || h < l) return RANGE_FAIL;
  }
  *lo = l; *hi = h;
  return h >= l ? RANGE_OK : RANGE_EMPTY;
}

} // namespace otg_affine

// otg_locus_core.hpp — the per-lane arithmetic of the locus mode (include/otter_gpu.h states the rule): the local wraparound alignment over a
// unit set that finds the repeat inside a flanked allele.  The key, the cell step, the biased prefix maximum and the order of the best cell
// are the tract mode's (otg_tract_core.hpp); the lanes of a unit set and its classes are the joint parse's (otg_unitparse_core.hpp).  What
// is new here is the join of the units at phase 0: the switch step closed together with the skipped unit bases in one pass per row.
//
// Shared by locus.hip (device) and tests/locus_core_host.cpp (host), which runs the same functions in the kernel's schedule (64 lanes in
// lockstep, units at lane boundaries, the exchanges done by indexing) against the plain restatement of the rule.
//
// The closed form of a row.  Per unit k, with T the cells after the diagonal step, the outside base and the fresh start, I = indel:
//   H1_k[j]  = max over q <= j of T_k[q] - (j - q) I          the biased prefix maximum of otg_tract_core.hpp, inside the unit
//   cand0_k  = max(H1_k[0], H1_k[p_k - 1] - I)                what reaches phase 0 from inside the unit
//   best0    = max over k of cand0_k                          one maximum over the task's lanes
//   entry_k  = max(H1_k[p_k - 1] - I, best0)                  what enters phase 0 from behind: the unit's own wrap, or a switch (free)
//   V_k[j]   = max(H1_k[j], entry_k - j I)                    the way on around the unit
// every subtraction saturating (tr_sub).  A value that enters a unit by a switch and walks round to p - 1 and back to phase 0 has lost p I,
// so it never improves best0: one pass is the fixed point of the skip and the switch steps taken together.  For one unit entry - j I is
// the wrap term of tr_close, so K = 1 gives the tract mode's cells.
//
// The narrow key (score * 2^16 + begin).  While row i + 1 is built from row i (i < L) a lane of unit k holds at most, field by field (score,
// begin), with match = M, indel = I and p_max the largest unit of the set:
//   a cell of row i, the fresh start, the diagonal candidate   (M (i + 1), i + 1)      as in otg_tract_core.hpp
//   the cell plus its scan bias j I, j < p_k                   (M (i + 1) + (p_k - 1) I, i + 1)
//   H1, its last position, cand0                               at most a cell of row i + 1: the scanned cell less its own bias, then only
//                                                              maxima of such values and saturating subtractions
//   best0, the entry                                           a maximum over lanes of cand0: a cell of row i + 1 of some unit
//   the entry less j I, the closed cell, the running best      at most a cell of row i + 1
// The largest are M L + (p_max - 1) I in the score field and L in the begin field.  Both stay below 2^16 while L <= tr_narrow_len(q, p_max):
// no field carries into the other up to that length, so the narrow and the wide tier order every pair of keys alike.  The wide key (32 / 32)
// holds every admitted task: 16 * OTG_LOCUS_MAX_LEN + 255 * 64 < 2^32.
#pragma once
#include <cstdint>
#include "otg_tract_core.hpp"
#include "otg_unitparse_core.hpp"

namespace otg_locus_core {

using namespace otg_tract_core;
using otg_unitalign_core::ua_class_lanes;
using otg_unitalign_core::ua_class_regs;
using otg_unitalign_core::ua_scan_take;
using otg_unitalign_core::ua_unit_key;
using otg_unitparse_core::up_class;
using otg_unitparse_core::UP_CLASSES;
using otg_unitparse_core::UP_NO_CLASS;

static_assert(OTG_LOCUS_MAX_LEN == OTG_UNITPARSE_MAX_LEN && OTG_LOCUS_MAX_LEN <= OTG_TRACT_MAX_LEN, "the cap is the smaller of the two passes'");
static_assert(16ull * OTG_LOCUS_MAX_LEN + 255ull * 64ull < (1ull << 32), "a wide key field would carry");
static_assert((65535u - 255u * 64u) / 16u >= 1u, "the narrow bound would vanish at the largest scores");

// the largest unit of a set
OTG_UA_HD uint32_t lc_pmax(const uint32_t* p, uint32_t K)
{
  uint32_t m = 1u;
  for (uint32_t k = 0; k < K; ++k) m = p[k] > m ? p[k] : m;
  return m;
}
// the longest allele of the narrow key for these scores and this unit set
OTG_UA_HD uint32_t lc_narrow_len(const otg_tract_params& q, const uint32_t* p, uint32_t K) { return tr_narrow_len(q, lc_pmax(p, K)); }
// the class of a unit set; seg64: every task takes a whole wave
OTG_UA_HD uint32_t lc_class(const uint32_t* p, uint32_t K, bool seg64)
{
  const uint32_t c = up_class(p, K);
  return seg64 && c < 4u ? 4u : c;
}

// ---- the join, per row.  h0 = H1[0] of the lane's unit (at its first lane), last = H1[p - 1] of the lane's unit, g = indel as a key difference
template <typename K> OTG_UA_HD K lc_wrap(K last, K g) { return tr_sub<K>(last, g); }
template <typename K> OTG_UA_HD K lc_cand0(K h0, K last, K g) { return tr_max<K>(h0, lc_wrap<K>(last, g)); }
template <typename K> OTG_UA_HD K lc_entry(K last, K best0, K g) { return tr_max<K>(lc_wrap<K>(last, g), best0); }
// m = the scanned biased cell of position j, bias = j I
template <typename K> OTG_UA_HD K lc_close(K m, K bias, K entry) { return tr_max<K>(m - bias, tr_sub<K>(entry, bias)); }

} // namespace otg_locus_core

// otg_unitset_core.hpp — the per-candidate and per-class arithmetic of the unit-set discovery (include/otter_gpu.h states the rule): the
// smallest rotation of a unit by a tournament over rotation starts, the hash of the rotated codes, the class table with its compare on a
// hash match, the key that elects a class's representative, the rank order, the redundancy test and the selection under the lane budget.
//
// Shared by unitset.hip (device) and tests/unitset_core_host.cpp (host), which runs the same functions in the kernels' schedule (64 lanes
// with strided rotation starts and a butterfly, the table filled in any order, sixteen rounds of selection) against the plain restatement
// of the rule.
//
// A candidate is a repeat segment of period p <= OTG_UNITALIGN_MAX_UNIT; its unit is the p bases at arena position pos.  A class is the
// set of candidates whose units have the same smallest rotation.  The table holds, per slot, the index (+ 1) of the candidate that claimed
// it: one compare-and-swap claims and publishes at once, since everything else about that candidate already lies in the candidate list.
#pragma once
#include <cstdint>
#include "../../include/otter_gpu.h"
#include "otg_motif_core.hpp"

#define OTG_US_HD OTG_MOTIF_HD

namespace otg_unitset_core {

using otg_motif_core::mo_code;
using otg_motif_core::mo_rot_less;

static_assert(OTG_UNITSET_TOP == 16 && OTG_UNITSET_TOP * (OTG_UNITSET_TOP - 1) / 2 == 120, "the pair list of a group");
static_assert(OTG_REPEAT_MAX_LEN < (1u << 20), "a segment's length and begin (of the repeat parse) take 20 bits each of the representative's key");
static_assert(OTG_UNITALIGN_MAX_LEN < (1u << 20), "the doubled representative is a row of the unit alignment");

constexpr uint32_t US_NONE = 0xffffffffu;                       // no rotation start, no slot, no class
constexpr uint32_t US_FRESH = 0x80000000u;                      // us_table_insert: this candidate claimed the slot
constexpr uint32_t US_SMALL_SEGS = 64;                          // groups of up to this many segments vote in one wave
constexpr uint32_t US_SLOTS_SMALL = 128, US_SLOTS_BIG = 2560;   // table slots of the two vote kernels: 2 x and 1.25 x the classes they admit
static_assert(US_SLOTS_BIG > OTG_UNITSET_MAX_CLASSES && US_SLOTS_SMALL >= 2 * US_SMALL_SEGS, "the table fills only after the class cap");

struct UsCand {
  uint64_t hash;                 // of the smallest rotation's codes, truncated to the process's hash bits
  uint64_t pos;                  // arena position of the unit as the segment wrote it
  uint32_t p;                    // 0: not a candidate (a literal, a period over the cap)
  uint32_t rot;                  // the start of the smallest rotation
  uint32_t length, allele, begin, pad;
};

// one ranked class of a group
struct UsEntry {
  uint64_t weight;
  uint64_t pos;                  // of the representative
  uint32_t segments, p;
};

OTG_US_HD bool us_params_ok(const otg_unitset_params& q)
{
  return q.min_bases >= 1u && q.min_bases <= (1u << 24) && q.min_permille <= 1000u && q.redundant_permille <= 1000u && q.reserved == 0u;
}

// ---- the smallest rotation.  c = the p codes of the unit.  The smaller of two starts (US_NONE: no start); equal rotations go to the smaller
// start, so the pick is symmetric and a butterfly leaves every lane with the same answer
OTG_US_HD uint32_t us_rot_pick(const uint8_t* c, uint32_t p, uint32_t a, uint32_t b)
{
  if (a == US_NONE) return b;
  if (b == US_NONE) return a;
  return mo_rot_less(c, p, b, a) ? b : a;
}
// the best of the starts lane, lane + 64, ...
OTG_US_HD uint32_t us_rot_lane(const uint8_t* c, uint32_t p, uint32_t lane)
{
  uint32_t best = US_NONE;
  for (uint32_t r = lane; r < p; r += 64u) best = us_rot_pick(c, p, best, r);
  return best;
}

// FNV-1a over the rotated codes and the length, the low `bits` bits of it
OTG_US_HD uint64_t us_hash(const uint8_t* c, uint32_t p, uint32_t rot, uint32_t bits)
{
  uint64_t h = 0xcbf29ce484222325ull;
  uint32_t j = rot;
  for (uint32_t k = 0; k < p; ++k) {
    h = (h ^ (uint64_t)(c[j] + 1u)) * 0x100000001b3ull;
    if (++j == p) j = 0;
  }
  h = (h ^ (uint64_t)p) * 0x100000001b3ull;
  h ^= h >> 29;
  return bits >= 64u ? h : (h & ((1ull << bits) - 1ull));
}

OTG_US_HD uint32_t us_slot(uint64_t hash, uint32_t p, uint32_t ns)
{
  uint64_t x = (hash ^ ((uint64_t)p << 40)) * 0x9e3779b97f4a7c15ull;
  x ^= x >> 32;
  return (uint32_t)(x % ns);
}

// do two units of length p have the same smallest rotation?  (rotation starts ra, rb; the bases at arena positions a, b)
OTG_US_HD bool us_same_rotation(const uint8_t* arena, uint64_t a, uint32_t ra, uint64_t b, uint32_t rb, uint32_t p)
{
  uint32_t ia = ra, ib = rb;
  for (uint32_t k = 0; k < p; ++k) {
    if (mo_code(arena[a + ia]) != mo_code(arena[b + ib])) return false;
    if (++ia == p) ia = 0;
    if (++ib == p) ib = 0;
  }
  return true;
}
// is the smallest rotation of a (length p) smaller than that of b (same length), code by code?
OTG_US_HD bool us_rotation_less(const uint8_t* arena, uint64_t a, uint32_t ra, uint64_t b, uint32_t rb, uint32_t p)
{
  uint32_t ia = ra, ib = rb;
  for (uint32_t k = 0; k < p; ++k) {
    const uint32_t ca = mo_code(arena[a + ia]), cb = mo_code(arena[b + ib]);
    if (ca != cb) return ca < cb;
    if (++ia == p) ia = 0;
    if (++ib == p) ib = 0;
  }
  return false;
}

// ---- the class table.  slots[h] = 0 or 1 + the index (within cands) of the candidate that claimed slot h.  cas(ptr, expected, desired)
// returns the old word.  Returns the slot of candidate i's class, with US_FRESH set when i claimed it, or US_NONE when the table is full
// (more classes than the kernel admits: the group overflows).  A hash match is confirmed on the rotated bases.
template <class Cas>
OTG_US_HD uint32_t us_table_insert(uint32_t* slots, uint32_t ns, const UsCand* cands, uint32_t i, const uint8_t* arena, Cas cas)
{
  const UsCand c = cands[i];
  uint32_t h = us_slot(c.hash, c.p, ns);
  for (uint32_t probe = 0; probe < ns; ++probe) {
    uint32_t v = slots[h];
    if (v == 0u) {
      v = cas(&slots[h], 0u, i + 1u);
      if (v == 0u) return h | US_FRESH;
    }
    const UsCand o = cands[v - 1u];
    if (o.p == c.p && o.hash == c.hash && us_same_rotation(arena, o.pos, o.rot, c.pos, c.rot, c.p)) return h;
    if (++h == ns) h = 0;
  }
  return US_NONE;
}

// ---- the representative: the longest segment, then the lower allele, then the lower begin, as one unsigned maximum
OTG_US_HD uint64_t us_rep_key(uint32_t length, uint32_t allele, uint32_t begin)
{
  return ((uint64_t)length << 44) | ((uint64_t)(0xffffffu - allele) << 20) | (uint64_t)(0xfffffu - begin);
}
OTG_US_HD uint32_t us_rep_allele(uint64_t key) { return 0xffffffu - (uint32_t)((key >> 20) & 0xffffffu); }
OTG_US_HD uint32_t us_rep_begin(uint64_t key) { return 0xfffffu - (uint32_t)(key & 0xfffffu); }

// ---- the rank
OTG_US_HD bool us_eligible(uint64_t weight, uint64_t top, const otg_unitset_params& q)
{
  return weight >= (uint64_t)q.min_bases && weight * 1000ull >= (uint64_t)q.min_permille * top;
}
// does class a (weight, length, a member's unit and rotation start) rank before class b?
OTG_US_HD bool us_before(const uint8_t* arena, uint64_t wa, uint32_t pa, uint64_t posa, uint32_t ra, uint64_t wb, uint32_t pb, uint64_t posb, uint32_t rb)
{
  if (wa != wb) return wa > wb;
  if (pa != pb) return pa < pb;
  return us_rotation_less(arena, posa, ra, posb, rb, pa);
}

// ---- the pair list of a group: ranked class c against every d ranked before it
OTG_US_HD uint32_t us_pairs(uint32_t n_ranked) { return n_ranked * (n_ranked - (n_ranked ? 1u : 0u)) / 2u; }
OTG_US_HD uint32_t us_pair_index(uint32_t c, uint32_t d) { return c * (c - 1u) / 2u + d; }   // d < c
// the two copies of a unit of length p against another class's representative gave `edits`
OTG_US_HD bool us_explained(uint32_t edits, uint32_t p, const otg_unitset_params& q) { return (uint64_t)edits * 1000ull <= (uint64_t)q.redundant_permille * 2ull * p; }

// ---- the selection: ranked classes of lengths p[0 .. n), bit c of `redundant` set when class c is explained; sel receives the ranks taken
OTG_US_HD uint32_t us_select(const uint32_t* p, uint32_t n, uint32_t redundant, uint32_t* sel)
{
  uint32_t taken = 0, lanes = 0;
  for (uint32_t c = 0; c < n; ++c) {
    const uint32_t need = (p[c] + 3u) / 4u;
    if (((redundant >> c) & 1u) || taken >= OTG_UNITPARSE_MAX_UNITS || lanes + need > OTG_UNITPARSE_MAX_LANES) continue;
    lanes += need;
    sel[taken++] = c;
  }
  return taken;
}

} // namespace otg_unitset_core

// otg_unitparse_core.hpp — the per-lane arithmetic of the joint unit parse (include/otter_gpu.h states the rule): the three-field key, the
// lane layout of a unit set, the cell step, the closure of the skipped-unit-base and the switch steps, the decision codes of the traceback
// store and the backward walk over them.
//
// Shared by unitparse.hip (device) and tests/unitparse_core_host.cpp (host), which runs the same functions in the kernel's schedule (64
// lanes in lockstep, units at lane boundaries, the ballot words, then the walk) against the plain restatement of the rule.
//
// A key is edits * 2^42 + switches * 2^21 + unit_bases, so one unsigned minimum orders (edits, switches, unit_bases).  Every value a lane
// holds is the key of a real path, or such a key plus the skips that lead on around the unit, so its fields are bounded by what a path can
// collect.  A minimal path to a cell of row i has at most i edits (i vertical steps reach every cell); it consumes a unit base by a diagonal
// step (at most i) or by a skip, which costs an edit: at most 2 i unit bases; it neither starts with a switch nor has two switches in a row
// (dropping one gives a smaller key), so its switches are at most its other steps: 2 i.  While row i + 1 is built from row i (i < L), field
// by field (edits, switches, unit_bases), with p <= OTG_UNITALIGN_MAX_UNIT:
//   both candidates of the cell step                      (i + 1, 2 i, 2 i + 1)
//   the cell plus its scan bias (p - 1 - j) W             (i + p, 2 i, 2 i + p)
//   position p - 1 after the scan plus one skip           (i + 1 + p, 2 i, 2 i + 1 + p)
//   the smallest phase-0 candidate plus one switch        (i + 1 + p, 2 i + 1, 2 i + 1 + p)
//   either of the two plus the way on to j, j W           (i + 2 p, 2 i + 1, 2 i + 2 p)
// The largest low field is 2 (L - 1) + 2 p.  It stays below 2^21 - 1 (all ones is the key of a lane outside every unit) while
// 2 L < 2^21 + 1 - 2 p, which for p = 256 gives OTG_UNITPARSE_MAX_LEN = (2^21 - 1 - 2 * 256 + 1) / 2 = 1048320; the switches stay below
// 2^21 and the edits below 2^22 with room to spare.
#pragma once
#include <cstdint>
#include "../../include/otter_gpu.h"
#include "otg_unitalign_core.hpp"

#define OTG_UP_HD OTG_MOTIF_HD

namespace otg_unitparse_core {

using otg_unitalign_core::ua_class_lanes;
using otg_unitalign_core::ua_class_regs;
using otg_unitalign_core::ua_fold;
using otg_unitalign_core::ua_scan_take;
using otg_unitalign_core::ua_unit_key;

constexpr int UP_FIELD = 21;                                       // bits of unit_bases and of switches; the edits take the 22 above
constexpr uint64_t UP_FIELD_MAX = ((uint64_t)1 << UP_FIELD) - 1u;
static_assert(2ull * (OTG_UNITPARSE_MAX_LEN - 1ull) + 2ull * OTG_UNITALIGN_MAX_UNIT < UP_FIELD_MAX, "the unit_bases field would carry");
static_assert(2ull * OTG_UNITPARSE_MAX_LEN + 2ull * OTG_UNITALIGN_MAX_UNIT >= UP_FIELD_MAX, "OTG_UNITPARSE_MAX_LEN is not the largest safe length");
static_assert(2ull * (OTG_UNITPARSE_MAX_LEN - 1ull) + 1ull < UP_FIELD_MAX, "the switches field would carry");
static_assert((uint64_t)OTG_UNITPARSE_MAX_LEN + 2ull * OTG_UNITALIGN_MAX_UNIT < ((uint64_t)1 << (64 - 2 * UP_FIELD)), "the edits field would overflow");
static_assert(OTG_UNITPARSE_MAX_LEN >= 262143, "the key must carry alleles of 2^18 - 1 bases");

OTG_UP_HD constexpr uint64_t up_sw() { return (uint64_t)1 << UP_FIELD; }               // one switch
OTG_UP_HD constexpr uint64_t up_e() { return (uint64_t)1 << (2 * UP_FIELD); }          // one edit
OTG_UP_HD constexpr uint64_t up_w() { return up_e() + 1u; }                            // one edit and one unit base: a skipped unit base
OTG_UP_HD constexpr uint64_t up_inf() { return ~(uint64_t)0; }                         // a position outside every unit
OTG_UP_HD uint32_t up_edits(uint64_t k) { return (uint32_t)(k >> (2 * UP_FIELD)); }
OTG_UP_HD uint32_t up_switches(uint64_t k) { return (uint32_t)((k >> UP_FIELD) & UP_FIELD_MAX); }
OTG_UP_HD uint32_t up_unit_bases(uint64_t k) { return (uint32_t)(k & UP_FIELD_MAX); }
OTG_UP_HD uint64_t up_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- the lanes of a unit set.  With R positions per lane unit k takes ceil(p_k / R) lanes and starts at a lane boundary, the units side
// by side in set order; R is the smallest of 1, 2, 4 at which the set fits 64 lanes, and the task takes the smallest power of two of lanes
// S >= 4 that holds it (S = 64 at R > 1).  The classes are those of the unit alignment: (S, R) = (4, 1) .. (64, 1), (64, 2), (64, 4).
constexpr int UP_CLASSES = otg_unitalign_core::UA_CLASSES;
constexpr uint32_t UP_NO_CLASS = 0xffffffffu;
OTG_UP_HD uint32_t up_lanes(const uint32_t* p, uint32_t K, uint32_t R)
{
  uint32_t n = 0;
  for (uint32_t k = 0; k < K; ++k) n += (p[k] + R - 1u) / R;
  return n;
}
// the class of a unit set; UP_NO_CLASS: it does not fit one wave
OTG_UP_HD uint32_t up_class(const uint32_t* p, uint32_t K)
{
  const uint32_t n1 = up_lanes(p, K, 1u);
  if (n1 <= 64u) return n1 > 32u ? 4u : n1 > 16u ? 3u : n1 > 8u ? 2u : n1 > 4u ? 1u : 0u;
  if (up_lanes(p, K, 2u) <= 64u) return 5u;
  return up_lanes(p, K, 4u) <= 64u ? 6u : UP_NO_CLASS;
}

// ---- one row
// the diagonal candidate of cell (i + 1, j) from (i, j - 1), and the base of s outside the unit from (i, j)
OTG_UP_HD uint64_t up_diag(uint64_t diag, bool match) { return diag + (match ? (uint64_t)1 : up_w()); }
OTG_UP_HD uint64_t up_vert(uint64_t up) { return up + up_e(); }
// the scan bias of position j of a unit of p bases and the way on from phase 0 to j (otg_unitalign_core.hpp derives the scan)
OTG_UP_HD uint64_t up_bias(uint32_t j, uint32_t p) { return (uint64_t)(p - 1u - j) * up_w(); }
OTG_UP_HD uint64_t up_onward(uint32_t j) { return (uint64_t)j * up_w(); }
// the phase-0 candidate of a unit from inside it: its own phase-0 cell, or its last position (after the scan) plus one skip
OTG_UP_HD uint64_t up_phase0(uint64_t cell0, uint64_t last) { return up_min(cell0, last + up_w()); }
// what reaches phase 0 of a unit from behind: its own last position, or the smallest phase-0 candidate of the set plus one switch
OTG_UP_HD uint64_t up_entry(uint64_t last, uint64_t best0) { return up_min(last + up_w(), best0 + up_sw()); }
// the closed cell of position j: m = its scanned biased cell, entry = up_entry of its unit
OTG_UP_HD uint64_t up_close(uint64_t m, uint64_t bias, uint64_t entry, uint64_t onward) { return up_min(m - bias, entry + onward); }

// The decision of a closed cell h, in the preference order of the traceback: 0 the diagonal, 1 the base outside the unit, 2 the skip from
// the position below (at phase 0 from p - 1, which holds exactly when the unit's last position plus one skip is h), 3 the switch.
enum { UP_DIAG = 0, UP_VERT = 1, UP_SKIP = 2, UP_SWITCH = 3 };
OTG_UP_HD uint32_t up_code(uint64_t h, uint64_t d, uint64_t v, uint32_t j, uint64_t last)
{
  return d == h ? UP_DIAG : v == h ? UP_VERT : (j != 0u || last + up_w() == h) ? UP_SKIP : UP_SWITCH;
}

// ---- the traceback store.  Per wave and row 2 R + 1 words of 64 bits, ballots over the lanes: word 2 r + b holds bit b of the code of
// register r of every lane, word 2 R the units (at their first lane) whose phase-0 candidate is the smallest of their task: the lowest one
// inside the task's lanes is the source of that row's switches.  Row i (1 .. L) of a task lies at (i - 1) * up_words(R).
OTG_UP_HD constexpr uint32_t up_words(uint32_t R) { return 2u * R + 1u; }

// The walk of one task from its end cell: segs[0 .. n_segs) are written from the last to the first.  lane0 = the first lane of the task in
// its wave, S its lanes; unit k of the set is units + unit_off[k], unit_len[k] bytes.  Returns 0, or a code that names what the store
// contradicted (the forward pass and the walk disagree: a defect, never an input's fault); nothing outside segs[0 .. n_segs) is written and
// the walk ends after at most up_walk_cap(L) steps whatever the store holds.
//
// The walk is a chain of dependent loads: the next row to read follows from the code just read.  Only the codes are on that chain; a unit of
// up to 8 bases is kept packed in a register, so the match test of a diagonal step (it only counts the edits) adds no load of its own.
OTG_UP_HD uint64_t up_walk_cap(uint32_t L) { return 8ull * L + 64ull; }

struct UpWalker {
  const uint8_t* units; const uint64_t* unit_off; const uint32_t* unit_len;
  uint32_t K, R, lane0, S;
  otg_unitparse_seg* segs;
  uint32_t at;                                                     // segs[at ..) are written
  uint32_t k, j, p, first;                                         // the unit, the position in it, its length, its first lane
  const uint8_t* u;
  uint64_t packed;                                                 // ua_unit_key of the bases of a unit of up to 8
  otg_unitparse_seg cur;

  OTG_UP_HD void enter(uint32_t unit, uint32_t first_lane)
  {
    k = unit; p = unit_len[k]; first = first_lane; u = units + unit_off[k];
    packed = 0u;
    if (p <= 8u)
      for (uint32_t q = 0; q < p; ++q) packed |= (uint64_t)ua_unit_key(u[q]) << (8u * q);
  }
  OTG_UP_HD uint32_t below() const { return (j ? j : p) - 1u; }
  OTG_UP_HD void diag(uint32_t base)
  {
    const uint32_t jp = below();
    const uint32_t key = p <= 8u ? (uint32_t)(packed >> (8u * jp)) & 255u : ua_unit_key(u[jp]);
    cur.unit_bases += 1u;
    cur.edits += ua_fold(base) != key;
    j = jp;
  }
  OTG_UP_HD void vert() { cur.edits += 1u; }
  OTG_UP_HD void skip() { cur.unit_bases += 1u; cur.edits += 1u; j = below(); }
  // the switch at row i: sources = the row's last word
  OTG_UP_HD uint32_t change(uint64_t sources, uint32_t i)
  {
    if (j != 0u) return 2u;
    const uint64_t mine = (sources >> lane0) & (S >= 64u ? ~(uint64_t)0 : (((uint64_t)1 << S) - 1u));
    if (mine == 0u) return 3u;
    uint32_t src = 0;
    while (!((mine >> src) & 1u)) ++src;
    uint32_t q = 0, acc = 0;
    while (q < K && acc != src) { acc += (unit_len[q] + R - 1u) / R; ++q; }
    if (q >= K || q == k) return 4u;
    if (at == 0u) return 5u;
    cur.begin = i;
    segs[--at] = cur;
    enter(q, lane0 + src);
    cur.unit = k; cur.end = i; cur.unit_bases = 0u; cur.edits = 0u;
    return 0u;
  }
};

OTG_UP_HD uint32_t up_walk(const uint64_t* trace, uint32_t R, uint32_t lane0, uint32_t S, const uint8_t* s, uint32_t L, const uint8_t* units,
                           const uint64_t* unit_off, const uint32_t* unit_len, uint32_t K, uint32_t end_unit, uint32_t end_phase,
                           otg_unitparse_seg* segs, uint32_t n_segs)
{
  const uint32_t words = up_words(R);
  const uint64_t cap = up_walk_cap(L);
  UpWalker W;
  W.units = units; W.unit_off = unit_off; W.unit_len = unit_len; W.K = K; W.R = R; W.lane0 = lane0; W.S = S; W.segs = segs; W.at = n_segs;
  uint32_t first = 0;
  for (uint32_t q = 0; q < end_unit; ++q) first += (unit_len[q] + R - 1u) / R;
  W.enter(end_unit, lane0 + first);
  W.j = end_phase;
  W.cur.unit = end_unit; W.cur.begin = 0u; W.cur.end = L; W.cur.unit_bases = 0u; W.cur.edits = 0u; W.cur.start_phase = 0u;
  uint32_t i = L;
  uint64_t step = 0;
  while (i > 0u) {
    if (step++ >= cap) return 1u;
    const uint64_t* row = trace + (uint64_t)(i - 1u) * words;
    const uint32_t lane = W.first + W.j / R, r = W.j % R;
    const uint32_t code = (uint32_t)((row[2u * r] >> lane) & 1u) | ((uint32_t)((row[2u * r + 1u] >> lane) & 1u) << 1);
    if (code == UP_DIAG) { W.diag(s[i - 1u]); --i; }
    else if (code == UP_VERT) { W.vert(); --i; }
    else if (code == UP_SKIP) W.skip();
    else if (const uint32_t bad = W.change(row[2u * R], i)) return bad;
  }
  if (W.at != 1u) return 6u;
  W.cur.begin = 0u; W.cur.start_phase = W.j;
  segs[0] = W.cur;
  return 0u;
}

} // namespace otg_unitparse_core

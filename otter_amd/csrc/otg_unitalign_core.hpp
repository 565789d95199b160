// otg_unitalign_core.hpp — the per-lane arithmetic of the cyclic unit alignment (include/otter_gpu.h states the rule): the packed key in its
// two widths, the cell step, the biased prefix minimum that closes the skipped-unit-base step around the cycle in one scan, the final order,
// and the segment classes and length buckets the tasks are binned by.
//
// Shared by unitalign.hip (device) and tests/unitalign_core_host.cpp (host), which runs the same functions in the kernel's schedule (64
// lanes in lockstep, segments side by side, the exchanges done by indexing) against the plain restatement of the rule.
//
// A key is edits * 2^SHIFT + unit_bases, so one unsigned minimum orders (edits, unit_bases).  The narrow key has SHIFT = 16.  While row
// i + 1 is built from row i (i < L) a lane holds at most, field by field (edits, unit_bases), with p <= OTG_UNITALIGN_MAX_UNIT:
//   a cell of row i                            (i, 2 i):       i vertical steps reach every cell, and a unit base is consumed by a diagonal
//                                                              step (at most i of them) or by a skip, which costs an edit
//   both candidates of the cell step           (i + 1, 2 i + 1)
//   the cell plus its scan bias (p - 1 - j) W  (i + p, 2 i + p)
//   position p - 1 after the scan plus the wrap term (j + 1) W:  (i + 2 p, 2 i + 2 p)
// The largest is 2 (L - 1) + 2 p in the low field.  It stays below 2^16 - 1 (all ones in both fields is the key of a lane outside the unit)
// while 2 L < 65537 - 2 p, which for p = 256 gives OTG_UNITALIGN_NARROW_LEN = (65535 - 2 * 256 + 1) / 2 = 32512.  No field carries into the
// other up to that length, so the narrow and the wide tier order every pair of keys alike.
#pragma once
#include <cstdint>
#include "../../include/otter_gpu.h"
#include "otg_motif_core.hpp"

#define OTG_UA_HD OTG_MOTIF_HD

namespace otg_unitalign_core {

using otg_motif_core::mo_code;

static_assert(2u * (OTG_UNITALIGN_NARROW_LEN - 1u) + 2u * OTG_UNITALIGN_MAX_UNIT < 65535u, "a narrow key field would carry");
static_assert(2u * OTG_UNITALIGN_NARROW_LEN + 2u * OTG_UNITALIGN_MAX_UNIT >= 65535u, "OTG_UNITALIGN_NARROW_LEN is not the largest safe length");

template <typename K> struct UaKey;
template <> struct UaKey<uint32_t> { static constexpr int SHIFT = 16; };
template <> struct UaKey<uint64_t> { static constexpr int SHIFT = 32; };
template <typename K> OTG_UA_HD constexpr K ua_e() { return (K)1 << UaKey<K>::SHIFT; }            // one edit
template <typename K> OTG_UA_HD constexpr K ua_w() { return ua_e<K>() + (K)1; }                  // one edit and one unit base: a skipped unit base
template <typename K> OTG_UA_HD constexpr K ua_inf() { return ~(K)0; }                           // a position outside the unit
template <typename K> OTG_UA_HD uint32_t ua_edits(K k) { return (uint32_t)(k >> UaKey<K>::SHIFT); }
template <typename K> OTG_UA_HD uint32_t ua_unit_bases(K k) { return (uint32_t)(k & (ua_e<K>() - (K)1)); }

// ---- classes.  A task takes a segment of S lanes with R unit positions per lane (position j = R * lane + r): the smallest power of two
// S >= max(p, 4) up to 64, then 2 and 4 positions per lane at S = 64.  seg64: every unit up to 64 bases takes a whole wave.
constexpr int UA_CLASSES = 7;
OTG_UA_HD constexpr int ua_class_lanes(int c) { return c < 4 ? 4 << c : 64; }
OTG_UA_HD constexpr int ua_class_regs(int c) { return c < 5 ? 1 : c == 5 ? 2 : 4; }
OTG_UA_HD uint32_t ua_class(uint32_t p, bool seg64)
{
  if (p > 128u) return 6u;
  if (p > 64u) return 5u;
  if (seg64 || p > 32u) return 4u;
  return p > 16u ? 3u : p > 8u ? 2u : p > 4u ? 1u : 0u;
}

// ---- length buckets: the tasks of a class are ordered by bucket, so the tasks that share a wave end within 1 / 16 of each other.
// L / 16 below 256, then the exponent and the four bits under the leading one.
constexpr uint32_t UA_BUCKETS = 16u + 12u * 16u;
OTG_UA_HD uint32_t ua_bucket(uint32_t L)
{
  if (L < 256u) return L >> 4;
  uint32_t e = 8u;
  while ((L >> (e + 1u)) != 0u) ++e;                              // L <= OTG_UNITALIGN_MAX_LEN < 2^20: e <= 19
  return 16u + (e - 8u) * 16u + ((L >> (e - 4u)) & 15u);
}

// the flags of a task that is not aligned; 0: it is
OTG_UA_HD uint32_t ua_refusal(uint32_t L, uint32_t p)
{
  if (p == 0u) return OTG_UNITALIGN_NO_UNIT;
  if (p > OTG_UNITALIGN_MAX_UNIT) return OTG_UNITALIGN_UNIT_TOO_LONG;
  if (L > OTG_UNITALIGN_MAX_LEN) return OTG_UNITALIGN_TOO_LONG;
  return 0u;
}

// ---- one row.  A base is compared as its byte with bit 5 cleared (the letter case).  A unit position holds that byte when it is one of
// A C G T and 0xff otherwise, which no folded byte equals; an allele byte that equals a unit position's is then one of A C G T as well,
// so one equality is the whole match test of the rule: same code, and the code below 4.
OTG_UA_HD uint32_t ua_fold(uint32_t ch) { return ch & 0xdfu; }
OTG_UA_HD uint32_t ua_unit_key(uint8_t ch) { return mo_code(ch) < 4u ? ua_fold(ch) : 0xffu; }

// the cell (i + 1, j) from (i, j - 1) = diag and (i, j) = up: the diagonal step (match: s[i] against u[j - 1]) and the base of s outside the unit
template <typename K> OTG_UA_HD K ua_cell(K diag, K up, bool match)
{
  const K d = diag + (match ? (K)1 : ua_w<K>());
  const K v = up + ua_e<K>();
  return d < v ? d : v;
}

// The skipped-unit-base step, H[j] = min over k of T[k] + ((j - k) mod p) W, in one prefix scan.  With the bias c(j) = (p - 1 - j) W,
// H1[j] = min over k <= j of T[k] + (j - k) W = (min over k <= j of T[k] + c(k)) - c(j): a plain prefix minimum of the biased cells.
template <typename K> OTG_UA_HD K ua_bias(uint32_t j, uint32_t p) { return (K)(p - 1u - j) * ua_w<K>(); }
// one step of that prefix minimum: `from` is the value `d` positions below, `ok` says it exists inside the segment (MAX: of the prefix
// maximum of the tract mode, otg_tract_core.hpp)
template <typename K, bool MAX = false> OTG_UA_HD K ua_scan_take(K x, K from, bool ok) { return ok && (MAX ? from > x : from < x) ? from : x; }
// m = the scanned biased cell of position j, last = that of position p - 1 (its bias is 0, so it is H1[p - 1]): the paths that wrap
// from p - 1 to 0 and go on to j cost (j + 1) W more
template <typename K> OTG_UA_HD K ua_close(K m, K last, uint32_t j, uint32_t p)
{
  const K h1 = m - ua_bias<K>(j, p), wr = last + (K)(j + 1u) * ua_w<K>();
  return h1 < wr ? h1 : wr;
}

// the final order: the smaller key, ties to the smaller position (a total order on the positions of a unit)
template <typename K> OTG_UA_HD bool ua_better(K a, uint32_t ja, K b, uint32_t jb) { return a < b || (a == b && ja < jb); }

} // namespace otg_unitalign_core

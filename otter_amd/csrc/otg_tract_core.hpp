// otg_tract_core.hpp — the per-lane arithmetic of the tract mode (include/otter_gpu.h states the rule): the local wraparound alignment that
// finds the repeat tract inside a flanked allele.  The packed key in its two widths, the cell step, the biased prefix maximum that closes
// the skipped-unit-base step around the cycle in one scan, the running best, the final order and the length up to which the narrow key
// holds.  The segment classes and length buckets are those of the unit alignment (otg_unitalign_core.hpp).
//
// Shared by tract.hip (device) and tests/tract_core_host.cpp (host), which runs the same functions in the kernel's schedule (64 lanes in
// lockstep, segments side by side, the exchanges done by indexing) against the plain restatement of the rule.
//
// A key is score * 2^SHIFT + begin, so one unsigned maximum orders (score, begin).  The narrow key has SHIFT = 16.  While row i + 1 is built
// from row i (i < L) a lane holds at most, field by field (score, begin), with match = M, indel = I and p the unit length:
//   a cell of row i                            (M i, i):           a score grows by M per consumed base at most, a begin is a row number
//   the fresh start of row i + 1               (0, i + 1)
//   the diagonal candidate                     (M (i + 1), i)      the other two candidates only subtract, saturating at key 0
//   the cell plus its scan bias j I            (M (i + 1) + (p - 1) I, i + 1)
//   the scanned cell less its bias, the wrap term, the closed cell, the running best: each at most a cell of row i + 1
// The largest are M L + (p - 1) I in the score field and L in the begin field.  Both stay below 2^16 while L <= tr_narrow_len: no field
// carries into the other up to that length, so the narrow and the wide tier order every pair of keys alike.  The wide key (32 / 32) holds
// every task the rule admits: 16 * 1048575 + 255 * 64 < 2^32.
#pragma once
#include <cstdint>
#include "otg_unitalign_core.hpp"

namespace otg_tract_core {

using otg_unitalign_core::UaKey;
using otg_unitalign_core::ua_e;

static_assert(16ull * OTG_TRACT_MAX_LEN + 255ull * 64ull < (1ull << 32), "a wide key field would carry");

OTG_UA_HD bool tr_params_ok(const otg_tract_params& q)
{
  return q.match >= 1u && q.match <= 16u && q.mismatch >= 1u && q.mismatch <= 64u && q.indel >= 1u && q.indel <= 64u && q.min_score <= (1u << 24);
}

// the longest allele of the narrow key for these scores and this unit length (1 <= p <= OTG_UNITALIGN_MAX_UNIT)
OTG_UA_HD uint32_t tr_narrow_len(const otg_tract_params& q, uint32_t p)
{
  const uint32_t bias = (p - 1u) * q.indel;                       // <= 255 * 64
  const uint32_t by_score = (65535u - bias) / q.match;
  return by_score < 65535u ? by_score : 65535u;
}

// the flags of a task that is not aligned; 0: it is
OTG_UA_HD uint32_t tr_refusal(uint32_t L, uint32_t p)
{
  if (p == 0u) return OTG_TRACT_NO_UNIT;
  if (p > OTG_UNITALIGN_MAX_UNIT) return OTG_TRACT_UNIT_TOO_LONG;
  if (L > OTG_TRACT_MAX_LEN) return OTG_TRACT_TOO_LONG;
  return 0u;
}

template <typename K> OTG_UA_HD uint32_t tr_score(K k) { return (uint32_t)(k >> UaKey<K>::SHIFT); }
template <typename K> OTG_UA_HD uint32_t tr_begin(K k) { return (uint32_t)(k & (ua_e<K>() - (K)1)); }
template <typename K> OTG_UA_HD K tr_pen(uint32_t score) { return (K)score << UaKey<K>::SHIFT; }      // a score as a key difference
template <typename K> OTG_UA_HD K tr_max(K a, K b) { return a > b ? a : b; }
// a penalty taken off a key: a score that would not stay positive leaves a key below every fresh start of the row (score 0, an older begin)
template <typename K> OTG_UA_HD K tr_sub(K k, K pen) { return tr_max<K>(k, pen) - pen; }

// the cell (i + 1, j) before the closure, from (i, j - 1) = diag and (i, j) = up; fresh = i + 1, the key of a start in this row
template <typename K> OTG_UA_HD K tr_cell(K diag, K up, bool match, K m, K x, K g, K fresh)
{
  const K d = match ? diag + m : tr_sub<K>(diag, x);
  return tr_max<K>(tr_max<K>(d, tr_sub<K>(up, g)), fresh);
}

// The skipped-unit-base step, H[j] = max over k of T[k] - ((j - k) mod p) I, in one prefix scan.  With the bias c(j) = j I in the score field,
// H1[j] = max over k <= j of T[k] - (j - k) I = (max over k <= j of T[k] + c(k)) - c(j): a plain prefix maximum of the biased cells.  T[j]
// itself takes part, so the difference never goes below the cell, and a path whose score is not positive loses to the cell's fresh start.
template <typename K> OTG_UA_HD K tr_bias(uint32_t j, K g) { return (K)j * g; }
// m = the scanned biased cell of position j, last = the closed cell H1[p - 1]: the paths that wrap from p - 1 to 0 and go on to j lose
// (j + 1) I more, and are no candidate when their score would not stay positive
template <typename K> OTG_UA_HD K tr_close(K m, K last, K bias, K g)
{
  return tr_max<K>(m - bias, tr_sub<K>(last, bias + g));
}

// the running best of a position: replaced only by a strictly larger score, so the smallest end wins
template <typename K> OTG_UA_HD bool tr_improves(K v, K best) { return v > (best | (ua_e<K>() - (K)1)); }

// the final order: the larger score, then the smaller end, then the larger begin, then the smaller position
template <typename K> OTG_UA_HD bool tr_better(K a, uint32_t ea, uint32_t ja, K b, uint32_t eb, uint32_t jb)
{
  const uint32_t sa = tr_score<K>(a), sb = tr_score<K>(b);
  if (sa != sb) return sa > sb;
  if (ea != eb) return ea < eb;
  if (a != b) return a > b;
  return ja < jb;
}

} // namespace otg_tract_core

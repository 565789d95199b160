// otg_repeat_core.hpp — the per-word and per-run arithmetic of the repeat-structure parse (include/otter_gpu.h states the rule): the walk over
// the match bits of one period that yields its kept runs, the candidate a run is under a window [lo, hi), the total order best() reduces
// with, and the unit compare that keeps the phase across an interruption.  The planes and the match bits are those of otg_motif_core.hpp.
//
// Shared by repeat.hip (device) and tests/repeat_core_host.cpp (host), which runs the same functions in the kernels' schedule (256 strided
// "threads", then the tree) against the plain restatement of the rule.
#pragma once
#include "otg_motif_core.hpp"

namespace otg_repeat_core {

using namespace otg_motif_core;

constexpr int REPEAT_T = 256;                                   // threads of every repeat workgroup

struct RpRun { uint32_t p, a, e; };                             // a kept run: period, first base, one past the last base it covers

// P of the rule; 0 for an allele beyond the length cap
OTG_MOTIF_HD uint32_t rp_period_range(uint32_t L, uint32_t max_period)
{
  if (L > OTG_REPEAT_MAX_LEN) return 0u;
  const uint32_t h = L >> 1;
  return h < max_period ? h : max_period;
}

// the index of the lowest set bit, x != 0
OTG_MOTIF_HD uint32_t rp_ffs(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__ffs((int)x) - 1u;
#else
  return (uint32_t)__builtin_ctz(x);
#endif
}

// the number of zero bits above the highest set bit; 32 for x == 0
OTG_MOTIF_HD uint32_t rp_clz(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__clz((int)x);
#else
  return x ? (uint32_t)__builtin_clz(x) : 32u;
#endif
}

// "enough" of step 3: k copies of period p
OTG_MOTIF_HD bool rp_enough(uint32_t k, uint32_t p, uint32_t min_copies, uint32_t min_span) { return k >= min_copies && (uint64_t)k * p >= min_span; }

// The shortest stretch [a, e) of period p whose copy count (e - a) / p is enough: k is enough exactly when k >= max(min_copies,
// ceil(min_span / p)), so a run is kept exactly when e - a reaches this (at most 1024 * 4096 or 65535 + 4096).
OTG_MOTIF_HD uint32_t rp_min_len(uint32_t p, uint32_t min_copies, uint32_t min_span)
{
  const uint32_t ks = (min_span + p - 1u) / p;
  return (ks > min_copies ? ks : min_copies) * p;
}

// A word x of match bits without the runs of ones that cannot belong to a kept run.  A kept run of period p has at least
// nb = rp_min_len(p) - p >= 1 bits.  What may belong to one: the ones at the top of the word (the run may go on in the next word), the ones
// at the bottom when a run is open (it goes on here), and a run of at least nb ones (found by an AND over a window of nb bits in
// log2(nb) shifts, grown back by the same shifts with OR; zeros come in at the top, where the first mask has the run anyway).  The runs
// that are left keep every bit, so the walk sees the same starts and ends for them.  In unrelated sequence a quarter of the bits are ones
// in runs of one or two: without this the walk takes eight to twelve transitions per word, with it mostly none.
OTG_MOTIF_HD uint32_t rp_prune(uint32_t x, bool open, uint32_t nb)
{
  const uint32_t lz = rp_clz(~x);
  uint32_t keep = lz ? 0xffffffffu << (32u - lz) : 0u;
  if (open) keep |= x & ~(x + 1u);
  if (nb < 32u) {
    uint32_t y = x, w = 1;
    for (; 2u * w <= nb; w <<= 1) y &= y >> w;
    y &= y >> (nb - w);                                         // bit i: x[i .. i + nb) are ones
    uint32_t d = y;
    for (w = 1; 2u * w <= nb; w <<= 1) d |= d << w;
    keep |= d | (d << (nb - w));
  }
  return x & keep;
}

// The kept runs of period p, 1 <= p <= L / 2, in ascending order of a: returns their number and, with out != nullptr, writes them to
// out[0 ..).  Planes as for mo_count (the zero tail makes every bit at or past L - p zero, so a run that reaches L - p closes there or is
// still open behind the last word).  The lane carries the open run's start across words; an all-ones word extends the run and an all-zero
// word closes it, any other word is pruned (rp_prune) and walked by find-first-bit on the word (the next start) and on its complement (the
// next end).
OTG_MOTIF_HD uint32_t rp_runs(const uint32_t* LO, const uint32_t* HI, const uint32_t* V, uint32_t L, uint32_t p, uint32_t min_len, RpRun* out)
{
  const uint32_t q = p >> 5, r = p & 31u, nw = (L - p + 31u) >> 5;
  const uint32_t nb = min_len - p;
  uint32_t l0 = LO[q], h0 = HI[q], v0 = V[q], cnt = 0, a = 0;
  bool open = false;
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t l1 = LO[w + q + 1], h1 = HI[w + q + 1], v1 = V[w + q + 1];
    uint32_t x = mo_eq_word(LO[w], HI[w], V[w], l0, l1, h0, h1, v0, v1, r);
    l0 = l1; h0 = h1; v0 = v1;
    if (x == (open ? 0xffffffffu : 0u)) continue;               // the run goes on / nothing starts
    x = rp_prune(x, open, nb);
    if (!open && x == 0u) continue;
    const uint32_t base = w << 5;
    for (;;) {
      if (open) {
        if (x == 0xffffffffu) break;
        const uint32_t t = rp_ffs(~x);                          // the run ends in front of bit t: it covers [a, base + t + p)
        if (base + t + p - a >= min_len) {
          if (out) { out[cnt].p = p; out[cnt].a = a; out[cnt].e = base + t + p; }
          ++cnt;
        }
        open = false;
        x &= ~((1u << t) - 1u);
      } else {
        if (x == 0u) break;
        const uint32_t t = rp_ffs(x);
        a = base + t;
        open = true;
        x |= (1u << t) - 1u;
      }
    }
  }
  if (open && L - a >= min_len) {                               // open behind the last word: bit L - p - 1 was its last one, e = L
    if (out) { out[cnt].p = p; out[cnt].a = a; out[cnt].e = L; }
    ++cnt;
  }
  return cnt;
}

// What a run is to best(lo, hi): gain g and cost w with the start st (w == 0: skipped, or no run yet), and which run it is.
struct RpCand { uint32_t g, w, st, p, idx; };

OTG_MOTIF_HD RpCand rp_cand(const RpRun& r, uint32_t idx, uint32_t lo, uint32_t hi, uint32_t min_copies, uint32_t min_span)
{
  RpCand c = {0u, 0u, 0u, 0u, 0u};
  const uint32_t st = r.a > lo ? r.a : lo, en = r.e < hi ? r.e : hi;
  if (en <= st) return c;
  const uint32_t k = (en - st) / r.p;
  if (!rp_enough(k, r.p, min_copies, min_span)) return c;
  c.g = st - lo + k * r.p; c.w = st - lo + r.p; c.st = st; c.p = r.p; c.idx = idx;
  return c;
}

// Is candidate x a better best() than y?  The higher g / w, cross-multiplied in 64 bits (g, w < 2^21); ties to the smaller st, then to the
// smaller p.  Two runs never share (st, p), so this is a total order on the candidates of a window and a reduction of any shape finds the same one.
OTG_MOTIF_HD bool rp_better(const RpCand& x, const RpCand& y)
{
  if (x.w == 0u) return false;
  if (y.w == 0u) return true;
  const uint64_t l = (uint64_t)x.g * y.w, r = (uint64_t)y.g * x.w;
  if (l != r) return l > r;
  if (x.st != y.st) return x.st < y.st;
  return x.p < y.p;
}

// c[t .. t + p) == c[pb .. pb + p) on the codes of s (step 6)
OTG_MOTIF_HD bool rp_unit_equal(const uint8_t* s, uint32_t t, uint32_t pb, uint32_t p)
{
  for (uint32_t i = 0; i < p; ++i)
    if (mo_code(s[t + i]) != mo_code(s[pb + i])) return false;
  return true;
}

} // namespace otg_repeat_core

// otg_motif_core.hpp — the per-allele arithmetic of the motif annotation (include/otter_gpu.h states the rule): base codes, the three
// bit-planes, the shifted self-comparison on them, and the two orders the reductions use.
//
// Shared by motif.hip (device) and tests/motif_core_host.cpp (host), which runs the same functions in the kernels' schedule (256 strided
// "threads", then the tree) against the plain restatement of the rule: the plane logic and the tie order are checked without a device.
#pragma once
#include <cstdint>
#include <cstring>
#include "../../include/otter_gpu.h"

#if defined(__HIPCC__)
#define OTG_MOTIF_HD __host__ __device__ __forceinline__
#else
#define OTG_MOTIF_HD inline
#endif

namespace otg_motif_core {

constexpr int MOTIF_T = 256;                                    // threads of every motif workgroup

OTG_MOTIF_HD uint32_t mo_code(uint8_t ch)
{
  return (ch == 'A' || ch == 'a') ? 0u : (ch == 'C' || ch == 'c') ? 1u : (ch == 'G' || ch == 'g') ? 2u : (ch == 'T' || ch == 't') ? 3u : 4u;
}

// P of the rule; 0 for an allele beyond the length cap
OTG_MOTIF_HD uint32_t mo_period_range(uint32_t L, uint32_t max_period)
{
  if (L > OTG_MOTIF_MAX_LEN) return 0u;
  const uint32_t h = L >> 1;
  return h < max_period ? h : max_period;
}

// ({hi, lo} >> r) & 0xffffffff, 0 <= r <= 31: v_alignbit_b32
OTG_MOTIF_HD uint32_t mo_funnel(uint32_t hi, uint32_t lo, uint32_t r)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, r);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> r);
#endif
}

OTG_MOTIF_HD uint32_t mo_popc(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}

// Word w of the three planes of s[0 .. L): bases 32 w .. 32 w + 31, bit k = base 32 w + k; lo / hi = bit 0 / 1 of the code, v = an ACGT byte
// below L (lo and hi are 0 where v is).  Reads 32 bytes at s + 32 w: called only with 32 w < L, it touches at most 31 bytes past the allele
// (the arenas extend 64 bytes past every row).
OTG_MOTIF_HD void mo_pack_word(const uint8_t* s, uint32_t L, uint32_t w, uint32_t* lo, uint32_t* hi, uint32_t* v)
{
  uint8_t b[32];
  __builtin_memcpy(b, s + (size_t)w * 32u, 32);
  uint32_t l = 0, h = 0, ok = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 32; ++k) {
    const uint32_t c = mo_code(b[k]);
    const uint32_t in = (c < 4u && w * 32u + (uint32_t)k < L) ? 1u : 0u;
    l |= (c & 1u & in) << k;
    h |= ((c >> 1) & 1u & in) << k;
    ok |= in << k;
  }
  *lo = l; *hi = h; *v = ok;
}

// The match bits of one word of a shifted compare at p = 32 q + r: bit k = (s[i] == s[i + p], both ACGT) for i = 32 w + k, from word w of
// the planes (lo, hi, v) and the words w + q (x0) and w + q + 1 (x1) that hold i + p.  What mo_count popcounts and otg_repeat_core.hpp walks.
OTG_MOTIF_HD uint32_t mo_eq_word(uint32_t lo, uint32_t hi, uint32_t v, uint32_t l0, uint32_t l1, uint32_t h0, uint32_t h1, uint32_t v0, uint32_t v1,
                                 uint32_t r)
{
  const uint32_t ls = mo_funnel(l1, l0, r), hs = mo_funnel(h1, h0, r), vs = mo_funnel(v1, v0, r);
  return ~((lo ^ ls) | (hi ^ hs)) & v & vs;
}

// m(p), 1 <= p <= L / 2, from planes of (L + 31) / 32 words followed by at least one zero word.  The zero tail makes every base at or past
// L invalid, so i + p < L needs no mask of its own; the words w < ceil((L - p) / 32) hold every i < L - p, and the highest word read is
// w + (p >> 5) + 1 <= (L + 31) / 32.  Per word: one funnel shift per plane, ~((lo ^ lo') | (hi ^ hi')) & v & v', a popcount.
OTG_MOTIF_HD uint32_t mo_count(const uint32_t* LO, const uint32_t* HI, const uint32_t* V, uint32_t L, uint32_t p)
{
  const uint32_t q = p >> 5, r = p & 31u, nw = (L - p + 31u) >> 5;
  uint32_t l0 = LO[q], h0 = HI[q], v0 = V[q], cnt = 0;
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t l1 = LO[w + q + 1], h1 = HI[w + q + 1], v1 = V[w + q + 1];
    cnt += mo_popc(mo_eq_word(LO[w], HI[w], V[w], l0, l1, h0, h1, v0, v1, r));
    l0 = l1; h0 = h1; v0 = v1;
  }
  return cnt;
}

// Is period pa (m = ma) a better "best" than period pb?  The higher m / (L - p), cross-multiplied in 64 bits (m, L < 2^20); ties to the
// smaller period; 0 = no period yet.  A total order on the periods of an allele, so a reduction finds the period the rule's ascending scan
// ends with, whatever its shape.
OTG_MOTIF_HD bool mo_better(uint32_t L, uint32_t pa, uint32_t ma, uint32_t pb, uint32_t mb)
{
  if (pa == 0u) return false;
  if (pb == 0u) return true;
  const uint64_t x = (uint64_t)ma * (L - pb), y = (uint64_t)mb * (L - pa);
  return x > y || (x == y && pa < pb);
}

// is p within the slack of the best ratio?  m(p) (L - best) 1000 >= (1000 - slack) m(best) (L - p), below 2^50
OTG_MOTIF_HD bool mo_within_slack(uint32_t L, uint32_t p, uint32_t mp, uint32_t best, uint32_t mbest, uint32_t slack)
{
  return (uint64_t)mp * (L - best) * 1000ull >= (uint64_t)(1000u - slack) * mbest * (L - p);
}

// the majority base of a phase from its four counts: ties to the lower code, no ACGT byte at all: N
OTG_MOTIF_HD uint8_t mo_majority(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
  uint32_t bc = c0; uint8_t ch = 'A';
  if (c1 > bc) { bc = c1; ch = 'C'; }
  if (c2 > bc) { bc = c2; ch = 'G'; }
  if (c3 > bc) { bc = c3; ch = 'T'; }
  return bc ? ch : (uint8_t)'N';
}

// is rotation a of the period-byte unit u smaller than rotation b, by byte value?  ties to the smaller offset (a total order)
OTG_MOTIF_HD bool mo_rot_less(const uint8_t* u, uint32_t period, uint32_t a, uint32_t b)
{
  if (a == b) return false;
  uint32_t ia = a, ib = b;
  for (uint32_t k = 0; k < period; ++k) {
    const uint8_t ca = u[ia], cb = u[ib];
    if (ca != cb) return ca < cb;
    if (++ia == period) ia = 0;
    if (++ib == period) ib = 0;
  }
  return a < b;
}

} // namespace otg_motif_core

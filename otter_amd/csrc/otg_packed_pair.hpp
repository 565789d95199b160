// otg_packed_pair.hpp — what the packed window kernels of the adaptive mode (wfa_adaptive.hip) share on the side of the SEQUENCES: the pair
// packed to 2 bits per base in LDS, the 32-base probe of their sweeps and the lane-mask helpers.  (The register tiers of wfa_affine_reg.hip
// keep their own pack and probe: their slack words differ.)
#pragma once
#include "otg_wfadaptive.hpp"

namespace otg_adaptive {

using otg_affine::lds_u32;
using lds_char = __attribute__((address_space(3))) char;

// lane masks of comparisons (v_cmp into an SGPR pair; the logic on them runs on the scalar unit) and a select on a lane mask.  Written with bools,
// hipcc 7.2 turns "does any lane ..." and "or into the flag" into a select, an and and a compare on the vector unit each (see wfa_affine_reg.hip)
__device__ __forceinline__ unsigned long long mk_eq(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 32); }
__device__ __forceinline__ unsigned long long mk_sle(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 41); }
__device__ __forceinline__ unsigned long long mk_ule(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 37); }
__device__ __forceinline__ int sel(unsigned long long m, int a, int b) { int r; asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m)); return r; }     // lane in m ? a : b

// Packs both sequences of a pair to 2 bits per base (word q = bases 16 q .. 16 q + 15, code (byte >> 1) & 3; pattern at word 0, text at word
// offT = (pl + 15) / 16 + 3; three slack words behind each): thread `tid` of `nt` packs words tid, tid + nt, ... — a wave for its own pair
// (lane, 64) or a block for its one pair (the caller's __syncthreads orders it).  Returns whether THIS WAVE met a byte outside ACGT.
__device__ __forceinline__ bool pack_pair(volatile lds_u32* SQ, const uint8_t* P, int pl, const uint8_t* T, int tl, int offT, int tid, int nt)
{
  bool bad = false;
  auto pack = [&](const uint8_t* S, int len, int woff) {
    for (int q = tid; q < (len + 15) / 16 + 3; q += nt) {
      uint32_t w = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int b0 = 16 * q + 8 * j;
        const uint64_t x = b0 < len ? otg_load8(S + b0) : 0ull;        // (the arena has 64 bytes of slack behind its last sequence)
#pragma unroll
        for (int t2 = 0; t2 < 8; ++t2) {
          const uint32_t c = (uint32_t)(x >> (8 * t2)) & 0xffu;
          const uint32_t code = (c >> 1) & 3u;
          if (b0 + t2 < len && c != ((0x47544341u >> (8 * code)) & 0xffu)) bad = true;
          w |= code << (2 * (8 * j + t2));
        }
      }
      SQ[woff + q] = w;
    }
  };
  pack(P, pl, 0);
  pack(T, tl, offT);
  return __ballot(bad) != 0ull;
}

// The packed pair of one wave: a probe compares 32 bases with six LDS reads instead of two HBM round trips — under the cut a wave advances one
// score at a time and every score ends in a probe, so the probe latency IS the kernel's speed.  A pair with a byte outside ACGT, or too
// long for the wave's share of LDS, is not packed (`ok` false) and runs on the byte probes of the generic kernels.
struct PackedPair {
  volatile lds_u32* SQ; int offT; bool ok;
  // seqw = words of LDS this wave owns for the pair (dynamic shared memory, sized by the launcher from the batch's longest read)
  __device__ __forceinline__ void init(const uint8_t* P, int pl, const uint8_t* T, int tl, int lane, int seqw)
  {
    offT = (pl + 15) / 16 + 3;
    ok = offT + (tl + 15) / 16 + 3 <= seqw;
    if (ok) ok = !pack_pair(SQ, P, pl, T, tl, offT, lane, 64);
  }
  __device__ __forceinline__ uint64_t ld32(int woff, int pos) const
  {
    const int w = woff + (pos >> 4);
    const uint32_t sh = (uint32_t)(pos & 15) * 2u;
    const uint32_t d0 = SQ[w], d1 = SQ[w + 1], d2 = SQ[w + 2];
    return (uint64_t)__builtin_amdgcn_alignbit(d1, d0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, sh) << 32);
  }
  // equal bases from pattern position v / text position h on, at most 32 and at most rem (0 <= v, h; rem >= 0): the drains' probe
  __device__ __forceinline__ int match32(int v, int h, int rem) const
  {
    const uint64_t xx = ld32(0, v) ^ ld32(offT, h);
    const int m = xx ? (int)(__builtin_ctzll(xx) >> 1) : 32;
    return imin(m, rem);
  }
};

// The sweeps' probe, wherever the offsets point (a branch-free sweep probes for invalid cells too: LDS reads outside the allocation return zero,
// inside it harmless words): equal leading bases of pattern[pv ..] and text[ph ..], at most 32.  SQB = the packed pair, offT4 = 4 * offT.
__device__ __forceinline__ int probe32(const volatile lds_char* SQB, int offT4, int pv, int ph)
{
  const int wp = (pv >> 2) & ~3, wt = offT4 + ((ph >> 2) & ~3);      // byte addresses of the first word of each 32-base window
  const uint32_t sp = (uint32_t)(pv & 15) * 2u, st = (uint32_t)(ph & 15) * 2u;
  const volatile lds_u32* pp = (const volatile lds_u32*)(SQB + wp);
  const volatile lds_u32* pt = (const volatile lds_u32*)(SQB + wt);
  const uint32_t p0 = pp[0], p1 = pp[1], p2 = pp[2], q0 = pt[0], q1 = pt[1], q2 = pt[2];
  const uint32_t xl = __builtin_amdgcn_alignbit(p1, p0, sp) ^ __builtin_amdgcn_alignbit(q1, q0, st);
  const uint32_t xh = __builtin_amdgcn_alignbit(p2, p1, sp) ^ __builtin_amdgcn_alignbit(q2, q1, st);
  uint32_t flo, fhi;      // v_ffbl_b32: index of the lowest set bit, 0xffffffff for zero — which is what the min below wants
  asm("v_ffbl_b32 %0, %1" : "=v"(flo) : "v"(xl));
  asm("v_ffbl_b32 %0, %1" : "=v"(fhi) : "v"(xh));
  const uint32_t a = flo < (fhi | 32u) ? flo : (fhi | 32u);
  return (int)((a < 64u ? a : 64u) >> 1);
}

} // namespace otg_adaptive

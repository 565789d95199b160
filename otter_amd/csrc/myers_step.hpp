// myers_step.hpp — one column of one 64-row block of the bit-parallel edit recurrence (Myers 1999 / Hyyrö 2003), on 32-bit halves.
//
// Shared by myers_edit.hip (device) and tests/edit_step_host.cpp (host): the host evaluates the plain boolean expressions below, the
// device issues them as v_bitop3_b32 with the truth table DERIVED from the same expression, so the two cannot drift apart.
//
// Why halves and three-input operations: on gfx950 a plain 32-bit VOP1/VOP2 integer operation and v_bitop3_b32 hold the SIMD ~2.2 cycles
// per wave64 instruction, v_bfi_b32 / compares / v_cndmask_b32_e64 / left shifts / every 64-bit operation ~4.2 (profiles/r04_valu_peak.json).
// Written on 64-bit values the compiler makes `a | ~(b | c)` a v_or + v_bfi per half and the carry bits a compare + select; here a block
// costs three slow instructions (the 64-bit add and the two 64-bit shifts) and about two dozen fast ones.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OTG_STEP_HD __host__ __device__ __forceinline__
#else
#define OTG_STEP_HD inline
#endif

namespace otg_myers {

// The three-input combinations of the recurrence, as the expressions that document them.
struct XorOr { constexpr uint32_t operator()(uint32_t a, uint32_t b, uint32_t c) const { return (a ^ b) | c; } };      // Xh = (sum ^ Pv) | Eq
struct OrNor { constexpr uint32_t operator()(uint32_t a, uint32_t b, uint32_t c) const { return a | ~(b | c); } };     // Ph = Mv | ~(Xh | Pv),  Pv' = Mh | ~(Xv | Ph)

// Truth table of f for v_bitop3_b32: bit (4a + 2b + c) of the table is f(a, b, c), i.e. f evaluated on the three index columns.
template <class F> constexpr uint8_t truth_table() { return (uint8_t)(F{}(0xF0u, 0xCCu, 0xAAu) & 0xFFu); }

template <class F> OTG_STEP_HD uint32_t op3(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, truth_table<F>());
#else
  return F{}(a, b, c);
#endif
}

// a + b on register pairs: one v_lshl_add_u64 (the carry-chained pair of 32-bit adds costs twice that)
OTG_STEP_HD void add64(uint32_t& lo, uint32_t& hi, uint32_t alo, uint32_t ahi, uint32_t blo, uint32_t bhi)
{
  const uint64_t a = (uint64_t)ahi << 32 | alo, b = (uint64_t)bhi << 32 | blo;
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t s;
  asm("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(s) : "v"(a), "v"(b));
#else
  const uint64_t s = a + b;
#endif
  lo = (uint32_t)s; hi = (uint32_t)(s >> 32);
}

// (hi:lo << 1) | carry, carry in {0, 1}: one v_lshlrev_b64 on the pair and one v_or_b32.  Pinned on the device: left to itself the compiler
// splits the shift of a pair assembled from halves into v_lshlrev_b32 + v_alignbit / v_lshl_or per half.
OTG_STEP_HD void shl1_in(uint32_t& lo, uint32_t& hi, uint32_t carry)
{
  uint64_t v = (uint64_t)hi << 32 | lo;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_lshlrev_b64 %0, 1, %1" : "=v"(v) : "v"(v));
#else
  v <<= 1;
#endif
  lo = (uint32_t)v | carry; hi = (uint32_t)(v >> 32);
}

// One column of one block.  Pv / Mv: vertical +1 / -1 deltas of the previous column (bit r = row r of the block), updated in place to this
// column's; Eq: match mask of the column's text symbol; hin in {-1, 0, +1}: horizontal delta entering the block's top row.  Returns the
// horizontal delta leaving its bottom row.
OTG_STEP_HD int block_step(uint32_t& PvL, uint32_t& PvH, uint32_t& MvL, uint32_t& MvH, uint32_t EqL, uint32_t EqH, int hin)
{
  const uint32_t hneg = (uint32_t)hin >> 31;          // hin < 0
  int nh = -hin;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(nh));                                 // opaque: otherwise the sign test of -hin is rebuilt as v_cmp_lt + v_cndmask_b32_e64
#endif
  const uint32_t hpos = (uint32_t)nh >> 31;           // hin > 0
  const uint32_t XvL = EqL | MvL, XvH = EqH | MvH;
  EqL |= hneg;
  uint32_t sL, sH;
  add64(sL, sH, EqL & PvL, EqH & PvH, PvL, PvH);
  const uint32_t XhL = op3<XorOr>(sL, PvL, EqL), XhH = op3<XorOr>(sH, PvH, EqH);
  uint32_t PhL = op3<OrNor>(MvL, XhL, PvL), PhH = op3<OrNor>(MvH, XhH, PvH);
  uint32_t MhL = PvL & XhL, MhH = PvH & XhH;
  const int ho = (int)(PhH >> 31) - (int)(MhH >> 31);
  shl1_in(PhL, PhH, hpos);
  shl1_in(MhL, MhH, hneg);
  PvL = op3<OrNor>(MhL, XvL, PhL); PvH = op3<OrNor>(MhH, XvH, PhH);
  MvL = PhL & XvL; MvH = PhH & XvH;
  return ho;
}

} // namespace otg_myers

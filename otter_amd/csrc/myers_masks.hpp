// myers_masks.hpp — pattern match masks of the bit-parallel edit tiers, one 64-row block at a time.
//
// Shared by myers_edit.hip / pipeline.hip (device) and tests/edit_masks_host.cpp (host).  A block of 64 pattern bytes is described by
//   b0, b1   the two bit-planes of the code (byte >> 1) & 3 the tiers already use (A = 0, C = 1, T = 2, G = 3), over the rows that hold A C G T
//   ok       the rows that hold one of A C G T
//   ex       the rows that hold the pattern's one further byte value (e.g. N)
// and the five mask rows of the column step follow from them with bit operations (rows_from_planes).  The block builder sees the 64 bytes only
// through ballots — "which rows hold byte c" — so on the device a block costs one coalesced 64-byte load and a handful of compares into scalar
// register pairs (a wave64 compare IS a ballot), with no loop over the bases; the host test evaluates the same builder with a ballot that loops.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OTG_MASKS_HD __host__ __device__ __forceinline__
#else
#define OTG_MASKS_HD inline
#endif

namespace otg_myers {

// one block of the per-read table (16 bytes per 64 bases): the planes alone; ok = the block's rows, ex = 0 (flagged reads have no table use)
struct alignas(16) PlaneBlock { uint64_t b0, b1; };
// one block of a pair's own scratch (the in-kernel builder)
struct alignas(16) MaskBlock { uint64_t b0, b1, ok, ex; };

constexpr uint32_t NO_MASKS = 0xffffffffu;      // side-array entry of a task whose pattern has no table blocks

// the rows [0, m - 64 b) of block b that exist in a pattern of m bytes
OTG_MASKS_HD uint64_t block_rows(int m, int b)
{
  const int left = m - (b << 6);
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

// The planes of one block.  eq(c): bit r set iff row r exists and holds byte c.  rows: the rows that exist.  Returns the rows holding
// none of A C G T in *rest.
template <class Eq> OTG_MASKS_HD MaskBlock block_planes(Eq&& eq, uint64_t rows, uint64_t* rest)
{
  const uint64_t a = eq('A'), c = eq('C'), g = eq('G'), t = eq('T');
  MaskBlock k;
  k.b0 = c | g; k.b1 = t | g; k.ok = a | c | g | t; k.ex = 0;
  *rest = rows & ~k.ok;
  return k;
}

// The one-extra-symbol rule on top of block_planes: the first byte value outside A C G T met in a pattern becomes its extra symbol
// (*other, -1 before), a second one makes the pattern unsupported (*bad).  byte_at(r): the byte of row r.
template <class Eq, class At> OTG_MASKS_HD MaskBlock block_masks(Eq&& eq, At&& byte_at, uint64_t rows, int* other, bool* bad)
{
  uint64_t rest;
  MaskBlock k = block_planes(eq, rows, &rest);
  if (rest) {
    if (*other < 0) *other = (int)byte_at(__builtin_ctzll(rest));
    k.ex = eq((uint8_t)*other);
    if (rest & ~k.ex) *bad = true;
  }
  return k;
}

// the mask rows of the column step, in the order of the code: eq[0..3] = A C T G, eq[4] = the extra symbol.  The planes are zero outside
// ok, so only the A row (code 0) has to be cut to it.
OTG_MASKS_HD void rows_from_planes(uint64_t b0, uint64_t b1, uint64_t ok, uint64_t ex, uint64_t eq[5])
{
  eq[0] = ~(b1 | b0) & ok;
  eq[1] = ~b1 & b0;
  eq[2] = b1 & ~b0;
  eq[3] = b1 & b0;
  eq[4] = ex;
}

} // namespace otg_myers

// myers_masks.hpp — pattern match masks of the bit-parallel edit tiers, one 64-row block at a time.
//
// Shared by myers_edit.hip / pipeline.hip (device) and tests/edit_masks_host.cpp, tests/edit_text_codes_host.cpp (host).  A block of 64 pattern bytes is described by
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

// Row code of a text byte: 8 x the index of its mask row in the order below (A C T G = 0..3 by (byte >> 1) & 3), any other byte 5, the zero
// row.  It does not depend on the pair as long as the pattern has no extra symbol (row 4), which is the case of every pattern with table blocks.
constexpr uint32_t ZERO_ROW = 5;
OTG_MASKS_HD uint32_t text_row_code(uint32_t byte)
{
  const uint32_t sym = (byte >> 1) & 3u;
  return 8u * (byte == ((0x47544341u >> (8 * sym)) & 0xffu) ? sym : ZERO_ROW);
}

// The codes of eight bytes at once (byte k of the result = text_row_code(byte k of v)), on whole words: the symbol index of every byte, the
// letter that index stands for (A 0x41, C 0x43, T 0x54, G 0x47: bit 6, the index in bits 1-2, bit 4 for T, bit 0 for the others), and the
// zero row where the byte is not that letter.  No operation carries from one byte into the next.
OTG_MASKS_HD uint64_t text_row_codes8(uint64_t v)
{
  constexpr uint64_t B = 0x0101010101010101ull;
  const uint64_t s = (v >> 1) & (3 * B);
  const uint64_t t = (s >> 1) & ~s & B;                                                  // 1 where the index is 2 (T)
  const uint64_t diff = v ^ ((0x40 * B) | (s << 1) | (t << 4) | (t ^ B));
  const uint64_t other = ((((diff & (0x7f * B)) + (0x7f * B)) | diff) >> 7 & B) * 0xff;  // 0xff where the byte is not its index's letter
  return ((s << 3) & ~other) | ((8 * ZERO_ROW * B) & other);
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

#if defined(__HIPCC__)
// One wave passes over a read of m bytes eight bytes per lane (unaligned 8-byte loads and stores; the last m % 8 bytes one per lane) and
// writes its row codes to codes[0, m) and / or the bytes themselves to copy[0, m); either may be null.  REV: the read is taken from its
// other end, byte j of it is src[m - 1 - j] (the eight bytes of a load turned round: two v_perm_b32).
template <bool REV> __device__ __forceinline__ void wave_read_codes(const uint8_t* __restrict__ src, int m, int lane, uint8_t* __restrict__ copy, uint8_t* __restrict__ codes)
{
  const int n8 = m >> 3;
  for (int c = lane; c < n8; c += 64) {
    uint64_t v;
    __builtin_memcpy(&v, REV ? src + (m - 8 * c - 8) : src + 8 * c, 8);
    if (REV) v = __builtin_bswap64(v);
    if (copy) __builtin_memcpy(copy + 8 * c, &v, 8);
    if (codes) { const uint64_t k = text_row_codes8(v); __builtin_memcpy(codes + 8 * c, &k, 8); }
  }
  const int j = 8 * n8 + lane;
  if (j < m) {
    const uint8_t b = REV ? src[m - 1 - j] : src[j];
    if (copy) copy[j] = b;
    if (codes) codes[j] = (uint8_t)text_row_code(b);
  }
}

// The table blocks of one read, by one wave: lane r holds row r of a block (byte_at(j): byte j of the read, j < m), four blocks in flight.
// Block b lands at out[b], kept by lane (b & 63) and stored 64 at a time (out may be null).  Returns whether the read holds a byte outside
// A C G T: such a read has no table use.
template <class At> __device__ __forceinline__ bool wave_read_planes(At&& byte_at, int m, int lane, PlaneBlock* __restrict__ out)
{
  const int nb = (m + 63) >> 6;
  uint64_t flagged = 0, k0 = 0, k1 = 0;
  for (int b4 = 0; b4 < nb; b4 += 4) {
    uint32_t ch[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int j = ((b4 + k) << 6) + lane; ch[k] = j < m ? (uint32_t)byte_at(j) : 0u; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int b = b4 + k;
      if (b >= nb) break;
      const uint64_t rows = block_rows(m, b);
      const uint32_t c = ch[k];
      uint64_t rest;
      const MaskBlock mk = block_planes([&](uint8_t v) { return __ballot(c == (uint32_t)v) & rows; }, rows, &rest);
      flagged |= rest;
      if (lane == (b & 63)) { k0 = mk.b0; k1 = mk.b1; }
      if (out && ((b & 63) == 63 || b == nb - 1)) { if (lane <= (b & 63)) out[(b & ~63) + lane] = PlaneBlock{k0, k1}; }
    }
  }
  return flagged != 0;
}
#endif

} // namespace otg_myers

// Host check of otter_amd/csrc/myers_masks.hpp (built by tests/test_edit_masks_host.py, with -fsanitize=address,undefined):
// the block builder (block_planes / block_masks, driven by a ballot that loops over the rows) and the plane-to-row derivation
// (rows_from_planes) against the per-base definition of the five mask rows, on random byte strings of lengths 0..200 that
// include bytes outside A C G T, lower-case letters and the zero byte.
// stdout: "strings <n> blocks <n> flagged <n> one_extra <n> unsupported <n>"; exit status 1 with a message on the first difference.
#include "myers_masks.hpp"
#include <cstdio>
#include <string>
#include <vector>

using namespace otg_myers;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 24); }

// the per-base definition: rows A C T G (the order of the code (byte >> 1) & 3) and the row of the one extra symbol; the extra symbol is
// the first byte outside A C G T, a second distinct one makes the pattern unsupported
struct Ref { std::vector<uint64_t> row[5]; int other = -1; bool bad = false; };

static Ref per_base(const std::string& s)
{
  const int m = (int)s.size(), nblk = (m + 63) / 64;
  Ref R;
  for (auto& r : R.row) r.assign(nblk, 0);
  for (int i = 0; i < m; ++i) {
    const uint8_t ch = (uint8_t)s[i];
    if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') continue;
    if (R.other < 0) R.other = ch; else if (R.other != ch) R.bad = true;
  }
  for (int i = 0; i < m; ++i) {
    const uint8_t ch = (uint8_t)s[i];
    const uint64_t bit = 1ull << (i & 63);
    if (ch == 'A') R.row[0][i >> 6] |= bit;
    else if (ch == 'C') R.row[1][i >> 6] |= bit;
    else if (ch == 'T') R.row[2][i >> 6] |= bit;
    else if (ch == 'G') R.row[3][i >> 6] |= bit;
    else if ((int)ch == R.other) R.row[4][i >> 6] |= bit;
  }
  return R;
}

static bool check(const std::string& s, long& blocks, long& flagged, long& one_extra, long& unsupported)
{
  const int m = (int)s.size(), nblk = (m + 63) / 64;
  const Ref R = per_base(s);
  // the in-kernel builder: block_masks over the blocks in order, then the rows
  int other = -1; bool bad = false; uint64_t any_rest = 0;
  std::vector<MaskBlock> mk(nblk);
  std::vector<PlaneBlock> tab(nblk);
  for (int b = 0; b < nblk; ++b) {
    const uint64_t rows = block_rows(m, b);
    const int left = m - 64 * b < 64 ? m - 64 * b : 64;
    if (rows != (left == 64 ? ~0ull : (1ull << left) - 1)) { std::printf("block_rows(%d, %d)\n", m, b); return false; }
    auto eq = [&](uint8_t v) { uint64_t r = 0; for (int l = 0; l < left; ++l) if ((uint8_t)s[64 * b + l] == v) r |= 1ull << l; return r; };
    auto at = [&](int r) { return (uint32_t)(uint8_t)s[64 * b + r]; };
    mk[b] = block_masks(eq, at, rows, &other, &bad);
    uint64_t rest;
    const MaskBlock pl = block_planes(eq, rows, &rest);        // the table builder
    tab[b] = PlaneBlock{pl.b0, pl.b1};
    any_rest |= rest;
    ++blocks;
  }
  if (bad != R.bad) { std::printf("m %d: bad %d, per-base %d\n", m, (int)bad, (int)R.bad); return false; }
  if (other != R.other) { std::printf("m %d: extra symbol %d, per-base %d\n", m, other, R.other); return false; }
  if ((any_rest != 0) != (R.other >= 0)) { std::printf("m %d: flag %d, per-base %d\n", m, (int)(any_rest != 0), (int)(R.other >= 0)); return false; }
  if (bad) { ++unsupported; return true; }                    // such a pattern goes to the wavefront kernel: its masks are never read
  for (int b = 0; b < nblk; ++b) {
    uint64_t rows5[5];
    rows_from_planes(mk[b].b0, mk[b].b1, mk[b].ok, mk[b].ex, rows5);
    for (int y = 0; y < 5; ++y)
      if (rows5[y] != R.row[y][b]) { std::printf("m %d block %d row %d: built %016llx, per-base %016llx\n", m, b, y, (unsigned long long)rows5[y], (unsigned long long)R.row[y][b]); return false; }
    if (any_rest == 0) {                                        // an unflagged read: the table's planes, ok = the block's rows, no extra symbol
      rows_from_planes(tab[b].b0, tab[b].b1, block_rows(m, b), 0ull, rows5);
      for (int y = 0; y < 5; ++y)
        if (rows5[y] != R.row[y][b]) { std::printf("m %d block %d row %d (table): derived %016llx, per-base %016llx\n", m, b, y, (unsigned long long)rows5[y], (unsigned long long)R.row[y][b]); return false; }
    }
  }
  if (any_rest) ++flagged;
  if (other >= 0) ++one_extra;
  return true;
}

int main()
{
  static const char acgt[] = "ACGT";
  static const uint8_t odd[] = {'N', 'a', 'c', 'g', 't', 'n', 0, 0xff, 'B', 'U', '@', 'E'};      // neighbours of A C G T in the code, case, extremes
  long strings = 0, blocks = 0, flagged = 0, one_extra = 0, unsupported = 0;
  for (int m = 0; m <= 200; ++m) {
    for (int rep = 0; rep < 24; ++rep) {
      std::string s(m, 'A');
      for (auto& c : s) c = acgt[rnd() & 3];
      // rep 0..7: A C G T only; 8..15: one extra byte value at 1..3 places; 16..23: bytes drawn freely (mostly unsupported)
      if (rep >= 8 && rep < 16 && m > 0) {
        const char x = (char)odd[rnd() % sizeof(odd)];
        for (int k = 0, nk = 1 + (int)(rnd() % 3); k < nk; ++k) s[rnd() % m] = x;
      } else if (rep >= 16 && m > 0) {
        for (int k = 0, nk = 1 + (int)(rnd() % 4); k < nk; ++k) s[rnd() % m] = (rep & 1) ? (char)odd[rnd() % sizeof(odd)] : (char)(rnd() & 0xff);
      }
      if (!check(s, blocks, flagged, one_extra, unsupported)) return 1;
      ++strings;
    }
    // the last row of a block, the first of the next
    if (m >= 1) { std::string s(m, 'G'); s[m - 1] = 'N'; if (!check(s, blocks, flagged, one_extra, unsupported)) return 1; ++strings; }
    if (m >= 65) { std::string s(m, 'T'); s[63] = 'N'; s[64] = 'N'; if (!check(s, blocks, flagged, one_extra, unsupported)) return 1; ++strings; }
  }
  std::printf("strings %ld blocks %ld flagged %ld one_extra %ld unsupported %ld\n", strings, blocks, flagged, one_extra, unsupported);
  return 0;
}

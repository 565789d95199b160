// Host check of the text row codes of otter_amd/csrc/myers_masks.hpp (built by tests/test_edit_text_codes_host.py, with
// -fsanitize=address,undefined): text_row_code against the definition of the code on all 256 byte values; text_row_codes8 against
// text_row_code on every byte value in every position of a word beside random neighbours, and on random words; and, for random byte strings
// of lengths 1 to 200 with bytes outside A C G T, the reversed copy as the device makes it — eight bytes at a time from the read's other end,
// turned round, the last length % 8 bytes one by one — against the reversed bytes, its codes against the definition, and its table blocks
// against those of the read, row j against row length - 1 - j.
#include "myers_masks.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace otg_myers;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint32_t code_by_definition(uint32_t b)
{
  switch (b) { case 'A': return 0; case 'C': return 8; case 'T': return 16; case 'G': return 24; default: return 40; }
}

// the blocks of a byte string, with a ballot that loops over the rows
static std::vector<MaskBlock> blocks_of(const std::vector<uint8_t>& s, bool* flagged)
{
  const int m = (int)s.size();
  std::vector<MaskBlock> out;
  *flagged = false;
  for (int b = 0; b < (m + 63) / 64; ++b) {
    const uint64_t rows = block_rows(m, b);
    uint64_t rest;
    out.push_back(block_planes([&](uint8_t v) { uint64_t q = 0; for (int r = 0; r < 64 && 64 * b + r < m; ++r) if (s[64 * b + r] == v) q |= 1ull << r; return q & rows; }, rows, &rest));
    if (rest) *flagged = true;
  }
  return out;
}

int main()
{
  std::mt19937_64 rng(20261020);
  for (uint32_t b = 0; b < 256; ++b) CHECK(text_row_code(b) == code_by_definition(b), "text_row_code(%u) = %u", b, text_row_code(b));
  long words = 0;
  for (int pos = 0; pos < 8; ++pos)
    for (uint32_t b = 0; b < 256; ++b)
      for (int rep = 0; rep < 8; ++rep) {
        uint64_t v = rep == 0 ? 0ull : rep == 1 ? ~0ull : rng();
        v = (v & ~(0xffull << (8 * pos))) | ((uint64_t)b << (8 * pos));
        const uint64_t k = text_row_codes8(v);
        for (int i = 0; i < 8; ++i) CHECK(((k >> (8 * i)) & 0xff) == text_row_code((uint32_t)(v >> (8 * i)) & 0xff), "codes8 byte %d of %016llx", i, (unsigned long long)v);
        ++words;
      }
  const char letters[] = "ACGTACGTACGTACGTNRacgt";
  long strings = 0, flagged_strings = 0;
  for (int m = 1; m <= 200; ++m)
    for (int rep = 0; rep < 12; ++rep) {
      std::vector<uint8_t> s(m);
      const bool pure = rep % 3 != 0;
      for (auto& c : s) c = (uint8_t)letters[rng() % (pure ? 16 : sizeof(letters) - 1)];
      // the device's way: chunk c of the copy is the eight bytes src[m - 8c - 8 .. m - 8c - 1] turned round, the last m % 8 bytes one by one
      std::vector<uint8_t> copy(m, 0xee), codes(m, 0xee);
      const int n8 = m >> 3;
      for (int c = 0; c < n8; ++c) {
        uint64_t v;
        std::memcpy(&v, s.data() + (m - 8 * c - 8), 8);
        v = __builtin_bswap64(v);
        std::memcpy(copy.data() + 8 * c, &v, 8);
        const uint64_t k = text_row_codes8(v);
        std::memcpy(codes.data() + 8 * c, &k, 8);
      }
      for (int j = 8 * n8; j < m; ++j) { copy[j] = s[m - 1 - j]; codes[j] = (uint8_t)text_row_code(copy[j]); }
      const std::vector<uint8_t> rev(s.rbegin(), s.rend());
      CHECK(copy == rev, "reversed copy, m = %d", m);
      for (int j = 0; j < m; ++j) CHECK(codes[j] == code_by_definition(rev[j]), "reversed code %d of %d", j, m);
      // its blocks: row j of the reversed read is row m - 1 - j of the read, plane by plane
      bool f_rev, f_fwd;
      const std::vector<MaskBlock> r = blocks_of(copy, &f_rev), f = blocks_of(s, &f_fwd);
      CHECK(f_rev == f_fwd && f_fwd == !std::all_of(s.begin(), s.end(), [](uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }), "flag, m = %d", m);
      for (int j = 0; j < m; ++j) {
        const int i = m - 1 - j;
        CHECK(((r[j >> 6].b0 >> (j & 63)) & 1) == ((f[i >> 6].b0 >> (i & 63)) & 1) && ((r[j >> 6].b1 >> (j & 63)) & 1) == ((f[i >> 6].b1 >> (i & 63)) & 1) &&
              ((r[j >> 6].ok >> (j & 63)) & 1) == ((f[i >> 6].ok >> (i & 63)) & 1), "row %d of the reversed read, m = %d", j, m);
      }
      const bool f1 = f_rev;
      ++strings; flagged_strings += f1;
    }
  std::printf("words %ld strings %ld flagged %ld fails %d\n", words, strings, flagged_strings, fails);
  return fails ? 1 : 0;
}

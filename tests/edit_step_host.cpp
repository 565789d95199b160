// Host check of otter_amd/csrc/myers_step.hpp (built by tests/test_edit_step_host.py, with -fsanitize=address,undefined):
// block_step() driven column by column over whole pairs, every value of the last column against a textbook O(mn) DP.
// Also prints the truth tables derived for the three-input operations, and checks them against the expressions bit by bit.
// stdout: "table <name> 0x..", then "pairs <n> columns <n>"; exit status 1 with a message on the first difference.
#include "myers_step.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace otg_myers;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 24); }

// D[i][n] for i = 0..m, with D[i][0] = max(0, i - pbf) (pbf rows of the pattern free at the beginning) and D[0][j] = j
static std::vector<int> dp_last_column(const std::string& p, const std::string& t, int pbf)
{
  const int m = (int)p.size(), n = (int)t.size();
  std::vector<int> col(m + 1), nxt(m + 1);
  for (int i = 0; i <= m; ++i) col[i] = std::max(0, i - pbf);
  for (int j = 1; j <= n; ++j) {
    nxt[0] = j;
    for (int i = 1; i <= m; ++i) nxt[i] = std::min({col[i] + 1, nxt[i - 1] + 1, col[i - 1] + (p[i - 1] != t[j - 1])});
    col.swap(nxt);
  }
  return col;
}

static bool check_pair(const std::string& p, const std::string& t, int pbf, long& columns)
{
  const int m = (int)p.size(), n = (int)t.size(), nblk = (m + 63) / 64;
  std::vector<uint32_t> PvL(nblk), PvH(nblk), MvL(nblk, 0), MvH(nblk, 0);
  for (int b = 0; b < nblk; ++b) {                    // first column: vertical delta +1 for rows i > pbf
    const int z = pbf - 64 * b;
    const uint64_t pv = z <= 0 ? ~0ull : (z >= 64 ? 0ull : (~0ull << z));
    PvL[b] = (uint32_t)pv; PvH[b] = (uint32_t)(pv >> 32);
  }
  int score = std::max(0, 64 * nblk - pbf);           // D[64 nblk][0]; rows past m match nothing and are ignored below
  for (int j = 0; j < n; ++j) {
    int h = 1;                                        // D[0][j+1] - D[0][j]
    for (int b = 0; b < nblk; ++b) {
      uint64_t eq = 0;
      for (int r = 0; r < 64 && 64 * b + r < m; ++r) if (p[64 * b + r] == t[j]) eq |= 1ull << r;
      h = block_step(PvL[b], PvH[b], MvL[b], MvH[b], (uint32_t)eq, (uint32_t)(eq >> 32), h);
      if (h < -1 || h > 1) { std::printf("horizontal delta %d out of range\n", h); return false; }
    }
    score += h;
    ++columns;
  }
  const std::vector<int> ref = dp_last_column(p, t, pbf);
  int sc = score;
  for (int i = 64 * nblk; i >= 1; --i) {
    if (i <= m && sc != ref[i]) {
      std::printf("m %d n %d pbf %d row %d: got %d, DP %d\n", m, n, pbf, i, sc, ref[i]);
      return false;
    }
    const int b = (i - 1) / 64, r = (i - 1) % 64;
    const uint64_t pv = (uint64_t)PvH[b] << 32 | PvL[b], mv = (uint64_t)MvH[b] << 32 | MvL[b];
    if ((pv >> r) & (mv >> r) & 1ull) { std::printf("row %d: +1 and -1 both set\n", i); return false; }
    sc -= (int)((pv >> r) & 1ull) - (int)((mv >> r) & 1ull);
  }
  if (sc != (n > 0 ? n : 0)) { std::printf("m %d n %d: row 0 reads %d\n", m, n, sc); return false; }
  return true;
}

static std::string rand_seq(int L, int alphabet) { std::string s(L, 'A'); for (auto& c : s) c = "ACGTN"[rnd() % alphabet]; return s; }

static std::string mutate(const std::string& a, int per_mille)
{
  std::string b;
  for (char c : a) {
    const uint32_t x = rnd() % 1000;
    if (x < (uint32_t)per_mille / 3) continue;                                        // deletion
    if (x < 2 * (uint32_t)per_mille / 3) { b += "ACGT"[rnd() % 4]; b += c; continue; }   // insertion
    if (x < (uint32_t)per_mille) { b += "ACGT"[rnd() % 4]; continue; }                // substitution
    b += c;
  }
  return b.empty() ? std::string("A") : b;
}

template <class F> static bool table_ok(const char* name)
{
  constexpr uint8_t tt = truth_table<F>();
  std::printf("table %s 0x%02x\n", name, tt);
  for (uint32_t a = 0; a < 2; ++a) for (uint32_t b = 0; b < 2; ++b) for (uint32_t c = 0; c < 2; ++c)
    if (((tt >> (4 * a + 2 * b + c)) & 1u) != (F{}(a, b, c) & 1u)) { std::printf("table %s: entry %u%u%u\n", name, a, b, c); return false; }
  return true;
}

int main()
{
  if (!table_ok<XorOr>("(a^b)|c") || !table_ok<OrNor>("a|~(b|c)")) return 1;
  long pairs = 0, columns = 0;
  auto run = [&](const std::string& p, const std::string& t, int pbf) { ++pairs; if (!check_pair(p, t, pbf, columns)) std::exit(1); };
  const int edges[] = {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300};
  for (int m : edges) {
    for (int d : {0, 1, 2, 31, 63, 64, 65}) {
      const int n = m - d;
      if (n < 1) continue;
      run(std::string(m, 'A'), std::string(n, 'A'), 0);            // every mask bit set: the add's carry runs through the whole block and out of it
      run(std::string(m, 'A'), std::string(n, 'C'), 0);            // no match at all
      const std::string r = rand_seq(m, 4);
      run(r, r.substr(0, n), 0);
      run(r, r.substr(d), d);                                      // free pattern prefix
      run(r, r.substr(d), d / 2);
      run(r, rand_seq(n, 4), 0);
    }
    const std::string r = rand_seq(m, 4);
    for (int row : {0, 30, 31, 32, 62, 63, 64, 65, 127, 128}) {   // one edit at a half-word / block edge
      if (row >= m) continue;
      std::string s = r; s[row] = s[row] == 'A' ? 'C' : 'A'; run(r, s, 0);
      s = r; s.erase(row, 1); if (!s.empty()) { run(r, s, 0); run(s, r, 0); }
    }
    std::string withn = r; withn[m / 2] = 'N'; run(withn, r, 0);   // a fifth symbol in the pattern
  }
  for (int it = 0; it < 400; ++it) {
    const int m = 1 + (int)(rnd() % 300);
    const std::string a = rand_seq(m, it % 3 ? 4 : (it % 2 ? 2 : 5));
    const std::string b = it % 4 == 3 ? rand_seq(1 + (int)(rnd() % 300), 4) : mutate(a, (int)(rnd() % 400));
    run(a, b, it % 5 == 0 ? (int)(rnd() % (m + 1)) : 0);
  }
  std::printf("pairs %ld columns %ld\n", pairs, columns);
  return 0;
}

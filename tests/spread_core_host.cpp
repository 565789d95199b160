// spread_core_host.cpp — the selection routine of otter_amd/csrc/otg_spread_core.hpp on the host, in the kernel's schedule: a wave of 64
// emulated lanes, the members of an allele spread over the strides of its region with absent lanes between them, the register tier
// (at most SP_REG_STRIDES strides held as an array of strides) and the re-read tier (a loader asked again on every pass), against
// std::sort with the rule's indexing.  Stand-alone: its own main, no input; prints the number of cases and exits 0, or names the first
// difference and exits 1.  Built by tests/test_spread_host.py with -fsanitize=address,undefined.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "otg_spread_core.hpp"

using namespace otg_spread_core;

struct HostWave {
  using Vec = std::array<uint32_t, 64>;
  uint32_t count_le(const Vec& v, uint32_t x) const
  {
    uint32_t c = 0;
    for (uint32_t l = 0; l < 64; ++l) c += v[l] <= x;
    return c;
  }
};

struct HostLoad {
  const std::vector<uint32_t>& slots;                               // the region's reads: a member's value or SP_ABSENT
  mutable uint64_t loads = 0;
  HostWave::Vec operator()(uint32_t s) const
  {
    HostWave::Vec v;
    for (uint32_t l = 0; l < 64; ++l) {
      const size_t i = (size_t)s * 64 + l;
      v[l] = i < slots.size() ? slots[i] : SP_ABSENT;
    }
    ++loads;
    return v;
  }
};

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}

static int check(const char* what, uint32_t m, int gap, const std::vector<uint32_t>& values, unsigned* n_reg, unsigned* n_load)
{
  // the region: the members in order, `gap` absent reads after every second member (gap = 0: the members alone)
  std::vector<uint32_t> slots;
  for (uint32_t i = 0; i < m; ++i) {
    slots.push_back(values[i]);
    if (gap && (i & 1u)) for (int g = 0; g < gap; ++g) slots.push_back(SP_ABSENT);
  }
  std::vector<uint32_t> sorted(values.begin(), values.begin() + m);
  std::sort(sorted.begin(), sorted.end());
  uint32_t want[5] = {0, 0, 0, 0, 0};
  for (uint32_t j = 0; j < 5 && m; ++j) want[j] = sorted[(size_t)((uint64_t)j * (m - 1) / 4)];
  const HostWave w{};
  const uint32_t n_strides = (uint32_t)((slots.size() + 63) / 64);
  HostLoad load{slots};
  uint32_t q[5];
  sp_quantiles_load<HostWave, HostLoad>(w, load, n_strides, m, q);
  ++*n_load;
  for (int j = 0; j < 5; ++j)
    if (q[j] != want[j]) { printf("re-read tier: %s m=%u gap=%d q[%d] = %u, expected %u\n", what, m, gap, j, q[j], want[j]); return 1; }
  if (m && load.loads != (uint64_t)SP_BITS * n_strides) { printf("re-read tier: %s m=%u: %llu loads\n", what, m, (unsigned long long)load.loads); return 1; }
  if (n_strides <= (uint32_t)SP_REG_STRIDES) {
    HostWave::Vec v[SP_REG_STRIDES];
    for (int s = 0; s < SP_REG_STRIDES; ++s) v[s] = load((uint32_t)s);
    sp_quantiles_reg<HostWave, SP_REG_STRIDES>(w, v, m, q);
    ++*n_reg;
    for (int j = 0; j < 5; ++j)
      if (q[j] != want[j]) { printf("register tier: %s m=%u gap=%d q[%d] = %u, expected %u\n", what, m, gap, j, q[j], want[j]); return 1; }
  }
  return 0;
}

int main()
{
  const uint32_t R64 = 64u * SP_REG_STRIDES;
  const uint32_t counts[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, R64, R64 + 1, 1000};
  unsigned n_reg = 0, n_load = 0, n_reg_full = 0;
  for (uint32_t m : counts) {
    for (int gap : {0, 1, 3}) {
      std::vector<uint32_t> v(m ? m : 1);
      for (auto& x : v) x = 417u;
      if (check("all equal", m, gap, v, &n_reg, &n_load)) return 1;
      for (auto& x : v) x = (rnd() & 1u) ? 90u : 93u;
      if (check("two distinct", m, gap, v, &n_reg, &n_load)) return 1;
      for (auto& x : v) x = 65536u - 3u + rnd() % 7u;                // 65533 .. 65539
      if (check("around 2^16", m, gap, v, &n_reg, &n_load)) return 1;
      for (auto& x : v) x = rnd() & ((1u << SP_BITS) - 1u);
      if (m > 1) { v[0] = (1u << SP_BITS) - 1u; v[1] = 0u; }
      else if (m == 1) v[0] = (1u << SP_BITS) - 1u;
      if (check("up to 2^21 - 1", m, gap, v, &n_reg, &n_load)) return 1;
      for (auto& x : v) x = rnd() % 40u;                             // many ties
      if (check("small with ties", m, gap, v, &n_reg, &n_load)) return 1;
    }
    n_reg_full += m == R64;
  }
  // both tiers ran, the register tier at its last size and the re-read tier just above it
  if (n_reg == 0 || n_load == 0 || n_reg_full != 1 || n_reg >= n_load) { printf("the tiers did not both run (%u, %u)\n", n_reg, n_load); return 1; }
  printf("ok %u %u\n", n_reg, n_load);
  return 0;
}

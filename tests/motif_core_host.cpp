// motif_core_host.cpp — the arithmetic of the motif kernels (otter_amd/csrc/otg_motif_core.hpp) on the host, in the kernels' schedule:
// 256 "threads" that take strided words / periods / rotation offsets, then the reduction tree of motif.hip.  A stand-alone program (built
// with -fsanitize=address,undefined by tests/test_motif_host.py): reads lines "max_period slack hex-bytes" and prints per line
// "period matches compared best_period flags hex-unit".  The planes are allocated with exactly the words the kernels give them and the
// sequence with exactly the 64 slack bytes the arenas have, so an index beyond either is reported by the sanitizer.
#include "otg_motif_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace otg_motif_core;

struct Result { uint32_t period = 0, matches = 0, compared = 0, best = 0, flags = 0; std::string unit; };

static Result annotate(const std::vector<uint8_t>& arena, uint32_t L, uint32_t max_period, uint32_t slack)
{
  Result R;
  const uint8_t* s = arena.data();
  if (L > OTG_MOTIF_MAX_LEN) R.flags = OTG_MOTIF_TOO_LONG;
  const uint32_t P = mo_period_range(L, max_period);
  if (P == 0) return R;
  // pack: thread t takes the words t, t + 256, ... of W + 2
  const uint32_t W = (L + 31u) >> 5;
  std::vector<uint32_t> LO(W + 2), HI(W + 2), V(W + 2);
  for (uint32_t t = 0; t < MOTIF_T; ++t)
    for (uint32_t w = t; w < W + 2u; w += MOTIF_T) {
      uint32_t l = 0, h = 0, v = 0;
      if (w < W) mo_pack_word(s, L, w, &l, &h, &v);
      LO[w] = l; HI[w] = h; V[w] = v;
    }
  std::vector<uint32_t> m(P);
  for (uint32_t p = 1; p <= P; ++p) m[p - 1] = mo_count(LO.data(), HI.data(), V.data(), L, p);
  // best: strided scans, then the tree
  uint32_t red_p[MOTIF_T], red_m[MOTIF_T];
  for (uint32_t t = 0; t < MOTIF_T; ++t) {
    uint32_t bp = 0, bm = 0;
    for (uint32_t p = 1u + t; p <= P; p += MOTIF_T)
      if (mo_better(L, p, m[p - 1], bp, bm)) { bp = p; bm = m[p - 1]; }
    red_p[t] = bp; red_m[t] = bm;
  }
  for (uint32_t d = MOTIF_T / 2; d > 0; d >>= 1)
    for (uint32_t t = 0; t < d; ++t)
      if (mo_better(L, red_p[t + d], red_m[t + d], red_p[t], red_m[t])) { red_p[t] = red_p[t + d]; red_m[t] = red_m[t + d]; }
  const uint32_t best = red_p[0], mbest = red_m[0];
  if (mbest == 0) return R;
  uint32_t period = best;
  for (uint32_t t = 0; t < MOTIF_T; ++t)
    for (uint32_t p = 1u + t; p <= best; p += MOTIF_T)
      if (mo_within_slack(L, p, m[p - 1], best, mbest, slack)) { if (p < period) period = p; break; }
  // unit: the two phase-count schedules of the kernel
  std::vector<uint8_t> unit(period);
  if (period <= (uint32_t)MOTIF_T) {
    const uint32_t k = MOTIF_T / period;
    std::vector<uint32_t> cnt((size_t)period * 4, 0u);
    for (uint32_t t = 0; t < MOTIF_T; ++t) {
      const uint32_t j = t % period, r = t / period;
      if (r >= k) continue;
      for (uint64_t i = j + (uint64_t)period * r; i < L; i += (uint64_t)period * k) { const uint32_t c = mo_code(s[i]); if (c < 4) ++cnt[(size_t)j * 4 + c]; }
    }
    for (uint32_t j = 0; j < period; ++j) unit[j] = mo_majority(cnt[j * 4], cnt[j * 4 + 1], cnt[j * 4 + 2], cnt[j * 4 + 3]);
  } else {
    for (uint32_t j = 0; j < period; ++j) {
      uint32_t c[4] = {0, 0, 0, 0};
      for (uint32_t i = j; i < L; i += period) { const uint32_t code = mo_code(s[i]); if (code < 4) ++c[code]; }
      unit[j] = mo_majority(c[0], c[1], c[2], c[3]);
    }
  }
  for (uint32_t t = 0; t < MOTIF_T; ++t) {
    uint32_t rot = t < period ? t : 0u;
    for (uint32_t o = t + MOTIF_T; o < period; o += MOTIF_T)
      if (mo_rot_less(unit.data(), period, o, rot)) rot = o;
    red_p[t] = rot;
  }
  for (uint32_t d = MOTIF_T / 2; d > 0; d >>= 1)
    for (uint32_t t = 0; t < d; ++t)
      if (mo_rot_less(unit.data(), period, red_p[t + d], red_p[t])) red_p[t] = red_p[t + d];
  const uint32_t rot = red_p[0];
  R.period = period; R.matches = m[period - 1]; R.compared = L - period; R.best = best;
  for (uint32_t i = 0; i < period; ++i) R.unit.push_back((char)unit[(rot + i) % period]);
  return R;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    uint32_t max_period = 0, slack = 0;
    std::string hex;
    in >> max_period >> slack >> hex;
    if (hex == "-") hex.clear();
    const uint32_t L = (uint32_t)(hex.size() / 2);
    std::vector<uint8_t> arena((size_t)L + 64, 0);
    for (uint32_t i = 0; i < L; ++i) arena[i] = (uint8_t)strtoul(hex.substr(2 * (size_t)i, 2).c_str(), nullptr, 16);
    const Result R = annotate(arena, L, max_period, slack);
    printf("%u %u %u %u %u ", R.period, R.matches, R.compared, R.best, R.flags);
    if (R.unit.empty()) printf("-");
    for (unsigned char c : R.unit) printf("%02x", c);
    printf("\n");
  }
  return 0;
}

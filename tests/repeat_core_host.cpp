// repeat_core_host.cpp — the arithmetic of the repeat kernels (otter_amd/csrc/otg_repeat_core.hpp) on the host, in the kernels' schedule:
// 256 "threads" that take strided words / periods / runs / unit offsets, the two passes of the run extraction around their scans, then the
// parse of repeat.hip with its reduction trees.  A stand-alone program (built with -fsanitize=address,undefined by
// tests/test_repeat_host.py): reads lines "max_period min_copies min_span hex-bytes" and prints per line
// "flags n_repeats covered n_segments begin,period,copies,length ...".  The planes, the runs, the stack and the segment scratch are
// allocated with exactly the sizes the kernels give them, the sequence with the 64 slack bytes the arenas have, so an index beyond any of
// them is reported by the sanitizer.
#include "otg_repeat_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace otg_repeat_core;

struct Seg { uint32_t begin, period, copies, length; };
struct Result { uint32_t flags = 0, n_repeats = 0, covered = 0; std::vector<Seg> segs; };

static Result parse(const std::vector<uint8_t>& arena, uint32_t L, uint32_t max_period, uint32_t min_copies, uint32_t min_span)
{
  Result out;
  const uint8_t* s = arena.data();
  if (L > OTG_REPEAT_MAX_LEN) out.flags = OTG_REPEAT_TOO_LONG;
  if (L == 0) return out;
  const uint32_t P = rp_period_range(L, max_period);
  // pack: thread t takes the words t, t + 256, ... of W + 2
  const uint32_t W = (L + 31u) >> 5;
  std::vector<uint32_t> LO(W + 2), HI(W + 2), V(W + 2);
  for (uint32_t t = 0; t < REPEAT_T; ++t)
    for (uint32_t w = t; w < W + 2u; w += REPEAT_T) {
      uint32_t l = 0, h = 0, v = 0;
      if (w < W && P) mo_pack_word(s, L, w, &l, &h, &v);
      LO[w] = l; HI[w] = h; V[w] = v;
    }
  // the counting pass, the scan of the counts, the writing pass (only the periods that keep a run)
  std::vector<uint32_t> cnt(P), pre(P);
  for (uint32_t p = 1; p <= P; ++p) {
    const uint32_t min_len = rp_min_len(p, min_copies, min_span);
    cnt[p - 1] = L >= min_len ? rp_runs(LO.data(), HI.data(), V.data(), L, p, min_len, nullptr) : 0u;
  }
  uint32_t K = 0;
  for (uint32_t p = 0; p < P; ++p) { pre[p] = K; K += cnt[p]; }
  std::vector<RpRun> R(K);
  for (uint32_t p = 1; p <= P; ++p)
    if (cnt[p - 1]) {
      const uint32_t got = rp_runs(LO.data(), HI.data(), V.data(), L, p, rp_min_len(p, min_copies, min_span), R.data() + pre[p - 1]);
      if (got != cnt[p - 1]) { fprintf(stderr, "the two passes disagree at p = %u\n", p); exit(2); }
    }
  // the parse
  std::vector<uint32_t> st_run(K), st_h(K);
  std::vector<Seg> SG((size_t)2 * K + 1);
  const uint32_t cap = 2u * K + 1u;
  uint32_t x = 0, H = L, depth = 0, prev_p = 0, prev_b = 0, lit_b = 0, lit_len = 0, nseg = 0;
  auto emit = [&](uint32_t begin, uint32_t period, uint32_t copies, uint32_t length) {
    if (nseg >= cap) { fprintf(stderr, "more than 2 K + 1 segments\n"); exit(3); }
    SG[nseg++] = Seg{begin, period, copies, length};
  };
  RpCand red[REPEAT_T];
  uint32_t red_t[REPEAT_T];
  for (;;) {
    for (uint32_t t = 0; t < REPEAT_T; ++t) {
      RpCand c = {0u, 0u, 0u, 0u, 0u};
      for (uint32_t i = t; i < K; i += REPEAT_T) {
        const RpCand cc = rp_cand(R[i], i, x, H, min_copies, min_span);
        if (rp_better(cc, c)) c = cc;
      }
      red[t] = c;
    }
    for (uint32_t d = REPEAT_T / 2; d > 0; d >>= 1)
      for (uint32_t t = 0; t < d; ++t)
        if (rp_better(red[t + d], red[t])) red[t] = red[t + d];
    const RpCand b = red[0];
    uint32_t ri;
    if (b.w == 0u) {
      if (H > x) { if (lit_len == 0u) lit_b = x; lit_len += H - x; }
      x = H;
      if (depth == 0u) break;
      --depth;
      ri = st_run[depth]; H = st_h[depth];
    } else if (b.st > x) {
      if (depth >= K) { fprintf(stderr, "a stack deeper than K\n"); exit(4); }
      st_run[depth] = b.idx; st_h[depth] = H;
      ++depth;
      H = b.st;
      continue;
    } else ri = b.idx;
    const RpRun run = R[ri];
    const uint32_t p = run.p, en = run.e < H ? run.e : H;
    uint32_t st = x;
    if (prev_p == p) {
      const uint32_t t_end = x + p < en - p + 1u ? x + p : en - p + 1u;
      for (uint32_t t = 0; t < REPEAT_T; ++t) {
        uint32_t found = 0xffffffffu;
        for (uint32_t u = x + t; u < t_end; u += REPEAT_T)
          if (rp_unit_equal(s, u, prev_b, p)) { found = u; break; }
        red_t[t] = found;
      }
      for (uint32_t d = REPEAT_T / 2; d > 0; d >>= 1)
        for (uint32_t t = 0; t < d; ++t)
          if (red_t[t + d] < red_t[t]) red_t[t] = red_t[t + d];
      const uint32_t found = red_t[0];
      if (found != 0xffffffffu && rp_enough((en - found) / p, p, min_copies, min_span)) st = found;
    }
    if (st > x) { if (lit_len == 0u) lit_b = x; lit_len += st - x; }
    if (lit_len) { emit(lit_b, 0u, 0u, lit_len); lit_len = 0u; }
    const uint32_t k = (en - st) / p;
    emit(st, p, k, k * p);
    ++out.n_repeats; out.covered += k * p;
    prev_p = p; prev_b = st;
    x = st + k * p;
  }
  if (lit_len) emit(lit_b, 0u, 0u, lit_len);
  out.segs.assign(SG.begin(), SG.begin() + nseg);
  return out;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    uint32_t max_period = 0, min_copies = 0, min_span = 0;
    std::string hex;
    in >> max_period >> min_copies >> min_span >> hex;
    if (hex == "-") hex.clear();
    const uint32_t L = (uint32_t)(hex.size() / 2);
    std::vector<uint8_t> arena((size_t)L + 64, 0);
    for (uint32_t i = 0; i < L; ++i) arena[i] = (uint8_t)strtoul(hex.substr(2 * (size_t)i, 2).c_str(), nullptr, 16);
    const Result R = parse(arena, L, max_period, min_copies, min_span);
    printf("%u %u %u %zu", R.flags, R.n_repeats, R.covered, R.segs.size());
    for (const Seg& g : R.segs) printf(" %u,%u,%u,%u", g.begin, g.period, g.copies, g.length);
    printf("\n");
  }
  return 0;
}

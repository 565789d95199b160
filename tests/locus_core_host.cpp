// locus_core_host.cpp — the arithmetic of the locus kernel's local pass (otter_amd/csrc/otg_locus_core.hpp) on the host, in the kernel's
// schedule: tasks ordered by (tier, class), the longest first, as otg_locus_resident plans them, 64 / S tasks to a wave of 64 lanes that
// run in lockstep, the units of a set side by side at lane boundaries, the rotate, the segmented prefix maximum, the maximum of the phase-0
// candidates over the task's lanes and the broadcasts done by indexing the lanes (row shifts inside 16 lanes where the kernel uses DPP, any
// lane where it uses ds_bpermute), finished tasks masked while their neighbours go on.  A stand-alone program (built with
// -fsanitize=address,undefined by tests/test_locus_host.py).  Input: "batch <n> <wide> <seg64> <match> <mismatch> <indel> <min_score>"
// followed by n lines "<hex allele | -> <hex unit>,<hex unit>,..."; output per task "score begin end flags tier class".  "narrow <match>
// <indel> <p>,<p>,..." prints lc_narrow_len, the bound of the narrow tier.  Every allele is allocated with the 15 bytes of slack the kernel
// may read, every unit with none, so an index beyond either is reported by the sanitizer.
#include "otg_locus_core.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace otg_locus_core;

struct Task { std::vector<uint8_t> s; std::vector<std::vector<uint8_t>> u; std::vector<uint32_t> p; uint32_t L = 0; };
struct Rec { uint32_t score = 0, begin = 0, end = 0, flags = 0, tier = 9, cls = 9; };

constexpr uint32_t NONE = 0xffffffffu;

template <typename T> static T from_lane(const T (&x)[64], uint32_t src) { return x[src & 63u]; }          // ds_bpermute: the address wraps
template <int D, typename T> static T row_up(const T (&x)[64], uint32_t lane) { return (lane & 15u) >= (uint32_t)D ? x[lane - D] : x[lane]; }

// one step of the prefix maximum; pos = the lane's place inside its unit
template <typename K, int S, int D> static void scan_step(K (&x)[64], const uint32_t (&pos)[64])
{
  if (D >= S) return;
  K nx[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const K from = S <= 16 ? row_up<D>(x, lane) : from_lane(x, lane - D);
    nx[lane] = ua_scan_take<K, true>(x[lane], from, pos[lane] >= (uint32_t)D);
  }
  for (uint32_t lane = 0; lane < 64; ++lane) x[lane] = nx[lane];
}

template <typename K, int R> static K pick(const K* v, uint32_t r)
{
  K x = v[0];
  for (int q = 1; q < R; ++q) x = r == (uint32_t)q ? v[q] : x;
  return x;
}

// one wave of lc_align<K, S, R>: tasks[g] (nullptr: no task) in segment g
template <typename K, int S, int R> static void wave(const Task* const* tasks, Rec* const* recs, const otg_tract_params& q)
{
  uint32_t L[64], p[64], ul[64], um[64][R], um_prev[64][R], last_lane[64], last_reg[64], below[64], bend[64][R];
  bool valid[64][R], live[64], is_last[64], is_first[64];
  K bias[64][R], V[64][R], best[64][R], last_bias[64];
  const uint8_t* s[64];
  const K km = tr_pen<K>(q.match), kx = tr_pen<K>(q.mismatch), kg = tr_pen<K>(q.indel);
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t jl = lane % S, seg_base = lane - jl;
    const Task* t = tasks[lane / S];
    live[lane] = t != nullptr;
    L[lane] = t ? t->L : 0u;
    s[lane] = t ? t->s.data() : nullptr;
    uint32_t k = NONE, ufirst = lane;
    const uint8_t* u = nullptr;
    ul[lane] = 0; p[lane] = 1;
    for (uint32_t c = 0, acc = 0; t && c < t->p.size(); ++c) {
      const uint32_t pc = t->p[c], nl = (pc + R - 1u) / R;
      if (jl >= acc && jl - acc < nl) { k = c; ul[lane] = jl - acc; p[lane] = pc; ufirst = seg_base + acc; u = t->u[c].data(); }
      acc += nl;
    }
    for (int r = 0; r < R; ++r) {
      const uint32_t j = ul[lane] * R + r;
      valid[lane][r] = k != NONE && j < p[lane];
      um[lane][r] = valid[lane][r] ? ua_unit_key(u[j]) : 0xffu;
      bias[lane][r] = valid[lane][r] ? tr_bias<K>(j, kg) : (K)0;
      V[lane][r] = (K)0; best[lane][r] = (K)0; bend[lane][r] = 0u;
    }
    last_lane[lane] = ufirst + (p[lane] - 1u) / R; last_reg[lane] = (p[lane] - 1u) % R;
    below[lane] = ul[lane] ? lane - 1u : last_lane[lane];
    is_last[lane] = lane == last_lane[lane]; is_first[lane] = ul[lane] == 0u && valid[lane][0];
    last_bias[lane] = tr_bias<K>(p[lane] - 1u, kg);
  }
  {
    uint32_t send[64];
    for (uint32_t lane = 0; lane < 64; ++lane) send[lane] = is_last[lane] ? pick<uint32_t, R>(um[lane], last_reg[lane]) : um[lane][R - 1];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      um_prev[lane][0] = from_lane(send, below[lane]);
      for (int r = 1; r < R; ++r) um_prev[lane][r] = um[lane][r - 1];
    }
  }
  uint32_t Lmax = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) Lmax = std::max(Lmax, L[lane]);
  for (uint32_t i0 = 0; i0 < Lmax; i0 += 16u) {                    // __any(i0 < L)
    uint8_t w[64][16];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      for (int k = 0; k < 16; ++k) w[lane][k] = 0;
      if (i0 < L[lane]) __builtin_memcpy(w[lane], s[lane] + i0, 16);
      for (int k = 0; k < 16; ++k) w[lane][k] = (uint8_t)otg_unitalign_core::ua_fold(w[lane][k]);
    }
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t row = i0 + k + 1u;
      K send[64], d0[64], T[64][R], h0[64], x[64], ex[64], lastv[64], lsend[64], best0[64], entry[64];
      for (uint32_t lane = 0; lane < 64; ++lane) send[lane] = (R > 1 && is_last[lane]) ? pick<K, R>(V[lane], last_reg[lane]) : V[lane][R - 1];
      for (uint32_t lane = 0; lane < 64; ++lane) d0[lane] = from_lane(send, below[lane]);
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t sc = w[lane][k];
        for (int r = 0; r < R; ++r) {
          const K cell = tr_cell<K>(r ? V[lane][r - 1] : d0[lane], V[lane][r], um_prev[lane][r] == sc, km, kx, kg, (K)row) + bias[lane][r];
          T[lane][r] = valid[lane][r] ? cell : (K)0;
        }
        h0[lane] = T[lane][0];
        for (int r = 1; r < R; ++r) T[lane][r] = ua_scan_take<K, true>(T[lane][r], T[lane][r - 1], true);
        x[lane] = T[lane][R - 1];
      }
      scan_step<K, S, 1>(x, ul); scan_step<K, S, 2>(x, ul); scan_step<K, S, 4>(x, ul); scan_step<K, S, 8>(x, ul); scan_step<K, S, 16>(x, ul);
      scan_step<K, S, 32>(x, ul);
      if (R > 1) {
        for (uint32_t lane = 0; lane < 64; ++lane) ex[lane] = from_lane(x, lane - 1u);
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (int r = 0; r < R - 1; ++r) T[lane][r] = ua_scan_take<K, true>(T[lane][r], ex[lane], ul[lane] > 0u);
      }
      for (uint32_t lane = 0; lane < 64; ++lane) { T[lane][R - 1] = x[lane]; lsend[lane] = pick<K, R>(T[lane], last_reg[lane]); }
      for (uint32_t lane = 0; lane < 64; ++lane) lastv[lane] = from_lane(lsend, last_lane[lane]) - last_bias[lane];
      for (uint32_t lane = 0; lane < 64; ++lane) best0[lane] = is_first[lane] ? lc_cand0<K>(h0[lane], lastv[lane], kg) : (K)0;
      for (uint32_t d = 1; d < (uint32_t)S; d <<= 1) {
        K o[64];
        for (uint32_t lane = 0; lane < 64; ++lane) o[lane] = from_lane(best0, lane ^ d);
        for (uint32_t lane = 0; lane < 64; ++lane) best0[lane] = tr_max<K>(best0[lane], o[lane]);
      }
      for (uint32_t lane = 0; lane < 64; ++lane) entry[lane] = lc_entry<K>(lastv[lane], best0[lane], kg);
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const bool act = row <= L[lane];
        for (int r = 0; r < R; ++r) {
          const K h = lc_close<K>(T[lane][r], bias[lane][r], entry[lane]);
          const bool on = act && valid[lane][r];
          V[lane][r] = on ? h : V[lane][r];
          const bool up = on && tr_improves<K>(h, best[lane][r]);
          best[lane][r] = up ? h : best[lane][r];
          bend[lane][r] = up ? row : bend[lane][r];
        }
      }
    }
  }
  K bk[64];
  uint32_t be[64], bj[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    bk[lane] = (K)0; be[lane] = 0xffffffffu; bj[lane] = 0xffffffffu;
    for (int r = 0; r < R; ++r)
      if (valid[lane][r] && tr_better<K>(best[lane][r], bend[lane][r], (lane % S) * R + r, bk[lane], be[lane], bj[lane])) {
        bk[lane] = best[lane][r]; be[lane] = bend[lane][r]; bj[lane] = (lane % S) * R + r;
      }
  }
  for (uint32_t d = 1; d < (uint32_t)S; d <<= 1) {
    K ok[64];
    uint32_t oe[64], oj[64];
    for (uint32_t lane = 0; lane < 64; ++lane) { ok[lane] = from_lane(bk, lane ^ d); oe[lane] = from_lane(be, lane ^ d); oj[lane] = from_lane(bj, lane ^ d); }
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (tr_better<K>(ok[lane], oe[lane], oj[lane], bk[lane], be[lane], bj[lane])) { bk[lane] = ok[lane]; be[lane] = oe[lane]; bj[lane] = oj[lane]; }
  }
  for (uint32_t lane = 0; lane < 64; lane += S)
    if (live[lane]) {
      Rec& r = *recs[lane / S];
      r.score = tr_score<K>(bk[lane]);
      const bool none = r.score == 0u || r.score < q.min_score;
      r.begin = none ? 0u : tr_begin<K>(bk[lane]); r.end = none ? 0u : be[lane]; r.flags = none ? OTG_LOCUS_NONE : 0u;
    }
}

template <typename K, int C> static void run_class(const std::vector<Task>& tasks, std::vector<Rec>& recs, const std::vector<uint32_t>& order, const otg_tract_params& q)
{
  constexpr int S = ua_class_lanes(C), R = ua_class_regs(C);
  constexpr uint32_t TPW = 64 / S;
  for (size_t w = 0; w * TPW < order.size(); ++w) {
    const Task* tk[TPW];
    Rec* rc[TPW];
    for (uint32_t g = 0; g < TPW; ++g) {
      const size_t slot = w * TPW + g;
      tk[g] = slot < order.size() ? &tasks[order[slot]] : nullptr;
      rc[g] = slot < order.size() ? &recs[order[slot]] : nullptr;
    }
    wave<K, S, R>(tk, rc, q);
  }
}

template <typename K> static void run_tier(uint32_t c, const std::vector<Task>& tasks, std::vector<Rec>& recs, const std::vector<uint32_t>& order, const otg_tract_params& q)
{
  switch (c) {
    case 0: run_class<K, 0>(tasks, recs, order, q); break;
    case 1: run_class<K, 1>(tasks, recs, order, q); break;
    case 2: run_class<K, 2>(tasks, recs, order, q); break;
    case 3: run_class<K, 3>(tasks, recs, order, q); break;
    case 4: run_class<K, 4>(tasks, recs, order, q); break;
    case 5: run_class<K, 5>(tasks, recs, order, q); break;
    default: run_class<K, 6>(tasks, recs, order, q); break;
  }
}

static std::vector<uint8_t> unhex(const std::string& h, size_t slack)
{
  const size_t n = h == "-" ? 0 : h.size() / 2;
  std::vector<uint8_t> v(n + slack, 0);
  for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
  return v;
}

static std::vector<std::string> split(const std::string& s)
{
  std::vector<std::string> out;
  std::istringstream in(s);
  std::string part;
  while (std::getline(in, part, ',')) out.push_back(part);
  return out;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string word;
    in >> word;
    if (word == "narrow") {
      otg_tract_params q{1u, 1u, 1u, 0u};
      std::string ps;
      in >> q.match >> q.indel >> ps;
      std::vector<uint32_t> p;
      for (const std::string& x : split(ps)) p.push_back((uint32_t)strtoul(x.c_str(), nullptr, 10));
      printf("%u\n", lc_narrow_len(q, p.data(), (uint32_t)p.size()));
      continue;
    }
    uint32_t n = 0, wide = 0, seg64 = 0;
    otg_tract_params q{0u, 0u, 0u, 0u};
    in >> n >> wide >> seg64 >> q.match >> q.mismatch >> q.indel >> q.min_score;
    if (word != "batch" || !tr_params_ok(q)) { fprintf(stderr, "expected a batch line with scores in range\n"); return 2; }
    std::vector<Task> tasks(n);
    std::vector<Rec> recs(n);
    std::vector<std::vector<uint32_t>> bins((size_t)2 * UP_CLASSES);
    for (uint32_t t = 0; t < n; ++t) {
      std::string hs, hu;
      if (!std::getline(std::cin, line)) { fprintf(stderr, "short batch\n"); return 2; }
      std::istringstream tin(line);
      tin >> hs >> hu;
      Task& k = tasks[t];
      k.s = unhex(hs, 15);
      k.L = (uint32_t)k.s.size() - 15u;
      for (const std::string& x : split(hu)) { k.u.push_back(unhex(x, 0)); k.p.push_back((uint32_t)k.u.back().size()); }
      const uint32_t cls = lc_class(k.p.data(), (uint32_t)k.p.size(), seg64 != 0);
      if (k.p.empty() || k.p.size() > OTG_UNITPARSE_MAX_UNITS || cls == UP_NO_CLASS) { fprintf(stderr, "task %u: a unit set the parse refuses\n", t); return 2; }
      if (k.L == 0u || k.L > OTG_LOCUS_MAX_LEN) { recs[t].flags = k.L ? OTG_LOCUS_TOO_LONG : OTG_LOCUS_NONE; continue; }
      const uint32_t tier = (wide || k.L > lc_narrow_len(q, k.p.data(), (uint32_t)k.p.size())) ? 1u : 0u;
      recs[t].tier = tier; recs[t].cls = cls;
      bins[tier * UP_CLASSES + cls].push_back(t);
    }
    for (uint32_t tc = 0; tc < 2u * UP_CLASSES; ++tc) {
      std::vector<uint32_t>& order = bins[tc];
      if (order.empty()) continue;
      std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return tasks[a].L != tasks[b].L ? tasks[a].L > tasks[b].L : a < b; });
      if (tc < (uint32_t)UP_CLASSES) run_tier<uint32_t>(tc, tasks, recs, order, q);
      else run_tier<uint64_t>(tc - UP_CLASSES, tasks, recs, order, q);
    }
    for (const Rec& r : recs) printf("%u %u %u %u %u %u\n", r.score, r.begin, r.end, r.flags, r.tier, r.cls);
  }
  return 0;
}

// unitalign_core_host.cpp — the arithmetic of the unit-alignment kernel (otter_amd/csrc/otg_unitalign_core.hpp) on the host, in the kernel's
// schedule: tasks binned by (tier, class, length bucket) as ua_classify bins them, 64 / S tasks to a wave of 64 lanes that run in
// lockstep, the rotate, the segmented prefix minimum and the broadcast done by indexing the lanes (row shifts inside 16 lanes where the
// kernel uses DPP, any lane where it uses ds_bpermute), finished tasks masked while their neighbours go on.  A stand-alone program (built
// with -fsanitize=address,undefined by tests/test_unitalign_host.py).  Input: "batch <n> <wide> <seg64>" followed by n lines
// "<hex allele | -> <hex unit | ->"; output per task "edits unit_bases end_phase flags tier class".  Every allele is allocated with the 15
// bytes of slack the kernel may read, every unit with none, so an index beyond either is reported by the sanitizer.
#include "otg_unitalign_core.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace otg_unitalign_core;

struct Task { std::vector<uint8_t> s, u; uint32_t L = 0, p = 0; };
struct Rec { uint32_t edits = 0, unit_bases = 0, end_phase = 0, flags = 0, tier = 9, cls = 9; };

template <typename T> static T from_lane(const T (&x)[64], uint32_t src) { return x[src & 63u]; }          // ds_bpermute: the address wraps
template <int D, typename T> static T row_up(const T (&x)[64], uint32_t lane) { return (lane & 15u) >= (uint32_t)D ? x[lane - D] : x[lane]; }

template <typename K, int S, int D> static void scan_step(K (&x)[64])
{
  if (D >= S) return;
  K nx[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const K from = S <= 16 ? row_up<D>(x, lane) : from_lane(x, lane - D);
    nx[lane] = ua_scan_take<K>(x[lane], from, lane % S >= (uint32_t)D);
  }
  for (uint32_t lane = 0; lane < 64; ++lane) x[lane] = nx[lane];
}

template <typename K, int R> static K pick(const K* v, uint32_t r)
{
  K x = v[0];
  for (int q = 1; q < R; ++q) x = r == (uint32_t)q ? v[q] : x;
  return x;
}

// one wave of ua_align<K, S, R>: tasks[g] (nullptr: no task) in segment g
template <typename K, int S, int R> static void wave(const Task* const* tasks, Rec* const* recs)
{
  uint32_t L[64], p[64], um[64][R], um_prev[64][R], last_lane[64], last_reg[64], below[64];
  bool valid[64][R], live[64], is_last[64];
  K bias[64][R], V[64][R];
  const uint8_t* s[64];
  const uint8_t* u[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t jl = lane % S, seg_base = lane - jl;
    const Task* t = tasks[lane / S];
    live[lane] = t != nullptr;
    L[lane] = t ? t->L : 0u; p[lane] = t ? t->p : 1u;
    s[lane] = t ? t->s.data() : nullptr; u[lane] = t ? t->u.data() : nullptr;
    for (int r = 0; r < R; ++r) {
      const uint32_t j = jl * R + r;
      valid[lane][r] = j < p[lane];
      um[lane][r] = (live[lane] && valid[lane][r]) ? ua_unit_key(u[lane][j]) : 0xffu;
      bias[lane][r] = valid[lane][r] ? ua_bias<K>(j, p[lane]) : (K)0;
      V[lane][r] = (K)0;
    }
    last_lane[lane] = seg_base + (p[lane] - 1u) / R; last_reg[lane] = (p[lane] - 1u) % R;
    below[lane] = jl ? lane - 1u : last_lane[lane];
    is_last[lane] = lane == last_lane[lane];
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
      for (int k = 0; k < 16; ++k) w[lane][k] = (uint8_t)ua_fold(w[lane][k]);
    }
    for (uint32_t k = 0; k < 16; ++k) {
      K send[64], d0[64], T[64][R], x[64], ex[64], lastv[64], lsend[64];
      for (uint32_t lane = 0; lane < 64; ++lane) send[lane] = (R > 1 && is_last[lane]) ? pick<K, R>(V[lane], last_reg[lane]) : V[lane][R - 1];
      for (uint32_t lane = 0; lane < 64; ++lane) d0[lane] = from_lane(send, below[lane]);
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t sc = w[lane][k];
        for (int r = 0; r < R; ++r) {
          const K cell = ua_cell<K>(r ? V[lane][r - 1] : d0[lane], V[lane][r], um_prev[lane][r] == sc) + bias[lane][r];
          T[lane][r] = valid[lane][r] ? cell : ua_inf<K>();
        }
        for (int r = 1; r < R; ++r) T[lane][r] = ua_scan_take<K>(T[lane][r], T[lane][r - 1], true);
        x[lane] = T[lane][R - 1];
      }
      scan_step<K, S, 1>(x); scan_step<K, S, 2>(x); scan_step<K, S, 4>(x); scan_step<K, S, 8>(x); scan_step<K, S, 16>(x); scan_step<K, S, 32>(x);
      if (R > 1) {
        for (uint32_t lane = 0; lane < 64; ++lane) ex[lane] = from_lane(x, lane - 1u);
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (int r = 0; r < R - 1; ++r) T[lane][r] = ua_scan_take<K>(T[lane][r], ex[lane], lane % S > 0u);
      }
      for (uint32_t lane = 0; lane < 64; ++lane) { T[lane][R - 1] = x[lane]; lsend[lane] = pick<K, R>(T[lane], last_reg[lane]); }
      for (uint32_t lane = 0; lane < 64; ++lane) lastv[lane] = from_lane(lsend, last_lane[lane]);
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const bool act = i0 + k < L[lane];
        for (int r = 0; r < R; ++r) {
          const K h = ua_close<K>(T[lane][r], lastv[lane], (lane % S) * R + r, p[lane]);
          V[lane][r] = (act && valid[lane][r]) ? h : V[lane][r];
        }
      }
    }
  }
  K best[64];
  uint32_t bj[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    best[lane] = ua_inf<K>(); bj[lane] = 0xffffffffu;
    for (int r = 0; r < R; ++r)
      if (valid[lane][r] && ua_better<K>(V[lane][r], (lane % S) * R + r, best[lane], bj[lane])) { best[lane] = V[lane][r]; bj[lane] = (lane % S) * R + r; }
  }
  for (uint32_t d = 1; d < (uint32_t)S; d <<= 1) {
    K ob[64];
    uint32_t oj[64];
    for (uint32_t lane = 0; lane < 64; ++lane) { ob[lane] = from_lane(best, lane ^ d); oj[lane] = from_lane(bj, lane ^ d); }
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (ua_better<K>(ob[lane], oj[lane], best[lane], bj[lane])) { best[lane] = ob[lane]; bj[lane] = oj[lane]; }
  }
  for (uint32_t lane = 0; lane < 64; lane += S)
    if (live[lane]) {
      Rec& r = *recs[lane / S];
      r.edits = ua_edits<K>(best[lane]); r.unit_bases = ua_unit_bases<K>(best[lane]); r.end_phase = bj[lane]; r.flags = 0u;
    }
}

template <typename K, int C> static void run_class(const std::vector<Task>& tasks, std::vector<Rec>& recs, const std::vector<uint32_t>& order)
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
    wave<K, S, R>(tk, rc);
  }
}

template <typename K> static void run_tier(uint32_t c, const std::vector<Task>& tasks, std::vector<Rec>& recs, const std::vector<uint32_t>& order)
{
  switch (c) {
    case 0: run_class<K, 0>(tasks, recs, order); break;
    case 1: run_class<K, 1>(tasks, recs, order); break;
    case 2: run_class<K, 2>(tasks, recs, order); break;
    case 3: run_class<K, 3>(tasks, recs, order); break;
    case 4: run_class<K, 4>(tasks, recs, order); break;
    case 5: run_class<K, 5>(tasks, recs, order); break;
    default: run_class<K, 6>(tasks, recs, order); break;
  }
}

static std::vector<uint8_t> unhex(const std::string& h, size_t slack)
{
  const size_t n = h == "-" ? 0 : h.size() / 2;
  std::vector<uint8_t> v(n + slack, 0);
  for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
  return v;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string word;
    uint32_t n = 0, wide = 0, seg64 = 0;
    in >> word >> n >> wide >> seg64;
    if (word != "batch") { fprintf(stderr, "expected a batch line\n"); return 2; }
    std::vector<Task> tasks(n);
    std::vector<Rec> recs(n);
    // the bins of ua_classify; inside a bin the kernel's order is that of its atomics, here the task order
    std::vector<std::vector<uint32_t>> bins((size_t)2 * UA_CLASSES * UA_BUCKETS);
    for (uint32_t t = 0; t < n; ++t) {
      std::string hs, hu;
      if (!std::getline(std::cin, line)) { fprintf(stderr, "short batch\n"); return 2; }
      std::istringstream tin(line);
      tin >> hs >> hu;
      Task& k = tasks[t];
      k.s = unhex(hs, 15); k.u = unhex(hu, 0);
      k.L = (uint32_t)k.s.size() - 15u; k.p = (uint32_t)k.u.size();
      const uint32_t refusal = ua_refusal(k.L, k.p);
      if (refusal || k.L == 0u) { recs[t].flags = refusal; continue; }
      const uint32_t tier = (wide || k.L > OTG_UNITALIGN_NARROW_LEN) ? 1u : 0u, cls = ua_class(k.p, seg64 != 0);
      recs[t].tier = tier; recs[t].cls = cls;
      bins[(tier * UA_CLASSES + cls) * UA_BUCKETS + (UA_BUCKETS - 1u - ua_bucket(k.L))].push_back(t);
    }
    for (uint32_t tc = 0; tc < 2u * UA_CLASSES; ++tc) {
      std::vector<uint32_t> order;
      for (uint32_t b = 0; b < UA_BUCKETS; ++b) order.insert(order.end(), bins[tc * UA_BUCKETS + b].begin(), bins[tc * UA_BUCKETS + b].end());
      if (order.empty()) continue;
      if (tc < (uint32_t)UA_CLASSES) run_tier<uint32_t>(tc, tasks, recs, order);
      else run_tier<uint64_t>(tc - UA_CLASSES, tasks, recs, order);
    }
    for (const Rec& r : recs) printf("%u %u %u %u %u %u\n", r.edits, r.unit_bases, r.end_phase, r.flags, r.tier, r.cls);
  }
  return 0;
}

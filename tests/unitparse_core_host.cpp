// unitparse_core_host.cpp — the arithmetic of the joint unit parse (otter_amd/csrc/otg_unitparse_core.hpp) on the host, in the kernel's
// schedule: tasks ordered by class and length as the plan of unitparse.hip orders them, 64 / S tasks to a wave of 64 lanes that run in
// lockstep, every unit at a lane boundary, the rotate, the prefix minimum segmented by unit, the minimum of the phase-0 candidates over the
// task's lanes (row shifts inside 16 lanes where the kernel uses DPP, any lane where it uses ds_bpermute), the ballot words of every row, and
// then the backward walk over those words.  A stand-alone program (built with -fsanitize=address,undefined by tests/test_unitparse_host.py).
// Input: "batch <n>" followed by n lines "<hex allele | -> <K> <hex unit> ..."; output per task "edits switches unit_bases n_segments
// end_unit end_phase flags class" followed by six numbers per segment.  Every allele is allocated with the 15 bytes of slack the kernel may
// read, every unit arena and every wave's store with none, so an index beyond any of them is reported by the sanitizer.
#include "otg_unitparse_core.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace otg_unitparse_core;

struct Task {
  std::vector<uint8_t> s, units;
  std::vector<uint64_t> unit_off;
  std::vector<uint32_t> unit_len;
  uint32_t L = 0, K = 0;
};
struct Rec {
  uint32_t edits = 0, switches = 0, unit_bases = 0, n_segments = 0, end_unit = 0, end_phase = 0, flags = 0, cls = 9;
  std::vector<otg_unitparse_seg> segs;
};

constexpr uint32_t NONE = 0xffffffffu;

template <typename T> static T from_lane(const T (&x)[64], uint32_t src) { return x[src & 63u]; }          // ds_bpermute: the address wraps
template <int D> static uint64_t row_up(const uint64_t (&x)[64], uint32_t lane) { return (lane & 15u) >= (uint32_t)D ? x[lane - D] : x[lane]; }

template <int S, int D> static void scan_step(uint64_t (&x)[64], const uint32_t (&ul)[64])
{
  if (D >= S) return;
  uint64_t nx[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint64_t from = S <= 16 ? row_up<D>(x, lane) : from_lane(x, lane - D);
    nx[lane] = ua_scan_take<uint64_t>(x[lane], from, ul[lane] >= (uint32_t)D);
  }
  for (uint32_t lane = 0; lane < 64; ++lane) x[lane] = nx[lane];
}

template <typename K, int R> static K pick(const K* v, uint32_t r)
{
  K x = v[0];
  for (int q = 1; q < R; ++q) x = r == (uint32_t)q ? v[q] : x;
  return x;
}

static uint64_t ballot(const bool (&b)[64])
{
  uint64_t w = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) w |= (uint64_t)b[lane] << lane;
  return w;
}

// one wave of up_forward<S, R, true> and the walks of its tasks: tasks[g] (nullptr: no task) in segment g
template <int S, int R> static int wave(const Task* const* tasks, Rec* const* recs)
{
  constexpr uint32_t WORDS = up_words(R);
  uint32_t L[64], p[64], k[64], ul[64], ufirst[64], um[64][R], um_prev[64][R], last_lane[64], last_reg[64], below[64];
  bool valid[64][R], live[64], is_last[64], is_first[64];
  uint64_t bias[64][R], onward[64][R], V[64][R];
  const uint8_t* s[64];
  uint32_t rows_w = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t jl = lane % S, seg_base = lane - jl;
    const Task* t = tasks[lane / S];
    live[lane] = t != nullptr;
    L[lane] = t ? t->L : 0u;
    s[lane] = t ? t->s.data() : nullptr;
    rows_w = std::max(rows_w, L[lane]);
    k[lane] = NONE; ul[lane] = 0; p[lane] = 1; ufirst[lane] = lane;
    const uint8_t* u = nullptr;
    for (uint32_t q = 0, acc = 0; t && q < t->K; ++q) {
      const uint32_t pq = t->unit_len[q], nl = (pq + R - 1u) / R;
      if (jl >= acc && jl - acc < nl) { k[lane] = q; ul[lane] = jl - acc; p[lane] = pq; ufirst[lane] = seg_base + acc; u = t->units.data() + t->unit_off[q]; }
      acc += nl;
    }
    for (int r = 0; r < R; ++r) {
      const uint32_t j = ul[lane] * R + r;
      valid[lane][r] = k[lane] != NONE && j < p[lane];
      um[lane][r] = valid[lane][r] ? ua_unit_key(u[j]) : 0xffu;
      bias[lane][r] = valid[lane][r] ? up_bias(j, p[lane]) : 0u;
      onward[lane][r] = up_onward(j);
      V[lane][r] = 0u;
    }
    last_lane[lane] = ufirst[lane] + (p[lane] - 1u) / R; last_reg[lane] = (p[lane] - 1u) % R;
    below[lane] = ul[lane] ? lane - 1u : last_lane[lane];
    is_last[lane] = lane == last_lane[lane];
    is_first[lane] = ul[lane] == 0u && valid[lane][0];
  }
  {
    uint32_t send[64];
    for (uint32_t lane = 0; lane < 64; ++lane) send[lane] = is_last[lane] ? pick<uint32_t, R>(um[lane], last_reg[lane]) : um[lane][R - 1];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      um_prev[lane][0] = from_lane(send, below[lane]);
      for (int r = 1; r < R; ++r) um_prev[lane][r] = um[lane][r - 1];
    }
  }
  std::vector<uint64_t> trace((size_t)rows_w * WORDS);              // exactly what the plan gives the wave
  for (uint32_t i0 = 0; i0 < rows_w; i0 += 16u) {                    // __any(i0 < L)
    uint8_t w[64][16];
    for (uint32_t lane = 0; lane < 64; ++lane) {
      for (int q = 0; q < 16; ++q) w[lane][q] = 0;
      if (i0 < L[lane]) __builtin_memcpy(w[lane], s[lane] + i0, 16);
      for (int q = 0; q < 16; ++q) w[lane][q] = (uint8_t)ua_fold(w[lane][q]);
    }
    for (uint32_t kk = 0; kk < 16; ++kk) {
      uint64_t send[64], d0[64], d[64][R], v[64][R], T[64][R], cell0[64], x[64], ex[64], lsend[64], last[64], cand[64], best0[64], nb[64];
      uint32_t code[64][R];
      for (uint32_t lane = 0; lane < 64; ++lane) send[lane] = (R > 1 && is_last[lane]) ? pick<uint64_t, R>(V[lane], last_reg[lane]) : V[lane][R - 1];
      for (uint32_t lane = 0; lane < 64; ++lane) d0[lane] = from_lane(send, below[lane]);
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t sc = w[lane][kk];
        for (int r = 0; r < R; ++r) {
          d[lane][r] = up_diag(r ? V[lane][r - 1] : d0[lane], um_prev[lane][r] == sc);
          v[lane][r] = up_vert(V[lane][r]);
          T[lane][r] = valid[lane][r] ? up_min(d[lane][r], v[lane][r]) + bias[lane][r] : up_inf();
        }
        cell0[lane] = up_min(d[lane][0], v[lane][0]);
        for (int r = 1; r < R; ++r) T[lane][r] = ua_scan_take<uint64_t>(T[lane][r], T[lane][r - 1], true);
        x[lane] = T[lane][R - 1];
      }
      scan_step<S, 1>(x, ul); scan_step<S, 2>(x, ul); scan_step<S, 4>(x, ul); scan_step<S, 8>(x, ul); scan_step<S, 16>(x, ul); scan_step<S, 32>(x, ul);
      if (R > 1) {
        for (uint32_t lane = 0; lane < 64; ++lane) ex[lane] = from_lane(x, lane - 1u);
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (int r = 0; r < R - 1; ++r) T[lane][r] = ua_scan_take<uint64_t>(T[lane][r], ex[lane], ul[lane] > 0u);
      }
      for (uint32_t lane = 0; lane < 64; ++lane) { T[lane][R - 1] = x[lane]; lsend[lane] = pick<uint64_t, R>(T[lane], last_reg[lane]); }
      for (uint32_t lane = 0; lane < 64; ++lane) last[lane] = from_lane(lsend, last_lane[lane]);
      for (uint32_t lane = 0; lane < 64; ++lane) best0[lane] = cand[lane] = is_first[lane] ? up_phase0(cell0[lane], last[lane]) : up_inf();
      for (uint32_t dd = 1; dd < (uint32_t)S; dd <<= 1) {
        for (uint32_t lane = 0; lane < 64; ++lane) nb[lane] = up_min(best0[lane], from_lane(best0, lane ^ dd));
        for (uint32_t lane = 0; lane < 64; ++lane) best0[lane] = nb[lane];
      }
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const bool act = i0 + kk < L[lane];
        const uint64_t entry = up_entry(last[lane], best0[lane]);
        for (int r = 0; r < R; ++r) {
          const uint64_t h = up_close(T[lane][r], bias[lane][r], entry, onward[lane][r]);
          code[lane][r] = up_code(h, d[lane][r], v[lane][r], ul[lane] * R + r, last[lane]);
          V[lane][r] = (act && valid[lane][r]) ? h : V[lane][r];
        }
      }
      uint64_t words[WORDS];
      bool bit[64];
      for (uint32_t lane = 0; lane < 64; ++lane) bit[lane] = is_first[lane] && cand[lane] == best0[lane];
      words[2 * R] = ballot(bit);
      for (int r = 0; r < R; ++r)
        for (int b = 0; b < 2; ++b) {
          for (uint32_t lane = 0; lane < 64; ++lane) bit[lane] = ((code[lane][r] >> b) & 1u) != 0u;
          words[2 * r + b] = ballot(bit);
        }
      const uint32_t row = i0 + kk;
      if (row < rows_w)
        for (uint32_t q = 0; q < WORDS; ++q) trace[(size_t)row * WORDS + q] = words[q];
    }
  }
  uint64_t best[64];
  uint32_t bg[64];
  for (uint32_t lane = 0; lane < 64; ++lane) {
    best[lane] = up_inf(); bg[lane] = NONE;
    for (int r = 0; r < R; ++r)
      if (valid[lane][r] && (V[lane][r] < best[lane] || (V[lane][r] == best[lane] && lane * R + r < bg[lane]))) { best[lane] = V[lane][r]; bg[lane] = lane * R + r; }
  }
  for (uint32_t dd = 1; dd < (uint32_t)S; dd <<= 1) {
    uint64_t ob[64];
    uint32_t og[64];
    for (uint32_t lane = 0; lane < 64; ++lane) { ob[lane] = from_lane(best, lane ^ dd); og[lane] = from_lane(bg, lane ^ dd); }
    for (uint32_t lane = 0; lane < 64; ++lane)
      if (ob[lane] < best[lane] || (ob[lane] == best[lane] && og[lane] < bg[lane])) { best[lane] = ob[lane]; bg[lane] = og[lane]; }
  }
  for (uint32_t lane = 0; lane < 64; ++lane)
    if (live[lane] && bg[lane] != NONE && bg[lane] / R == lane) {
      Rec& r = *recs[lane / S];
      r.edits = up_edits(best[lane]); r.switches = up_switches(best[lane]); r.unit_bases = up_unit_bases(best[lane]);
      r.n_segments = r.switches + 1u; r.end_unit = k[lane]; r.end_phase = ul[lane] * R + bg[lane] % R; r.flags = 0u;
    }
  // the backward pass: one task after the other, over the wave's words
  for (uint32_t g = 0; g < 64u / S; ++g) {
    const Task* t = tasks[g];
    if (!t) continue;
    Rec& r = *recs[g];
    r.segs.assign(r.n_segments, otg_unitparse_seg{9u, 9u, 9u, 9u, 9u, 9u});
    const uint32_t bad = up_walk(trace.data(), R, g * S, S, t->s.data(), t->L, t->units.data(), t->unit_off.data(), t->unit_len.data(), t->K, r.end_unit, r.end_phase,
                                 r.segs.data(), r.n_segments);
    if (bad) { fprintf(stderr, "the walk contradicts the forward pass (code %u)\n", bad); return 3; }
  }
  return 0;
}

template <int C> static int run_class(const std::vector<Task>& tasks, std::vector<Rec>& recs, const std::vector<uint32_t>& order)
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
    if (int rc2 = wave<S, R>(tk, rc)) return rc2;
  }
  return 0;
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
    uint32_t n = 0;
    in >> word >> n;
    if (word != "batch") { fprintf(stderr, "expected a batch line\n"); return 2; }
    std::vector<Task> tasks(n);
    std::vector<Rec> recs(n);
    std::vector<uint32_t> by_class[UP_CLASSES];
    for (uint32_t t = 0; t < n; ++t) {
      if (!std::getline(std::cin, line)) { fprintf(stderr, "short batch\n"); return 2; }
      std::istringstream tin(line);
      std::string hs;
      Task& k = tasks[t];
      tin >> hs >> k.K;
      k.s = unhex(hs, 15); k.L = (uint32_t)k.s.size() - 15u;
      for (uint32_t q = 0; q < k.K; ++q) {
        std::string hu;
        tin >> hu;
        const std::vector<uint8_t> u = unhex(hu, 0);
        k.unit_off.push_back(k.units.size()); k.unit_len.push_back((uint32_t)u.size());
        k.units.insert(k.units.end(), u.begin(), u.end());
      }
      const uint32_t cls = k.K ? up_class(k.unit_len.data(), k.K) : UP_NO_CLASS;
      if (cls == UP_NO_CLASS || k.K > OTG_UNITPARSE_MAX_UNITS) { fprintf(stderr, "a unit set the parse refuses\n"); return 2; }
      if (k.L > OTG_UNITPARSE_MAX_LEN) { recs[t].flags = OTG_UNITPARSE_TOO_LONG; continue; }
      if (k.L == 0u) continue;
      recs[t].cls = cls;
      by_class[cls].push_back(t);
    }
    for (uint32_t c = 0; c < (uint32_t)UP_CLASSES; ++c) {
      std::vector<uint32_t>& v = by_class[c];
      if (v.empty()) continue;
      std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return tasks[a].L != tasks[b].L ? tasks[a].L > tasks[b].L : a < b; });
      int rc = 0;
      switch (c) {
        case 0: rc = run_class<0>(tasks, recs, v); break;
        case 1: rc = run_class<1>(tasks, recs, v); break;
        case 2: rc = run_class<2>(tasks, recs, v); break;
        case 3: rc = run_class<3>(tasks, recs, v); break;
        case 4: rc = run_class<4>(tasks, recs, v); break;
        case 5: rc = run_class<5>(tasks, recs, v); break;
        default: rc = run_class<6>(tasks, recs, v); break;
      }
      if (rc) return rc;
    }
    for (const Rec& r : recs) {
      printf("%u %u %u %u %u %u %u %u", r.edits, r.switches, r.unit_bases, r.n_segments, r.end_unit, r.end_phase, r.flags, r.cls);
      for (const otg_unitparse_seg& g : r.segs) printf(" %u %u %u %u %u %u", g.unit, g.begin, g.end, g.unit_bases, g.edits, g.start_phase);
      printf("\n");
    }
  }
  return 0;
}

// unitset_core_host.cpp — the shared functions of the unit-set discovery (otter_amd/csrc/otg_unitset_core.hpp) run on the host in the
// kernels' schedule: the smallest rotation by 64 lanes with strided starts and a butterfly, the hash, the class table filled by a sequential
// compare-and-swap in a shuffled order, the largest weight, sixteen rounds of selection by T strided "threads" and a tree, the pair list, the
// selection.  Stand-alone (its own main), built with -fsanitize=address,undefined by tests/test_unitset_host.py.
//
// stdin, per group:
//   group <n_alleles> <min_bases> <min_permille> <redundant_permille> <hash_bits> <slots> <threads> <shuffle_seed>
//   <allele as hex, or -> <n_segments> then per repeat segment: <begin> <period> <length>        (n_alleles lines)
// stdout, per group:
//   set <n_units> <n_classes> <n_ranked> <flags> <weight_total> <hash matches that the compare told apart>
//   <unit as hex> <weight> <segments> <length>                                                    (n_units lines)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>
#include "otg_unitset_core.hpp"

using namespace otg_unitset_core;

static std::vector<uint8_t> unhex(const std::string& h)
{
  std::vector<uint8_t> o;
  if (h == "-") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return o;
}

// step 3 of the unit alignment as include/otter_gpu.h writes it -> edits
static uint32_t unit_edits(const uint8_t* s, uint32_t L, const uint8_t* u, uint32_t p)
{
  const uint64_t E = 1ull << 32, W = E + 1;
  std::vector<uint64_t> V(p, 0), T(p);
  for (uint32_t i = 0; i < L; ++i) {
    const uint32_t cs = mo_code(s[i]);
    for (uint32_t j = 0; j < p; ++j) T[j] = V[j] + E;
    for (uint32_t j = 0; j < p; ++j) {
      const uint64_t d = V[j] + ((cs == mo_code(u[j]) && cs < 4u) ? 0 : E) + 1;
      T[(j + 1) % p] = std::min(T[(j + 1) % p], d);
    }
    for (uint32_t k = 0; k < 2 * p; ++k) T[(k + 1) % p] = std::min(T[(k + 1) % p], T[k % p] + W);
    V = T;
  }
  return (uint32_t)(*std::min_element(V.begin(), V.end()) >> 32);
}

struct HostCas {
  uint32_t operator()(uint32_t* p, uint32_t expected, uint32_t desired) const
  {
    const uint32_t old = *p;
    if (old == expected) *p = desired;
    return old;
  }
};

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream head(line);
    std::string word;
    uint32_t n_alleles, hash_bits, ns, T, seed;
    otg_unitset_params q;
    head >> word >> n_alleles >> q.min_bases >> q.min_permille >> q.redundant_permille >> hash_bits >> ns >> T >> seed;
    q.reserved = 0;
    if (word != "group" || !us_params_ok(q) || ns == 0 || T == 0 || (T & (T - 1))) { fprintf(stderr, "bad header: %s\n", line.c_str()); return 2; }
    std::vector<uint8_t> arena;
    std::vector<uint64_t> off;
    std::vector<UsCand> cands;
    for (uint32_t a = 0; a < n_alleles; ++a) {
      std::getline(std::cin, line);
      std::istringstream row(line);
      std::string hex;
      uint32_t n_segs;
      row >> hex >> n_segs;
      const std::vector<uint8_t> s = unhex(hex);
      off.push_back(arena.size());
      arena.insert(arena.end(), s.begin(), s.end());
      for (uint32_t k = 0; k < n_segs; ++k) {
        UsCand c{};
        row >> c.begin >> c.p >> c.length;
        if (c.p == 0 || c.p > OTG_UNITALIGN_MAX_UNIT || c.begin + c.p > s.size()) { fprintf(stderr, "bad segment\n"); return 2; }
        c.allele = a; c.pos = off[a] + c.begin;
        cands.push_back(c);
      }
    }
    // ---- us_candidates: the codes, 64 lanes, the butterfly, the hash
    for (UsCand& c : cands) {
      std::vector<uint8_t> code(c.p);
      for (uint32_t j = 0; j < c.p; ++j) code[j] = (uint8_t)mo_code(arena[c.pos + j]);
      uint32_t best[64], next[64];
      for (uint32_t lane = 0; lane < 64; ++lane) best[lane] = us_rot_lane(code.data(), c.p, lane);
      for (uint32_t d = 1; d < 64; d <<= 1) {
        for (uint32_t lane = 0; lane < 64; ++lane) next[lane] = us_rot_pick(code.data(), c.p, best[lane], best[lane ^ d]);
        std::copy(next, next + 64, best);
      }
      for (uint32_t lane = 1; lane < 64; ++lane)
        if (best[lane] != best[0]) { fprintf(stderr, "the lanes disagree on a rotation\n"); return 3; }
      c.rot = best[0];
      c.hash = us_hash(code.data(), c.p, c.rot, hash_bits);
    }
    // ---- us_vote: the table in a shuffled order
    std::vector<uint32_t> order(cands.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::mt19937 rng(seed);
    if (seed) std::shuffle(order.begin(), order.end(), rng);
    std::vector<uint32_t> slot(ns, 0), segs(ns, 0);
    std::vector<uint64_t> weight(ns, 0), rep(ns, 0);
    std::vector<bool> taken(ns, false);
    uint64_t total = 0;
    uint32_t n_classes = 0, told_apart = 0;
    bool over = false;
    for (uint32_t i : order) {
      const UsCand& c = cands[i];
      total += c.length;
      {                                                              // how often does the compare decide?  (the probe sequence of us_table_insert)
        uint32_t h = us_slot(c.hash, c.p, ns);
        for (uint32_t probe = 0; probe < ns && slot[h]; ++probe) {
          const UsCand& o = cands[slot[h] - 1];
          if (o.p == c.p && o.hash == c.hash) {
            if (us_same_rotation(arena.data(), o.pos, o.rot, c.pos, c.rot, c.p)) break;
            ++told_apart;
          }
          if (++h == ns) h = 0;
        }
      }
      const uint32_t r = us_table_insert(slot.data(), ns, cands.data(), i, arena.data(), HostCas{});
      if (r == US_NONE) { over = true; continue; }
      const uint32_t h = r & ~US_FRESH;
      if (r & US_FRESH) ++n_classes;
      weight[h] += c.length; segs[h] += 1;
      rep[h] = std::max(rep[h], us_rep_key(c.length, c.allele, c.begin));
    }
    const bool overflow = over || n_classes > OTG_UNITSET_MAX_CLASSES;
    uint64_t top = 0;
    for (uint32_t h = 0; h < ns; ++h)
      if (slot[h]) top = std::max(top, weight[h]);
    auto before = [&](uint32_t x, uint32_t y) {
      const UsCand &a = cands[slot[x] - 1], &b = cands[slot[y] - 1];
      return us_before(arena.data(), weight[x], a.p, a.pos, a.rot, weight[y], b.p, b.pos, b.rot);
    };
    std::vector<uint32_t> ranked;
    for (uint32_t round = 0; round < OTG_UNITSET_TOP && !overflow; ++round) {
      std::vector<uint32_t> red(T, US_NONE);
      for (uint32_t tid = 0; tid < T; ++tid)
        for (uint32_t h = tid; h < ns; h += T) {
          if (!slot[h] || taken[h] || !us_eligible(weight[h], top, q)) continue;
          if (red[tid] == US_NONE || before(h, red[tid])) red[tid] = h;
        }
      for (uint32_t d = T / 2; d > 0; d >>= 1)
        for (uint32_t tid = 0; tid < d; ++tid) {
          const uint32_t u = red[tid], v = red[tid + d];
          red[tid] = u == US_NONE ? v : (v != US_NONE && before(v, u)) ? v : u;
        }
      if (red[0] == US_NONE) break;
      taken[red[0]] = true;
      ranked.push_back(red[0]);
    }
    // ---- us_tasks, the unit alignment, us_select_groups
    const uint32_t nr = (uint32_t)ranked.size();
    std::vector<uint32_t> p(OTG_UNITSET_TOP, 0), sel(OTG_UNITPARSE_MAX_UNITS, 0);
    std::vector<uint64_t> pos(OTG_UNITSET_TOP, 0);
    for (uint32_t c = 0; c < nr; ++c) {
      p[c] = cands[slot[ranked[c]] - 1].p;
      pos[c] = off[us_rep_allele(rep[ranked[c]])] + us_rep_begin(rep[ranked[c]]);
    }
    std::vector<uint32_t> edits(us_pairs(nr) + 1, 0);
    uint32_t redundant = 0;
    for (uint32_t c = 1; c < nr; ++c)
      for (uint32_t d = 0; d < c; ++d) {
        if (pos[c] + 2ull * p[c] > arena.size()) { fprintf(stderr, "a representative's two copies leave the arena\n"); return 3; }
        edits[us_pair_index(c, d)] = unit_edits(arena.data() + pos[c], 2 * p[c], arena.data() + pos[d], p[d]);
        if (us_explained(edits[us_pair_index(c, d)], p[c], q)) redundant |= 1u << c;
      }
    const uint32_t n_units = us_select(p.data(), nr, redundant, sel.data());
    const uint32_t flags = (overflow ? OTG_UNITSET_OVERFLOW : 0u) | (n_units ? 0u : OTG_UNITSET_NONE);
    printf("set %u %u %u %u %llu %u\n", n_units, overflow ? OTG_UNITSET_MAX_CLASSES + 1 : n_classes, nr, flags, (unsigned long long)total, told_apart);
    for (uint32_t k = 0; k < n_units; ++k) {
      const uint32_t c = sel[k], h = ranked[c];
      for (uint32_t j = 0; j < p[c]; ++j) printf("%02x", "ACGTN"[mo_code(arena[pos[c] + j])]);
      printf(" %llu %u %u\n", (unsigned long long)weight[h], segs[h], p[c]);
    }
  }
  return 0;
}

// CPU restatement used by the tests (built with g++ into a temporary directory):
//   edit_align_ref align [diamond]   stdin: "<pattern> <text>" per line ("-" = empty); stdout: "<score> <op string or ->"
//       WFA2-lib's unit-cost end-to-end alignment with the edit piggy-back tie-break (wavefront_compute_edit_idm_piggyback: candidates
//       ins, del, misms; three sequential tests in that order, the last equal one wins; a cell whose max overshoots an end is nulled)
//       over FULL wavefronts, then the op string unpacked forward (a maximal match run, then per operation the operation and a
//       maximal match run).  `diamond` recomputes the same alignment restricted to |k - kend| <= s - t (the device kernel's region).
//   edit_align_ref compare           stdin: regions as "R <region> <n_truth> <n_spannings> <n_query>", then "T <seq>" x n_truth,
//       "S <value>" x n_spannings, "Q <seq>" x n_query; stdout: what compare() prints per region (src/compare.cpp:106-146),
//       stderr: its warning lines without the timestamp.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {

constexpr int NUL = -(1 << 30);

struct Result { int score; std::string ops; };

int extend(const std::string& P, const std::string& T, int k, int h)
{
  int v = h - k;
  while (v < (int)P.size() && h < (int)T.size() && P[v] == T[h]) { ++v; ++h; }
  return h;
}

// diamond < 0: full wavefronts; otherwise the score s the diamond is built from
Result align(const std::string& P, const std::string& T, int diamond)
{
  const int pl = (int)P.size(), tl = (int)T.size(), kend = tl - pl;
  std::vector<std::vector<int>> off;      // off[t][k - lo[t]]
  std::vector<std::vector<char>> op;
  std::vector<int> lo, hi;
  auto range = [&](int t, int* a, int* b) {
    *a = std::max(-t, -pl); *b = std::min(t, tl);
    if (diamond >= 0) { *a = std::max(*a, kend - (diamond - t)); *b = std::min(*b, kend + (diamond - t)); }
  };
  auto get = [&](int t, int k) { return (k < lo[t] || k > hi[t]) ? NUL : off[t][k - lo[t]]; };
  int t = 0;
  for (;; ++t) {
    int a, b;
    range(t, &a, &b);
    lo.push_back(a); hi.push_back(b);
    off.emplace_back(b >= a ? b - a + 1 : 0, NUL);
    op.emplace_back(b >= a ? b - a + 1 : 0, 0);
    for (int k = a; k <= b; ++k) {
      int mx;
      char o = 0;
      if (t == 0) mx = 0;
      else {
        const int ins = get(t - 1, k - 1) + 1, del = get(t - 1, k + 1), misms = get(t - 1, k) + 1;
        mx = std::max(del, std::max(misms, ins));
        if (mx == ins) o = 'I';
        if (mx == del) o = 'D';
        if (mx == misms) o = 'X';
      }
      const int h = mx, v = mx - k;
      if (mx < 0 || v < 0 || h > tl || v > pl) mx = NUL;
      else mx = extend(P, T, k, h);
      off[t][k - a] = mx;
      op[t][k - a] = o;
    }
    if (get(t, kend) >= tl) break;
    if (t > pl + tl + 2) { std::cerr << "no end\n"; exit(2); }
  }
  const int s = t;
  std::string ops(s, '?');
  int k = kend;
  for (int u = s; u >= 1; --u) {
    const char o = op[u][k - lo[u]];
    ops[u - 1] = o;
    if (o == 'I') k -= 1; else if (o == 'D') k += 1;
  }
  std::string out;
  int v = 0, h = 0;
  for (int q = 0; q <= s; ++q) {
    if (q > 0) {
      const char o = ops[q - 1];
      out += o;
      if (o == 'I') ++h; else if (o == 'D') ++v; else { ++v; ++h; }
    }
    while (v < pl && h < tl && P[v] == T[h]) { out += 'M'; ++v; ++h; }
  }
  return {s, out};
}

struct DistCompare { int i, j; double edit, ops; };

void compare_region(const std::string& region, const std::vector<std::string>& truth, const std::vector<int>& spannings,
                    std::vector<std::string> query)
{
  if (query.size() == 1) query.push_back(query.front());
  if (truth.size() > 2) { std::cerr << "WARNING: skipping region due to multiple expected alignments (>2) for region: " << region << '\n'; return; }
  if (truth.size() == 1) { std::cerr << "WARNING: skipping region due to single expected alignment for region: " << region << '\n'; return; }
  if (truth.empty()) { std::cerr << "WARNING: skipping region due no expected alignments for region: " << region << '\n'; return; }
  if (query.empty()) { std::cerr << "WARNING: skipping region due no query alleles for region: " << region << '\n'; return; }
  std::vector<DistCompare> d;
  for (int i = 0; i < (int)truth.size(); ++i) {
    const std::string& subj = truth[i];
    for (int j = 0; j < (int)query.size(); ++j) {
      const std::string& q = query[j];
      if (subj == q || (subj == "N" && q == "NDNNN") || (q == "N" && subj == "NDNNN")) d.push_back({i, j, 0, (double)q.size()});
      else if (subj == "N" || q == "N" || subj == "NDNNN" || q == "NDNNN") d.push_back({i, j, (double)(q.size() - 1), (double)q.size()});
      else {
        const Result r = subj.size() > q.size() ? align(subj, q, -1) : align(q, subj, -1);
        d.push_back({i, j, (double)r.score, (double)r.ops.size()});
      }
    }
  }
  std::sort(d.begin(), d.end(), [](const DistCompare& x, const DistCompare& y) {
    if (x.edit == y.edit) return x.ops < y.ops;
    else return x.edit < y.edit;
  });
  size_t e1 = 1;
  for (; e1 < d.size(); ++e1) if (d[e1].i != d[0].i && d[e1].j != d[0].j) break;
  for (size_t idx : {(size_t)0, e1}) {
    const DistCompare& m = d[idx];
    const int sp = m.i < (int)spannings.size() ? spannings[m.i] : -1;       // (the reference reads outside its vector here)
    std::cout << region << '\t' << truth[m.i].size() << '\t' << query[m.j].size() << '\t' << sp << '\t' << m.edit << '\t' << m.ops << '\n';
  }
}

} // namespace

int main(int argc, char** argv)
{
  const std::string mode = argc > 1 ? argv[1] : "align";
  if (mode == "align") {
    const bool diamond = argc > 2 && std::string(argv[2]) == "diamond";
    std::string p, t;
    while (std::cin >> p >> t) {
      if (p == "-") p.clear();
      if (t == "-") t.clear();
      Result r = align(p, t, -1);
      if (diamond) {
        const Result d = align(p, t, r.score);
        if (d.score != r.score) { std::cerr << "diamond score differs\n"; return 3; }
        r = d;
      }
      std::cout << r.score << ' ' << (r.ops.empty() ? "-" : r.ops) << '\n';
    }
    return 0;
  }
  if (mode == "compare") {
    std::string tag;
    while (std::cin >> tag) {
      if (tag != "R") { std::cerr << "bad input\n"; return 2; }
      std::string region; int nt, ns, nq;
      std::cin >> region >> nt >> ns >> nq;
      std::vector<std::string> truth(nt), query(nq);
      std::vector<int> sp(ns);
      for (auto& x : truth) std::cin >> tag >> x;
      for (auto& x : sp) std::cin >> tag >> x;
      for (auto& x : query) std::cin >> tag >> x;
      compare_region(region, truth, sp, query);
    }
    return 0;
  }
  std::cerr << "unknown mode\n";
  return 2;
}

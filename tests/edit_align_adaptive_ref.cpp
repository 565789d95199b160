// CPU restatement of the unit-cost end-to-end alignment WITH its op string under WFA2-lib's adaptive wavefront reduction,
// wf_heuristic_wfadaptive(min_wavefront_length, max_distance_threshold, steps_between_cutoffs), used by the tests (built with g++ into a
// temporary directory).  Written from the rule, not from the device code:
//   edit_align_adaptive_ref align <min_wavefront_length> <max_distance_threshold> <steps_between_cutoffs>
//       stdin: "<pattern> <text>" per line ("-" = empty); stdout: "<score> <cells> <op string or ->"
// The whole history is kept: for every score the wavefront it computed (offsets and one operation per diagonal) and the sub-range the
// cut left of it.  A cell of score t looks for its three sources (insertion from k-1, deletion from k+1, mismatch from k) in what the cut
// left of score t-1 only; the operation is chosen as WFA2-lib's edit piggy-back chooses it (tests in the order insertion, deletion,
// mismatch, the last equal one wins: tests/edit_align_ref.cpp), the cell is dropped when it overshoots either sequence, else extended
// along its matches.  After the end test has failed, the cut: every `steps` scores, when the wavefront holds at least
// `min_wavefront_length` diagonals, each diagonal's distance is what it still has to align, max(plen - v, tlen - h); from the low end
// diagonals further than `max_distance_threshold` from the best distance are dropped, never past the diagonal below the end diagonal,
// then likewise from the high end, never past the diagonal above it (nor below the new low end).  cells = the widths of all wavefronts as
// computed, i.e. before their cut.  The walk back and the unpacking are those of tests/edit_align_ref.cpp.  The cut is recalled from
// upstream's wavefront_heuristic.c and cannot be verified offline; the scores and cells it leads to are checked against the oracle.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

namespace {

constexpr int NONE = -(1 << 30);
constexpr int FAR = 1 << 30;

struct Front {
  int lo = 0, hi = -1;           // diagonals computed at this score
  int keep_lo = 0, keep_hi = -1; // what the cut left
  std::vector<int> off;          // offset (text position) per diagonal, NONE = dropped cell
  std::vector<char> op;
  int at(int k) const { return (k < keep_lo || k > keep_hi) ? NONE : off[k - lo]; }
};

struct Params { int min_len, max_dist, steps; };

struct Result { int score; unsigned long long cells; std::string ops; };

Result align(const std::string& P, const std::string& T, const Params& par)
{
  const int pl = (int)P.size(), tl = (int)T.size(), kend = tl - pl;
  std::vector<Front> hist;
  unsigned long long cells = 0;
  int wait = 0;
  for (int t = 0;; ++t) {
    Front f;
    if (t == 0) { f.lo = 0; f.hi = 0; }
    else {
      const Front& prev = hist.back();
      f.lo = std::max(prev.keep_lo - 1, -pl);
      f.hi = std::min(prev.keep_hi + 1, tl);
    }
    const int w = f.hi - f.lo + 1;
    f.off.assign(w, NONE);
    f.op.assign(w, 0);
    cells += (unsigned long long)w;
    for (int k = f.lo; k <= f.hi; ++k) {
      int best;
      char o = 0;
      if (t == 0) best = 0;
      else {
        const Front& prev = hist.back();
        const int ins = prev.at(k - 1) + 1, del = prev.at(k + 1), mis = prev.at(k) + 1;
        best = std::max(ins, std::max(del, mis));
        if (best == ins) o = 'I';
        if (best == del) o = 'D';
        if (best == mis) o = 'X';
      }
      int h = best, v = best - k;
      if (best < 0 || v < 0 || h > tl || v > pl) h = NONE;
      else while (v < pl && h < tl && P[v] == T[h]) { ++v; ++h; }
      f.off[k - f.lo] = h;
      f.op[k - f.lo] = o;
    }
    f.keep_lo = f.lo; f.keep_hi = f.hi;
    const bool ended = kend >= f.lo && kend <= f.hi && f.off[kend - f.lo] >= tl;
    if (!ended) {
      // the cut
      --wait;
      if (wait <= 0 && w >= par.min_len) {
        auto dist = [&](int k) {
          const int h = f.off[k - f.lo];
          if (h < 0) return FAR;
          return std::max(pl - (h - k), tl - h);
        };
        int best = FAR;
        for (int k = f.lo; k <= f.hi; ++k) best = std::min(best, dist(k));
        const int low_stop = std::min(kend - 1, f.hi);
        int nlo = f.lo;
        while (nlo < low_stop && dist(nlo) - best > par.max_dist) ++nlo;
        const int high_stop = std::max(kend + 1, nlo);
        int nhi = f.hi;
        while (nhi > high_stop && dist(nhi) - best > par.max_dist) --nhi;
        f.keep_lo = nlo; f.keep_hi = nhi;
        wait = par.steps;
      }
    }
    hist.push_back(std::move(f));
    if (ended) break;
    if (t > pl + tl + 2) { std::cerr << "no end\n"; exit(2); }
  }
  const int s = (int)hist.size() - 1;
  std::string ops(s, '?');
  int k = kend;
  for (int u = s; u >= 1; --u) {
    const Front& f = hist[u];
    if (k < f.lo || k > f.hi) { std::cerr << "walk left the wavefront\n"; exit(3); }
    const char o = f.op[k - f.lo];
    ops[u - 1] = o;
    if (o == 'I') k -= 1; else if (o == 'D') k += 1;
  }
  if (k != 0) { std::cerr << "walk did not reach diagonal 0\n"; exit(3); }
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
  return {s, cells, out};
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 5 || std::string(argv[1]) != "align") { std::cerr << "usage: edit_align_adaptive_ref align <a> <b> <c>\n"; return 2; }
  Params par{atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
  if (par.steps < 1) par.steps = 1;
  std::string p, t;
  while (std::cin >> p >> t) {
    if (p == "-") p.clear();
    if (t == "-") t.clear();
    const Result r = align(p, t, par);
    std::cout << r.score << ' ' << r.cells << ' ' << (r.ops.empty() ? "-" : r.ops) << '\n';
  }
  return 0;
}

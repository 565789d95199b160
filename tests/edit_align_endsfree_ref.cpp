// CPU restatement of the unit-cost alignment WITH its op string when end gaps are free (WFAlignerEdit(Alignment)::alignEndsFree), used by
// the tests (built with g++ into a temporary directory).  Written from the rule, not from the device code:
//   edit_align_endsfree_ref full | hexagon | adaptive <min_wavefront_length> <max_distance_threshold> <steps_between_cutoffs>
//       stdin: "<pattern> <text> <pattern_begin_free> <pattern_end_free> <text_begin_free> <text_end_free>" per line ("-" = empty)
//       stdout: "<score> <cells> <op string or ->"
// The rule.  Diagonal k = h - v (h text position, v pattern position), a wavefront stores h.  Score 0 holds the diagonals
// [max(-pattern_begin_free, -plen), min(text_begin_free, tlen)], diagonal k starting at h = max(k, 0): the cells of the first row and
// the first column that cost nothing.  A cell of score t takes the largest of insertion (diagonal k-1, +1), deletion (k+1) and mismatch
// (k, +1) of score t-1 and records which, tested in the order insertion, deletion, mismatch, the last equal one winning (WFA2-lib's edit
// piggy-back, tests/edit_align_ref.cpp); it is dropped when it overshoots either sequence, else extended along its matches.  The
// diagonals of a score are looked at in ascending order and the alignment ends at the first whose cell has reached the end of the text
// with at most pattern_end_free of the pattern left, or the end of the pattern with at most text_end_free of the text left.  The walk
// back starts there and ends on a diagonal of score 0.  The op string names every column: the free gap in front (I for a start on a
// positive diagonal, D on a negative one), a maximal match run, per operation the operation and a maximal match run, then I up to the
// end of the text and D up to the end of the pattern.  score = the operations walked (free gaps cost nothing).
//   full      every wavefront whole: score t spans the score-0 range grown by t either side, clamped to [-plen, tlen].
//             cells = the widths of all wavefronts.
//   hexagon   the same alignment computed again inside the region the device pass keeps: with S the score-0 range and
//             E = [kend - text_end_free, kend + pattern_end_free] (kend = tlen - plen; every ending cell lies on a diagonal of E), both
//             clamped, score t keeps [S.lo - t, S.hi + t] n [E.lo - (s - t), E.hi + (s - t)], s being the score `full` found.  The
//             program fails (exit 3) unless score and op string are those of `full`; cells as `full`.
//   adaptive  under wf_heuristic_wfadaptive: after the end test has failed, every `steps` scores, when the wavefront holds at least
//             `min_wavefront_length` diagonals, each diagonal's distance is what it still has to align when end gaps are free,
//             min(max(tlen - h, plen - v - pattern_end_free), max(plen - v, tlen - h - text_end_free)); from the low end diagonals
//             further than `max_distance_threshold` from the best distance are dropped, never past the diagonal below E, then likewise
//             from the high end, never past the diagonal above E (nor below the new low end).  The next score spans what was left, grown
//             by one, and finds its sources in what was left only.  cells = the widths of all wavefronts as computed.  The cut is
//             recalled from upstream's wavefront_heuristic.c (tests/edit_align_adaptive_ref.cpp); the scores and cells it leads to are
//             checked against the oracle.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

namespace {

constexpr int NONE = -(1 << 30);
constexpr int FAR = 1 << 30;

struct Free { int pb, pe, tb, te; };
struct Cut { bool on; int min_len, max_dist, steps; };

struct Front {
  int lo = 0, hi = -1;           // diagonals computed at this score
  int keep_lo = 0, keep_hi = -1; // what the cut left
  std::vector<int> off;
  std::vector<char> op;
  int at(int k) const { return (k < keep_lo || k > keep_hi) ? NONE : off[k - lo]; }
};

struct Result { int score; unsigned long long cells; std::string ops; };

// hexagon_s < 0: the wavefronts grow by one either side of what the previous score kept; otherwise the region built from that score
Result align(const std::string& P, const std::string& T, const Free& fr, const Cut& cut, int hexagon_s)
{
  const int pl = (int)P.size(), tl = (int)T.size(), kend = tl - pl;
  const int s_lo = std::max(-fr.pb, -pl), s_hi = std::min(fr.tb, tl);
  const int e_lo = std::max(kend - std::min(fr.te, tl), -pl), e_hi = std::min(kend + std::min(fr.pe, pl), tl);
  std::vector<Front> hist;
  unsigned long long cells = 0;
  int wait = 0, k_end = 0;
  for (int t = 0;; ++t) {
    Front f;
    if (hexagon_s >= 0) {
      f.lo = std::max(std::max(s_lo - t, e_lo - (hexagon_s - t)), -pl);
      f.hi = std::min(std::min(s_hi + t, e_hi + (hexagon_s - t)), tl);
    } else if (t == 0) { f.lo = s_lo; f.hi = s_hi; }
    else {
      f.lo = std::max(hist.back().keep_lo - 1, -pl);
      f.hi = std::min(hist.back().keep_hi + 1, tl);
    }
    const int w = std::max(f.hi - f.lo + 1, 0);
    f.off.assign(w, NONE);
    f.op.assign(w, 0);
    cells += (unsigned long long)w;
    bool ended = false;
    for (int k = f.lo; k <= f.hi; ++k) {
      int best;
      char o = 0;
      if (t == 0) best = std::max(k, 0);
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
      if (!ended && h >= 0 && ((h >= tl && pl - v <= fr.pe) || (v >= pl && tl - h <= fr.te))) { ended = true; k_end = k; }
    }
    f.keep_lo = f.lo; f.keep_hi = f.hi;
    if (!ended && cut.on) {
      --wait;
      if (wait <= 0 && w >= cut.min_len) {
        auto dist = [&](int k) {
          const int h = f.off[k - f.lo];
          if (h < 0) return FAR;
          const int left_v = pl - (h - k), left_h = tl - h;
          return std::min(std::max(left_h, left_v - fr.pe), std::max(left_v, left_h - fr.te));
        };
        int best = FAR;
        for (int k = f.lo; k <= f.hi; ++k) best = std::min(best, dist(k));
        const int low_stop = std::min(kend - fr.te - 1, f.hi);
        int nlo = f.lo;
        while (nlo < low_stop && dist(nlo) - best > cut.max_dist) ++nlo;
        const int high_stop = std::max(kend + fr.pe + 1, nlo);
        int nhi = f.hi;
        while (nhi > high_stop && dist(nhi) - best > cut.max_dist) --nhi;
        f.keep_lo = nlo; f.keep_hi = nhi;
        wait = cut.steps;
      }
    }
    hist.push_back(std::move(f));
    if (ended) break;
    if (t > pl + tl + 2 || (hexagon_s >= 0 && t >= hexagon_s)) { std::cerr << "no end\n"; exit(2); }
  }
  const int s = (int)hist.size() - 1;
  std::string ops(s, '?');
  int k = k_end;
  for (int u = s; u >= 1; --u) {
    const Front& f = hist[u];
    if (k < f.lo || k > f.hi) { std::cerr << "walk left the wavefront\n"; exit(3); }
    const char o = f.op[k - f.lo];
    ops[u - 1] = o;
    if (o == 'I') k -= 1; else if (o == 'D') k += 1; else if (o != 'X') { std::cerr << "walk met a cell without an operation\n"; exit(3); }
  }
  if (k < s_lo || k > s_hi) { std::cerr << "walk did not reach a diagonal of score 0\n"; exit(3); }
  int h = std::max(k, 0), v = std::max(-k, 0);
  std::string out(h, 'I');
  out.append(v, 'D');
  for (int q = 0; q <= s; ++q) {
    if (q > 0) {
      const char o = ops[q - 1];
      out += o;
      if (o == 'I') ++h; else if (o == 'D') ++v; else { ++v; ++h; }
    }
    while (v < pl && h < tl && P[v] == T[h]) { out += 'M'; ++v; ++h; }
  }
  if (h != hist[s].off[k_end - hist[s].lo] || h - v != k_end) { std::cerr << "the op string does not end on the ending cell\n"; exit(3); }
  out.append(tl - h, 'I');
  out.append(pl - v, 'D');
  return {s, cells, out};
}

} // namespace

int main(int argc, char** argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  Cut cut{false, 0, 0, 1};
  if (mode == "adaptive" && argc == 5) { cut = {true, atoi(argv[2]), atoi(argv[3]), std::max(atoi(argv[4]), 1)}; }
  else if (!((mode == "full" || mode == "hexagon") && argc == 2)) { std::cerr << "usage: edit_align_endsfree_ref full | hexagon | adaptive <a> <b> <c>\n"; return 2; }
  std::string p, t;
  Free fr;
  while (std::cin >> p >> t >> fr.pb >> fr.pe >> fr.tb >> fr.te) {
    if (p == "-") p.clear();
    if (t == "-") t.clear();
    Result r = align(p, t, fr, cut, -1);
    if (mode == "hexagon") {
      const Result x = align(p, t, fr, cut, r.score);
      if (x.score != r.score || x.ops != r.ops) { std::cerr << "the hexagon gives another alignment\n"; return 3; }
    }
    std::cout << r.score << ' ' << r.cells << ' ' << (r.ops.empty() ? "-" : r.ops) << '\n';
  }
  return 0;
}

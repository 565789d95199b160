// Host check of the closed-form score ranges of the gap-affine register tiers (otter_amd/csrc/affine_score_range.hpp; built by
// tests/test_affine_score_range_host.py with -fsanitize=address,undefined).  `Recurrence` is the bookkeeping the kernel carried from score
// to score before the closed form replaced it (commit 80c7124, wfa_affine_reg.hip: the ten history variables r1..r4 and id, their update
// order, the clamps and the diamond clip).  Both are run score by score up to and including the score at which the recurrence gives up,
// over pl, tl in 1..12, start ranges lo0 in -4..0 and hi0 in 0..4, end ranges from end-free lengths 0..4 on both sides and U in 0..40;
// every score must agree in kind (range, empty, fail) and, for a range, in both ends.  Score 1 must be the only empty score.
#include "affine_score_range.hpp"
#include <cstdio>

using namespace otg_affine;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

struct Recurrence {
  int lo0, hi0, pl, tl, U, elo, ehi;
  int r1lo = 1, r1hi = 0, r2lo = 1, r2hi = 0, r3lo = 1, r3hi = 0, r4lo = 1, r4hi = 0, idlo = 1, idhi = 0;
  // one score, as the kernel's preamble and its two exits had it
  int step(int s, int* lo_out, int* hi_out)
  {
    const bool first = s == 0;
    int lo, hi;
    if (first) { lo = lo0; hi = hi0; }
    else {
      lo = 1 << 30; hi = -(1 << 30);
      if (r2hi >= r2lo) { lo = imin(lo, r2lo); hi = imax(hi, r2hi); }
      if (r4hi >= r4lo) { lo = imin(lo, r4lo - 1); hi = imax(hi, r4hi + 1); }
      if (idhi >= idlo) { lo = imin(lo, idlo - 1); hi = imax(hi, idhi + 1); }
      if (lo < -pl) lo = -pl;
      if (hi > tl) hi = tl;
      if (hi >= lo) {
        const int room = U - s;
        lo = imax(lo, elo - room); hi = imin(hi, ehi + room);
        if (room < 0 || hi < lo) return RANGE_FAIL;
      }
    }
    r4lo = r3lo; r4hi = r3hi; r3lo = r2lo; r3hi = r2hi; r2lo = r1lo; r2hi = r1hi;
    if (hi < lo) {
      r1lo = 1; r1hi = 0; idlo = 1; idhi = 0;
      return RANGE_EMPTY;
    }
    r1lo = lo; r1hi = hi;
    idlo = first ? 1 : lo; idhi = first ? 0 : hi;
    *lo_out = lo; *hi_out = hi;
    return RANGE_OK;
  }
};

int main()
{
  long long sets = 0, scores = 0, empties = 0, ends = 0;
  for (int pl = 1; pl <= 12; ++pl)
    for (int tl = 1; tl <= 12; ++tl)
      for (int lo0 = -4; lo0 <= 0; ++lo0)
        for (int hi0 = 0; hi0 <= 4; ++hi0)
          for (int tef = 0; tef <= 4; ++tef)
            for (int pef = 0; pef <= 4; ++pef)
              for (int U = 0; U <= 40; ++U) {
                const int kend = tl - pl, elo = kend - tef, ehi = kend + pef;
                ++sets;
                Recurrence r{lo0, hi0, pl, tl, U, elo, ehi};
                for (int s = 0;; ++s) {
                  int rl = 0, rh = 0, cl = 0, ch = 0;
                  const int rk = r.step(s, &rl, &rh);
                  const int ck = affine_score_range(s, lo0, hi0, pl, tl, U, elo, ehi, &cl, &ch);
                  ++scores;
                  CHECK(rk == ck, "kind: pl %d tl %d lo0 %d hi0 %d elo %d ehi %d U %d score %d: recurrence %d closed form %d", pl, tl, lo0, hi0, elo, ehi, U, s, rk, ck);
                  if (rk == RANGE_OK && ck == RANGE_OK)
                    CHECK(rl == cl && rh == ch, "range: pl %d tl %d lo0 %d hi0 %d elo %d ehi %d U %d score %d: recurrence [%d, %d] closed form [%d, %d]", pl, tl, lo0, hi0, elo, ehi, U, s, rl, rh, cl, ch);
                  if (rk == RANGE_EMPTY || ck == RANGE_EMPTY) {
                    ++empties;
                    CHECK(s == 1, "empty score %d: pl %d tl %d lo0 %d hi0 %d elo %d ehi %d U %d", s, pl, tl, lo0, hi0, elo, ehi, U);
                  }
                  if (rk == RANGE_FAIL || ck == RANGE_FAIL) { ++ends; break; }
                  if (s > U + 2) { CHECK(false, "no end: pl %d tl %d U %d", pl, tl, U); break; }
                }
              }
  std::printf("sets %lld scores %lld empty %lld ended %lld fails %d\n", sets, scores, empties, ends, fails);
  return fails ? 1 : 0;
}

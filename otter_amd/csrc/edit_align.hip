// edit_align.hip — batched unit-cost wavefront aligner WITH op strings (gfx950).
//
// Replaces wfa::WFAlignerEdit(Alignment, MemoryMed)::alignEnd2End + getAlignmentScore() + getAlignmentCigar()
// (reference: src/compare.cpp:59-61,95), and ::alignEndsFree (src/analignments.cpp:88-96) with the free end gaps explicit
// (otg_edit_align_span_batch; the kernels' EF instantiations).
//
// Three steps per batch:
//   1. the exact score s of every pair from the existing score chain (otg_launch_edit: wavefront + bit-parallel tiers);
//   2. a provenance pass restricted to the diamond |k - kend| <= s - t of score t: ONE wave64 per alignment, lanes =
//      diagonals, the wavefront of furthest-reaching offsets updated in place (LDS tier, or a global-row tier for wide
//      ones), 2 bits of provenance per (score, diagonal) cell written to an HBM arena sized exactly from the known scores
//      (two 64-bit ballots per 64-diagonal chunk);
//   3. lane 0 of the same wave walks the provenance back from (s, kend), storing the s edit operations in forward order;
//      the whole wave then unpacks them the way WFA2-lib's pcigar_unpack_linear does: a maximal match run, then per
//      operation the operation and a maximal match run (wavefront_pcigar.c:151).
// Provenance rule = wavefront_compute_edit_idm_piggyback (wavefront_compute_edit.c:143-190): candidates ins (k-1, +1),
// del (k+1), misms (k, +1); max; three sequential tests ins, del, misms, the last equal one wins; then the cell is nulled
// when h > tlen or v > plen.
//
// Under wfadaptive(min_wavefront_length, max_distance_threshold, steps_between_cutoffs) (otg_edit_align_heur_batch) the same three steps run
// WITHOUT the diamond: the cut reads the offset of every live diagonal of a score, so the pass has to carry the whole wavefront the score
// chain carried — edit_align_adaptive_kernel, further down.
#include "otg_wfadaptive.hpp"
#include "otg_chain.hpp"
#include <algorithm>
#include <cstdlib>

namespace {

using lds_i32 = __attribute__((address_space(3))) int32_t;

constexpr uint8_t OP_INS = 1, OP_DEL = 2, OP_MISMS = 3;

// diagonal range of score t inside the diamond (end-to-end: the score-t wavefront spans [-t, t] clamped to the matrix)
__host__ __device__ __forceinline__ void diamond_range(int t, int s, int kend, int pl, int tl, int* lo, int* hi)
{
  int a = -t, b = t;
  if (a < kend - (s - t)) a = kend - (s - t);
  if (b > kend + (s - t)) b = kend + (s - t);
  if (a < -pl) a = -pl;
  if (b > tl) b = tl;
  *lo = a; *hi = b;
}

// Free ends: S = the diagonals of score 0, E = the diagonals an alignment may end on (every ending cell lies on one of them),
// both clamped to the matrix [-pl, tl].  An end-to-end task has S = {0}, E = {kend}.
struct SpanGeom { int slo, shi, elo, ehi; };

__host__ __device__ __forceinline__ SpanGeom span_geom(const otg_align_task& t, int pl, int tl)
{
  const int kend = tl - pl;
  if (!t.endsfree) return SpanGeom{0, 0, kend, kend};
  SpanGeom g;
  g.slo = t.pattern_begin_free < pl ? -t.pattern_begin_free : -pl;
  g.shi = t.text_begin_free < tl ? t.text_begin_free : tl;
  g.elo = kend - (t.text_end_free < tl ? t.text_end_free : tl);            // >= -pl
  g.ehi = kend + (t.pattern_end_free < pl ? t.pattern_end_free : pl);      // <= tl
  return g;
}

// diagonal range of score t with free ends: what S can have reached after t scores and what can still reach E within the s - t left
// (with S = {0}, E = {kend} this is diamond_range)
__host__ __device__ __forceinline__ void span_range(int t, int s, const SpanGeom& g, int pl, int tl, int* lo, int* hi)
{
  int a = g.slo - t, b = g.shi + t;
  if (a < g.elo - (s - t)) a = g.elo - (s - t);
  if (b > g.ehi + (s - t)) b = g.ehi + (s - t);
  if (a < -pl) a = -pl;
  if (b > tl) b = tl;
  *lo = a; *hi = b;
}

// the union of the ranges of the scores 0 .. s: the wavefront window is sized and based on it
__host__ __device__ __forceinline__ void span_union(int s, const SpanGeom& g, int pl, int tl, int* kmin, int* kmax)
{
  int a = g.slo, b = g.shi;
  for (int t = 0; t <= s; ++t) {
    int lo, hi;
    span_range(t, s, g, pl, tl, &lo, &hi);
    if (hi < lo) continue;
    if (lo < a) a = lo;
    if (hi > b) b = hi;
  }
  *kmin = a; *kmax = b;
}

__host__ __device__ __forceinline__ uint64_t prov_row_bytes(int lo, int hi)
{
  return hi >= lo ? (uint64_t)((hi - lo + 64) / 64) * 16u : 0u;
}

struct AlignJob {
  uint64_t prov_off;      // into the provenance arena (bytes, 16-aligned)
  uint64_t ops_off;       // into the op buffer (s bytes)
  uint64_t cig_off;       // into the device cigar arena (ignored when no cigar is produced)
};

// Backtrace (ONE lane calls it): walks the provenance rows back from (s, kend), storing the s edit operations in forward order in opv.
// range(sc, &lo, &hi) = the diagonals row sc covers (its size follows from them); r_end = the bytes of all s rows.  Returns the number of
// insertions, 0xFFFFFFFF when the walk leaves a row, meets a cell without provenance or does not end on a diagonal of score 0,
// [k0_lo, k0_hi] (end-to-end: diagonal 0); *k_begin = the diagonal it ended on.
template <class Range>
__device__ __forceinline__ uint32_t edit_backtrace(const uint8_t* prow0, uint64_t r_end, int s, int kend, uint8_t* opv, Range range,
                                                   int k0_lo, int k0_hi, int* k_begin)
{
  uint32_t n_ins = 0;
  int k = kend;
  for (int sc = s; sc >= 1; --sc) {
    int lo, hi;
    range(sc, &lo, &hi);
    const uint64_t rb = prov_row_bytes(lo, hi);
    r_end -= rb;
    if (k < lo || k > hi) { n_ins = 0xFFFFFFFFu; break; }
    const int idx = k - lo;
    const uint64_t* src = (const uint64_t*)(prow0 + r_end + (uint64_t)(idx >> 6) * 16u);
    const uint32_t bit = (uint32_t)(idx & 63);
    const uint32_t op = (uint32_t)((src[0] >> bit) & 1u) | ((uint32_t)((src[1] >> bit) & 1u) << 1);
    opv[sc - 1] = (uint8_t)op;
    if (op == OP_INS) { ++n_ins; k -= 1; }
    else if (op == OP_DEL) k += 1;
    else if (op != OP_MISMS) { n_ins = 0xFFFFFFFFu; break; }
  }
  if ((k < k0_lo || k > k0_hi) && n_ins != 0xFFFFFFFFu) n_ins = 0xFFFFFFFFu;
  *k_begin = k;
  return n_ins;
}

// Unpack (whole wave) from cell (v, h), writing at out + pos: a maximal match run, then per operation the operation and a maximal match run.
__device__ __forceinline__ void edit_unpack_run(const uint8_t* P, const uint8_t* T, int pl, int tl, int s, const uint8_t* opv, uint8_t* out, int lane,
                                                int& v, int& h, uint32_t& pos)
{
  for (int q = 0; q <= s; ++q) {
    if (q > 0) {
      const uint32_t op = opv[q - 1];
      const uint8_t ch = op == OP_INS ? 'I' : op == OP_DEL ? 'D' : 'X';
      if (lane == 0) out[pos] = ch;
      ++pos;
      if (op == OP_INS) ++h; else if (op == OP_DEL) ++v; else { ++v; ++h; }
    }
    const int rem = pl - v < tl - h ? pl - v : tl - h;
    const int m = rem > 0 ? otg_wave_match(P, T, v, h, rem, lane) : 0;
    for (int i = lane; i < m; i += 64) out[pos + (uint32_t)i] = 'M';
    pos += (uint32_t)m; v += m; h += m;
  }
}

// End to end: from (0, 0).  False when the string does not end at (pl, tl).
__device__ __forceinline__ bool edit_unpack(const uint8_t* P, const uint8_t* T, int pl, int tl, int s, const uint8_t* opv, uint8_t* out, int lane)
{
  int v = 0, h = 0;
  uint32_t pos = 0;
  edit_unpack_run(P, T, pl, tl, s, opv, out, lane, v, h, pos);
  return v == pl && h == tl;
}

// Free ends: the walk began on diagonal k_begin of score 0 and the pass ended on cell (k_end, h_end).  The free gap in front (k_begin x I or
// -k_begin x D), the operations, then I up to tl and D up to pl.  False when the operations do not lead to the ending cell.
__device__ __forceinline__ bool edit_unpack_span(const uint8_t* P, const uint8_t* T, int pl, int tl, int s, const uint8_t* opv, uint8_t* out, int lane,
                                                 int k_begin, int k_end, int h_end)
{
  int h = k_begin > 0 ? k_begin : 0, v = k_begin < 0 ? -k_begin : 0;
  for (int i = lane; i < h; i += 64) out[i] = 'I';
  for (int i = lane; i < v; i += 64) out[i] = 'D';
  uint32_t pos = (uint32_t)(h + v);
  edit_unpack_run(P, T, pl, tl, s, opv, out, lane, v, h, pos);
  if (h != h_end || h - v != k_end) return false;
  for (int i = lane; i < tl - h; i += 64) out[pos + (uint32_t)i] = 'I';
  pos += (uint32_t)(tl - h);
  for (int i = lane; i < pl - v; i += 64) out[pos + (uint32_t)i] = 'D';
  return true;
}

// stat[ti] = s on success; -2: the end cell was not reached or the backtrace left the diamond; -3: the unpacked string does not end at (plen, tlen)
// EF: tasks with free ends — the region is span_range, the score-0 row covers S, the pass ends on the first diagonal of row s, in
// ascending order, whose cell satisfies the ends-free end test, the walk back ends on a diagonal of S and the free gaps are written out.
template <int CAP, int WPB, bool GLOBAL_WF, bool EF>
__global__ __launch_bounds__(WPB * 64) void edit_align_kernel(
    const uint8_t* __restrict__ arena, const otg_align_task* __restrict__ tasks, const int32_t* __restrict__ scores,
    const uint32_t* __restrict__ todo, uint32_t n_todo, const AlignJob* __restrict__ jobs,
    uint8_t* __restrict__ prov, uint8_t* __restrict__ ops, uint8_t* __restrict__ cig, uint32_t* __restrict__ cig_len,
    int32_t* __restrict__ stat, uint32_t* __restrict__ ticket, int32_t* gws, int gcap)
{
  extern __shared__ __attribute__((aligned(16))) int32_t smem[];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  volatile int32_t* gwf = GLOBAL_WF ? (volatile int32_t*)(gws + (size_t)(blockIdx.x * WPB + wib) * (size_t)gcap) : nullptr;
  volatile lds_i32* lwf = (volatile lds_i32*)smem + wib * CAP;
  auto wf_rd = [&](int j) -> int { if constexpr (GLOBAL_WF) return gwf[j]; else return lwf[j]; };
  auto wf_wr = [&](int j, int v) { if constexpr (GLOBAL_WF) gwf[j] = v; else lwf[j] = v; };

  for (;;) {
    const uint32_t tk = otg_wave_atomic_add(ticket, 1u);
    if (tk >= n_todo) break;
    const uint32_t ti = todo[tk];
    const otg_align_task t = tasks[ti];
    const AlignJob jb = jobs[ti];
    const uint8_t* P = arena + t.pattern_off;
    const uint8_t* T = arena + t.text_off;
    const int pl = (int)t.pattern_len, tl = (int)t.text_len;
    const int kend = tl - pl;
    const int s = scores[ti];
    // the union of the diamond ranges is [ceil((kend - s) / 2), floor((kend + s) / 2)] clamped: the host sized CAP / gcap from it
    int kmin;
    SpanGeom g = {0, 0, kend, kend};
    if constexpr (EF) {
      int kmax;
      g = span_geom(t, pl, tl);
      span_union(s, g, pl, tl, &kmin, &kmax);
    } else {
      kmin = kend - s; kmin = kmin >= 0 ? kmin / 2 : -((-kmin) / 2);
      if (kmin < -pl) kmin = -pl;
    }
    const int kbase = kmin - 1;                   // one spare slot below, one above: reads of k +- 1 stay inside
    auto range = [&](int sc, int* lo, int* hi) {
      if constexpr (EF) span_range(sc, s, g, pl, tl, lo, hi);
      else diamond_range(sc, s, kend, pl, tl, lo, hi);
    };
    const int pef = EF ? t.pattern_end_free : 0, tef = EF ? t.text_end_free : 0;
    int k_fin = kend, h_fin = tl;                 // EF: the ending cell
    bool found = false;
    uint8_t* const prow0 = prov + jb.prov_off;
    uint64_t row = 0;
    int lo_prev = 0, hi_prev = 0;
    bool ok = true;
    for (int sc = 0; sc <= s; ++sc) {
      int lo, hi;
      range(sc, &lo, &hi);
      // left neighbour of the first chunk: the diamond of score sc - 1 is wider, so (sc - 1, lo - 1) can be a live cell
      int carry = (sc > 0 && lo - 1 >= lo_prev && lo - 1 <= hi_prev) ? wf_rd(lo - 1 - kbase) : OTG_NULL_OFF;
      for (int c = lo; c <= hi; c += 64) {
        const int k = c + lane;
        const int j = k - kbase;
        const bool in = k <= hi;
        int mx;
        uint32_t op = 0;
        if (sc == 0) {
          mx = EF ? (k > 0 ? k : 0) : 0;
        } else {
          const int o = (in && k >= lo_prev && k <= hi_prev) ? wf_rd(j) : OTG_NULL_OFF;
          const int r = (in && k + 1 >= lo_prev && k + 1 <= hi_prev) ? wf_rd(j + 1) : OTG_NULL_OFF;
          int l = __shfl_up(o, 1);
          if (lane == 0) l = carry;
          carry = __shfl(o, 63);
          const int ins = l + 1, del = r, misms = o + 1;
          mx = ins > del ? ins : del;
          mx = misms > mx ? misms : mx;
          if (mx == ins) op = OP_INS;
          if (mx == del) op = OP_DEL;
          if (mx == misms) op = OP_MISMS;
        }
        int h = mx, v = mx - k;
        const bool valid = in && mx >= 0 && v >= 0 && h <= tl && v <= pl;
        if (valid && v < pl && h < tl) {
          const int rem = pl - v < tl - h ? pl - v : tl - h;
          int m = otg_match64(P, T, v, h, rem);
          v += m; h += m;
          while (m == 64 && v < pl && h < tl) {
            const int rem2 = pl - v < tl - h ? pl - v : tl - h;
            m = otg_match64(P, T, v, h, rem2);
            v += m; h += m;
          }
        }
        if (in) wf_wr(j, valid ? h : OTG_NULL_OFF);
        if (sc > 0) {
          const unsigned long long b0 = __ballot(in && (op & 1u));
          const unsigned long long b1 = __ballot(in && (op & 2u));
          uint64_t* dst = (uint64_t*)(prow0 + row + (uint64_t)((c - lo) >> 6) * 16u);
          if (lane == 0) dst[0] = b0;
          if (lane == 1) dst[1] = b1;
        }
        if constexpr (EF) {
          // the end test, on the last row only: chunks come in ascending order, so the lowest lane of the first chunk that has one wins
          if (sc == s && !found) {
            const unsigned long long fb = __ballot(valid && otg_ends_free_done(h, v, pl, tl, pef, tef));
            if (fb) {
              const int fl = (int)__builtin_ctzll(fb);
              found = true; k_fin = c + fl; h_fin = __shfl(h, fl);
            }
          }
        }
      }
      if (sc > 0) row += prov_row_bytes(lo, hi);
      lo_prev = lo; hi_prev = hi;
    }
    // the end cell must have been reached at score s (else the score chain and this pass disagree)
    if constexpr (EF) { if (!found) ok = false; }
    else if (kend < lo_prev || kend > hi_prev || wf_rd(kend - kbase) < tl) ok = false;
    // ---- backtrace (lane 0): ops in forward order
    uint8_t* const opv = ops + jb.ops_off;
    uint32_t n_ins = 0;
    int k_begin = 0;
    if (ok && lane == 0)
      n_ins = edit_backtrace(prow0, row, s, k_fin, opv, range, EF ? g.slo : 0, EF ? g.shi : 0, &k_begin);
    __threadfence_block();                        // lane 0's op stores before the whole wave reads them back
    n_ins = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_ins);
    if (n_ins == 0xFFFFFFFFu) ok = false;
    if (!ok) {
      if (lane == 0) stat[ti] = -2;
      continue;
    }
    // ---- unpack (whole wave): maximal match run, then per op the op and a maximal match run
    if constexpr (EF) {
      k_begin = __builtin_amdgcn_readfirstlane(k_begin);
      if (cig && !edit_unpack_span(P, T, pl, tl, s, opv, cig + jb.cig_off, lane, k_begin, k_fin, h_fin)) { if (lane == 0) stat[ti] = -3; continue; }
      // columns = pl + every I: the free ones in front (a start on a positive diagonal), the operations, the ones up to the end of the text
      if (lane == 0) { cig_len[ti] = (uint32_t)pl + (uint32_t)(k_begin > 0 ? k_begin : 0) + n_ins + (uint32_t)(tl - h_fin); stat[ti] = s; }
      continue;
    }
    if (cig && !edit_unpack(P, T, pl, tl, s, opv, cig + jb.cig_off, lane)) { if (lane == 0) stat[ti] = -3; continue; }
    if (lane == 0) { cig_len[ti] = (uint32_t)pl + n_ins; stat[ti] = s; }
  }
}

// ---------------------------------------------------------------------------------------------------
// The provenance pass under wfadaptive.  Step 1 (the adaptive score chain, wfa_adaptive.hip) gave the score s and the cell
// count W = the sum over the scores of the wavefront's width before the cut; the host sized this task's provenance from them: a row of
// width w takes ceil(w / 64) * 16 bytes, so all rows fit W / 4 + 16 (s + 1) bytes, and behind them a table of the (lo, hi) of every score.
// ONE wave64 per alignment, lanes = diagonals, chunks of 64 in ascending order, the wavefront (int32 offsets: no length limit) updated in
// place with the left neighbour carried, in a modular LDS window (slot = k mod CAP) or, for a wavefront wider than the window, in a row of
// HBM: the LDS tier puts such a task on a list and the global-row tier runs it again from score 0 into the same provenance slot.
// Per score t: the range is the post-cut range of t - 1 grown by one diagonal either side (clamped to the matrix); sources outside that
// post-cut range are null; provenance rule, nulling and extension as in the exact kernel; two ballots per chunk; the end test on kend;
// otherwise the cut (wfadaptive_cut, the code the score chain runs).  The pass is deterministic, so it has to end at the chain's score with
// the chain's cell count: anything else is reported in stat (the host turns it into OTG_ERR_FATAL).
struct AdaptiveJob {
  uint64_t prov_off;      // into the provenance arena (bytes, 16-aligned): the rows
  uint64_t prov_cap;      // bytes the rows may take
  uint64_t rng_off;       // into the provenance arena: s + 1 pairs (lo, hi)
  uint64_t ops_off;       // into the op buffer (s bytes)
  uint64_t cig_off;       // into the device cigar arena (ignored when no cigar is produced)
};

__device__ __forceinline__ int wave_min_i32(int v) { return -otg_wave_max_i32(-v); }      // |v| <= 2^30 here

template <int CAP>
struct AdWfLds {
  volatile lds_i32* wf;
  __device__ __forceinline__ int rd(int k) const { return wf[k & (CAP - 1)]; }
  __device__ __forceinline__ void wr(int k, int h) const { wf[k & (CAP - 1)] = h; }
  __device__ __forceinline__ void sync() const {}
};
struct AdWfGlobal {
  volatile int32_t* wf; int kb;      // wf[k + kb], -pl - 1 <= k <= tl + 1
  __device__ __forceinline__ int rd(int k) const { return wf[k + kb]; }
  __device__ __forceinline__ void wr(int k, int h) const { wf[k + kb] = h; }
  __device__ __forceinline__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }      // a cell is read back by other lanes than the one that stored it
};

// stat[ti] = s on success; untouched (-1) while the task waits on the LDS tier's overflow list; -2: the pass did not end at the chain's score, or the
// backtrace failed; -3: the unpacked string does not end at (plen, tlen); -4: the rows outgrew their slot; -5: the cell counts differ.
// CAP == 0: the global-row tier (gws: gcap offsets per wave).
// EF: tasks with free ends — score 0 covers S, the distances and the limits of the cut are the ends-free ones (the code the score chain runs
// for such a task), the pass ends on the lowest diagonal whose cell satisfies the ends-free end test, the walk back ends on a diagonal of S.
template <int CAP, int WPB, bool EF>
__global__ __launch_bounds__(WPB * 64) void edit_align_adaptive_kernel(
    const uint8_t* __restrict__ arena, const otg_align_task* __restrict__ tasks, const int32_t* __restrict__ scores, const uint64_t* __restrict__ cells,
    const uint32_t* __restrict__ todo, const uint32_t* __restrict__ n_todo_ptr, uint32_t n_todo_imm, const AdaptiveJob* __restrict__ jobs,
    uint8_t* __restrict__ prov, uint8_t* __restrict__ ops, uint8_t* __restrict__ cig, uint32_t* __restrict__ cig_len,
    int32_t* __restrict__ stat, uint32_t* __restrict__ ticket, uint32_t* __restrict__ n_overflow, uint32_t* __restrict__ overflow_list,
    uint32_t* __restrict__ n_finished, otg_adaptive::Heur H, int32_t* gws, int gcap)
{
  constexpr bool GLOBAL_WF = CAP == 0;
  constexpr int LCAP = GLOBAL_WF ? 2 : CAP;
  __shared__ __attribute__((aligned(16))) int32_t s_wf[WPB][LCAP];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const uint32_t n_todo = n_todo_ptr ? *n_todo_ptr : n_todo_imm;

  for (;;) {
    const uint32_t tk = otg_wave_atomic_add(ticket, 1u);
    if (tk >= n_todo) break;
    const uint32_t ti = todo[tk];
    const otg_align_task t = tasks[ti];
    const AdaptiveJob jb = jobs[ti];
    const uint8_t* P = arena + t.pattern_off;
    const uint8_t* T = arena + t.text_off;
    const int pl = (int)t.pattern_len, tl = (int)t.text_len;
    const int kend = tl - pl;
    const int s = scores[ti];
    const uint64_t W_want = cells[ti];
    uint8_t* const prow0 = prov + jb.prov_off;
    int2* const rng = (int2*)(prov + jb.rng_off);
    uint64_t row = 0;
    const SpanGeom g = EF ? span_geom(t, pl, tl) : SpanGeom{0, 0, kend, kend};
    const int pef = EF ? t.pattern_end_free : 0, tef = EF ? t.text_end_free : 0;
    int k_fin = kend, h_fin = tl;                   // EF: the ending cell
    // 0: ended at score sc; 1: the wavefront outgrew the window; < 0: a stat code
    auto pass = [&](auto st) -> int {
      int lo = EF ? g.slo : 0, hi = EF ? g.shi : 0, plo = 0, phi = 0;      // the range of this score; the range of the previous one after its cut
      int sc = 0, steps_wait = 0;
      uint64_t W = 0;
      for (;;) {
        if (!GLOBAL_WF && hi - lo + 1 > CAP) return 1;
        if (sc > s) return -2;
        const uint64_t rb = sc > 0 ? prov_row_bytes(lo, hi) : 0u;
        if (row + rb > jb.prov_cap) return -4;
        W += (uint64_t)(hi - lo + 1);
        if (lane == 0) rng[sc] = make_int2(lo, hi);
        int carry = OTG_NULL_OFF;                   // (the diagonal below lo is never inside the previous range)
        int dmin = otg_adaptive::BIG;               // per lane: smallest left_to_align among its cells
        int kfin = otg_adaptive::BIG;               // per lane (EF): lowest of its diagonals whose cell may end the alignment
        for (int c = lo; c <= hi; c += 64) {
          const int k = c + lane;
          const bool in = k <= hi;
          int mx;
          uint32_t op = 0;
          if (sc == 0) {
            mx = EF ? (k > 0 ? k : 0) : 0;
          } else {
            const int o = (in && k >= plo && k <= phi) ? st.rd(k) : OTG_NULL_OFF;
            const int r = (in && k + 1 >= plo && k + 1 <= phi) ? st.rd(k + 1) : OTG_NULL_OFF;
            int l = __shfl_up(o, 1);
            if (lane == 0) l = carry;
            carry = __shfl(o, 63);
            const int ins = l + 1, del = r, misms = o + 1;
            mx = ins > del ? ins : del;
            mx = misms > mx ? misms : mx;
            if (mx == ins) op = OP_INS;
            if (mx == del) op = OP_DEL;
            if (mx == misms) op = OP_MISMS;
          }
          int h = mx, v = mx - k;
          const bool valid = in && mx >= 0 && v >= 0 && h <= tl && v <= pl;
          if (valid && v < pl && h < tl) {
            const int rem = pl - v < tl - h ? pl - v : tl - h;
            int m = otg_match64(P, T, v, h, rem);
            v += m; h += m;
            while (m == 64 && v < pl && h < tl) {
              const int rem2 = pl - v < tl - h ? pl - v : tl - h;
              m = otg_match64(P, T, v, h, rem2);
              v += m; h += m;
            }
          }
          if (in) st.wr(k, valid ? h : OTG_NULL_OFF);
          if (valid) dmin = otg_adaptive::imin(dmin, otg_adaptive::left_to_align(h, k, pl, tl, EF, pef, tef));
          if constexpr (EF) { if (valid && otg_ends_free_done(h, v, pl, tl, pef, tef)) kfin = otg_adaptive::imin(kfin, k); }
          if (sc > 0) {
            const unsigned long long b0 = __ballot(in && (op & 1u));
            const unsigned long long b1 = __ballot(in && (op & 2u));
            uint64_t* dst = (uint64_t*)(prow0 + row + (uint64_t)((c - lo) >> 6) * 16u);
            if (lane == 0) dst[0] = b0;
            if (lane == 1) dst[1] = b1;
          }
        }
        row += rb;
        st.sync();
        // ---- end test on the extended wavefront
        if constexpr (EF) {
          const int kf = wave_min_i32(kfin);
          if (kf < otg_adaptive::BIG) {
            if (sc != s) return -2;
            k_fin = kf; h_fin = __builtin_amdgcn_readfirstlane(st.rd(kf));
            return W == W_want ? 0 : -5;
          }
        } else if (kend >= lo && kend <= hi && __builtin_amdgcn_readfirstlane(st.rd(kend)) >= tl) {
          if (sc != s) return -2;
          return W == W_want ? 0 : -5;
        }
        // ---- the cut
        const int mind = wave_min_i32(dmin);
        otg_adaptive::wfadaptive_cut(H, steps_wait, mind, pl, tl, EF, pef, tef, lo, hi, lane, [&](int k) { return st.rd(k); });
        plo = lo; phi = hi;
        lo = lo - 1 < -pl ? -pl : lo - 1;
        hi = hi + 1 > tl ? tl : hi + 1;
        ++sc;
      }
    };
    int rc;
    if constexpr (GLOBAL_WF) {
      if (pl + tl + 3 > gcap) rc = -4;            // (the host sizes the rows for the longest pair of the batch)
      else rc = pass(AdWfGlobal{(volatile int32_t*)(gws + (size_t)(blockIdx.x * WPB + wib) * (size_t)gcap), pl + 1});
    } else {
      rc = pass(AdWfLds<CAP>{(volatile lds_i32*)&s_wf[wib][0]});
    }
    if (rc == 1) {                                // wave-uniform: every lane stores the same value to the same address
      const uint32_t q = otg_wave_atomic_add(n_overflow, 1u);
      overflow_list[q] = ti;
      continue;
    }
    if (rc < 0) {
      if (lane == 0) stat[ti] = rc;
      continue;
    }
    // ---- backtrace (lane 0) through the range table, then the unpack (whole wave)
    __threadfence_block();                        // the ballots and the table (lanes 0 and 1) before lane 0 reads them back
    uint8_t* const opv = ops + jb.ops_off;
    uint32_t n_ins = 0;
    int k_begin = 0;
    if (lane == 0)
      n_ins = edit_backtrace(prow0, row, s, k_fin, opv, [&](int sc, int* lo, int* hi) { const int2 r = rng[sc]; *lo = r.x; *hi = r.y; },
                             g.slo, g.shi, &k_begin);
    __threadfence_block();                        // lane 0's op stores before the whole wave reads them back
    n_ins = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_ins);
    if (n_ins == 0xFFFFFFFFu) {
      if (lane == 0) stat[ti] = -2;
      continue;
    }
    if constexpr (EF) {
      k_begin = __builtin_amdgcn_readfirstlane(k_begin);
      if (cig && !edit_unpack_span(P, T, pl, tl, s, opv, cig + jb.cig_off, lane, k_begin, k_fin, h_fin)) { if (lane == 0) stat[ti] = -3; continue; }
      if (lane == 0) { cig_len[ti] = (uint32_t)pl + (uint32_t)(k_begin > 0 ? k_begin : 0) + n_ins + (uint32_t)(tl - h_fin); stat[ti] = s; }
    } else {
      if (cig && !edit_unpack(P, T, pl, tl, s, opv, cig + jb.cig_off, lane)) { if (lane == 0) stat[ti] = -3; continue; }
      if (lane == 0) { cig_len[ti] = (uint32_t)pl + n_ins; stat[ti] = s; }
    }
    (void)otg_wave_atomic_add(n_finished, 1u);
  }
}

} // namespace

// Host side of otg_edit_align_batch / otg_edit_align_span_batch: scores first (the existing chain), then the provenance pass in chunks bounded
// by a memory budget.  Tasks with free ends (endsfree != 0) run on the kernels' EF instantiations, the others on the end-to-end ones.
// d_arena / d_tasks resident (arena padded by >= 64 readable bytes); h_tasks the same tasks on the host.  Fills scores_out, len_out and,
// when d_cig_base is non-null, the op strings at d_cig_base + cig_slot[i] (cig_slot: n_tasks entries, host).
int otg_launch_edit_align(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const otg_align_task* h_tasks, uint32_t n_tasks,
                          int32_t* scores_out, uint32_t* len_out, uint8_t* d_cig_base, const uint64_t* cig_slot, double* score_ms, double* prov_ms,
                          uint32_t* finished)
{
  if (n_tasks == 0) return OTG_OK;
  int32_t* d_scores = (int32_t*)otg_slot(ctx, SLOT_SCORES, (size_t)n_tasks * sizeof(int32_t));
  uint64_t* d_cells = (uint64_t*)otg_slot(ctx, SLOT_CELLS, (size_t)n_tasks * sizeof(uint64_t));
  if (!d_scores || !d_cells) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemsetAsync(d_scores, 0xff, (size_t)n_tasks * sizeof(int32_t), ctx->stream));
  float sms = 0;
  int rc = otg_launch_edit(ctx, d_arena, d_tasks, n_tasks, d_scores, d_cells, score_ms ? &sms : nullptr, nullptr);
  if (rc) return rc;
  if (score_ms) *score_ms = sms;
  HIP_TRY(ctx, hipMemcpyAsync(scores_out, d_scores, (size_t)n_tasks * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t i = 0; i < n_tasks; ++i)
    if (scores_out[i] < 0) return otg_fail(ctx, OTG_ERR_FATAL, "edit task %u did not terminate", i);

  // per task: provenance bytes (exact, the same row sizes the kernel walks), op bytes, wavefront width
  std::vector<AlignJob> jobs(n_tasks);
  std::vector<uint64_t> pbytes(n_tasks);
  std::vector<int> width(n_tasks);
  for (uint32_t i = 0; i < n_tasks; ++i) {
    const int pl = (int)h_tasks[i].pattern_len, tl = (int)h_tasks[i].text_len, s = scores_out[i], kend = tl - pl;
    uint64_t b = 0;
    int kmin, kmax;
    if (h_tasks[i].endsfree) {
      const SpanGeom g = span_geom(h_tasks[i], pl, tl);
      for (int sc = 1; sc <= s; ++sc) { int lo, hi; span_range(sc, s, g, pl, tl, &lo, &hi); b += prov_row_bytes(lo, hi); }
      span_union(s, g, pl, tl, &kmin, &kmax);
    } else {
      for (int sc = 1; sc <= s; ++sc) { int lo, hi; diamond_range(sc, s, kend, pl, tl, &lo, &hi); b += prov_row_bytes(lo, hi); }
      kmin = kend - s; kmin = kmin >= 0 ? kmin / 2 : -((-kmin) / 2); if (kmin < -pl) kmin = -pl;
      kmax = kend + s; kmax = kmax >= 0 ? kmax / 2 : -((-kmax + 1) / 2); if (kmax > tl) kmax = tl;
    }
    pbytes[i] = b;
    width[i] = kmax - kmin + 3;
    jobs[i].cig_off = cig_slot ? cig_slot[i] : 0;
  }
  // chunks: consecutive tasks while the provenance + op bytes stay within the budget (a single larger task gets a chunk of its own)
  static const uint64_t budget = (uint64_t)otg_env_int("OTG_EDIT_ALIGN_BUDGET_MB", 2048) << 20;
  constexpr int CAP = 2048, WPB = 4;
  float ms_total = 0;
  uint32_t c0 = 0;
  while (c0 < n_tasks) {
    uint32_t c1 = c0;
    uint64_t pb = 0, ob = 0;
    int gmax = 0;
    while (c1 < n_tasks) {
      const uint64_t add_p = pbytes[c1], add_o = ((uint64_t)scores_out[c1] + 15) & ~15ull;
      if (c1 > c0 && pb + ob + add_p + add_o > budget) break;
      jobs[c1].prov_off = pb; jobs[c1].ops_off = ob;
      pb += add_p; ob += add_o;
      if (width[c1] > CAP) gmax = std::max(gmax, width[c1]);
      ++c1;
    }
    const uint32_t n = c1 - c0;
    std::vector<uint32_t> lds_list, glb_list, lds_ef, glb_ef;
    for (uint32_t i = c0; i < c1; ++i) {
      if (h_tasks[i].endsfree) (width[i] <= CAP ? lds_ef : glb_ef).push_back(i);
      else (width[i] <= CAP ? lds_list : glb_list).push_back(i);
    }
    uint8_t* d_prov = (uint8_t*)otg_slot(ctx, SLOT_BT_POOL, pb + 64);
    uint8_t* d_ops = (uint8_t*)otg_slot(ctx, SLOT_REVOPS, ob + 64);
    AlignJob* d_jobs = (AlignJob*)otg_slot(ctx, SLOT_AUX1, (size_t)n_tasks * sizeof(AlignJob));
    uint32_t* d_todo = (uint32_t*)otg_slot(ctx, SLOT_AUX2, ((size_t)n + 16) * sizeof(uint32_t));
    uint32_t* d_len = (uint32_t*)otg_slot(ctx, SLOT_CIG_LEN, (size_t)n_tasks * sizeof(uint32_t));
    int32_t* d_stat = (int32_t*)otg_slot(ctx, SLOT_AUX3, (size_t)n_tasks * sizeof(int32_t));
    if (!d_prov || !d_ops || !d_jobs || !d_todo || !d_len || !d_stat) return OTG_ERR_HIP;
    uint32_t* d_tick = d_todo + n;            // one ticket counter per list after the todo list
    std::vector<uint32_t> todo(lds_list);
    todo.insert(todo.end(), glb_list.begin(), glb_list.end());
    todo.insert(todo.end(), lds_ef.begin(), lds_ef.end());
    todo.insert(todo.end(), glb_ef.begin(), glb_ef.end());
    HIP_TRY(ctx, hipMemcpyAsync(d_jobs + c0, jobs.data() + c0, (size_t)n * sizeof(AlignJob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_todo, todo.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_tick, 0, 16 * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_stat + c0, 0xff, (size_t)n * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (!lds_list.empty()) {
      const uint32_t want = ((uint32_t)lds_list.size() + WPB - 1) / WPB;
      const uint32_t grid = std::min<uint32_t>((uint32_t)ctx->n_cu * 4, want);
      hipLaunchKernelGGL((edit_align_kernel<CAP, WPB, false, false>), dim3(grid), dim3(WPB * 64), (size_t)CAP * WPB * sizeof(int32_t), ctx->stream,
                         d_arena, d_tasks, d_scores, d_todo, (uint32_t)lds_list.size(), d_jobs, d_prov, d_ops, d_cig_base, d_len, d_stat, d_tick,
                         (int32_t*)nullptr, 0);
    }
    if (!lds_ef.empty()) {
      const uint32_t want = ((uint32_t)lds_ef.size() + WPB - 1) / WPB;
      const uint32_t grid = std::min<uint32_t>((uint32_t)ctx->n_cu * 4, want);
      hipLaunchKernelGGL((edit_align_kernel<CAP, WPB, false, true>), dim3(grid), dim3(WPB * 64), (size_t)CAP * WPB * sizeof(int32_t), ctx->stream,
                         d_arena, d_tasks, d_scores, d_todo + lds_list.size() + glb_list.size(), (uint32_t)lds_ef.size(), d_jobs, d_prov, d_ops,
                         d_cig_base, d_len, d_stat, d_tick + 2, (int32_t*)nullptr, 0);
    }
    if (!glb_list.empty() || !glb_ef.empty()) {
      // the two global-row launches follow each other on the stream: one workspace, sized for the larger grid
      constexpr int GW = 4;
      const uint32_t grid_a = std::min<uint32_t>((uint32_t)ctx->n_cu, ((uint32_t)glb_list.size() + GW - 1) / GW);
      const uint32_t grid_b = std::min<uint32_t>((uint32_t)ctx->n_cu, ((uint32_t)glb_ef.size() + GW - 1) / GW);
      const int gcap = gmax + 64;
      int32_t* ws = (int32_t*)otg_slot(ctx, SLOT_WF_WS, (size_t)std::max(grid_a, grid_b) * GW * (size_t)gcap * sizeof(int32_t));
      if (!ws) return OTG_ERR_HIP;
      if (grid_a)
        hipLaunchKernelGGL((edit_align_kernel<0, GW, true, false>), dim3(grid_a), dim3(GW * 64), 0, ctx->stream,
                           d_arena, d_tasks, d_scores, d_todo + lds_list.size(), (uint32_t)glb_list.size(), d_jobs, d_prov, d_ops, d_cig_base, d_len,
                           d_stat, d_tick + 1, ws, gcap);
      if (grid_b)
        hipLaunchKernelGGL((edit_align_kernel<0, GW, true, true>), dim3(grid_b), dim3(GW * 64), 0, ctx->stream,
                           d_arena, d_tasks, d_scores, d_todo + lds_list.size() + glb_list.size() + lds_ef.size(), (uint32_t)glb_ef.size(), d_jobs, d_prov,
                           d_ops, d_cig_base, d_len, d_stat, d_tick + 3, ws, gcap);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    std::vector<int32_t> stat(n);
    HIP_TRY(ctx, hipMemcpyAsync(len_out + c0, d_len + c0, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(stat.data(), d_stat + c0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = otg_timer_add(ctx, &ms_total, nullptr)) return rc;
    for (uint32_t i = 0; i < n; ++i)
      if (stat[i] != scores_out[c0 + i])
        return otg_fail(ctx, OTG_ERR_FATAL, "edit alignment task %u: provenance pass failed (code %d, score %d)", c0 + i, stat[i], scores_out[c0 + i]);
    if (finished) { finished[0] += (uint32_t)(lds_list.size() + lds_ef.size()); finished[1] += (uint32_t)(glb_list.size() + glb_ef.size()); }
    c0 = c1;
  }
  if (prov_ms) *prov_ms = ms_total;
  return OTG_OK;
}

// Host side of otg_edit_align_heur_batch under wfadaptive: the caller has set ctx's heuristic for the score chain (and restores it).  As
// otg_launch_edit_align; additionally fills cells_out (host, n_tasks) and adds to finished[0] / [1] the tasks the LDS tier / the global-row tier finished.
int otg_launch_edit_align_adaptive(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const otg_align_task* h_tasks, uint32_t n_tasks,
                                   int32_t* scores_out, uint64_t* cells_out, uint32_t* len_out, uint8_t* d_cig_base, const uint64_t* cig_slot,
                                   double* score_ms, double* prov_ms, uint32_t finished[2])
{
  if (n_tasks == 0) return OTG_OK;
  int32_t* d_scores = (int32_t*)otg_slot(ctx, SLOT_SCORES, (size_t)n_tasks * sizeof(int32_t));
  uint64_t* d_cells = (uint64_t*)otg_slot(ctx, SLOT_CELLS, (size_t)n_tasks * sizeof(uint64_t));
  if (!d_scores || !d_cells) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemsetAsync(d_scores, 0xff, (size_t)n_tasks * sizeof(int32_t), ctx->stream));
  float sms = 0;
  int rc = otg_launch_edit(ctx, d_arena, d_tasks, n_tasks, d_scores, d_cells, score_ms ? &sms : nullptr, nullptr);
  if (rc) return rc;
  if (score_ms) *score_ms = sms;
  HIP_TRY(ctx, hipMemcpyAsync(scores_out, d_scores, (size_t)n_tasks * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(cells_out, d_cells, (size_t)n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t i = 0; i < n_tasks; ++i)
    if (scores_out[i] < 0) return otg_fail(ctx, OTG_ERR_FATAL, "edit task %u did not terminate", i);

  // per task: the bytes of its rows (the bound from the cell count: ceil(w / 64) * 16 <= w / 4 + 16 per row) and of its range table
  std::vector<AdaptiveJob> jobs(n_tasks);
  std::vector<uint64_t> pbytes(n_tasks);
  for (uint32_t i = 0; i < n_tasks; ++i) {
    const uint64_t s = (uint64_t)scores_out[i];
    jobs[i].prov_cap = (cells_out[i] / 4 + 16 * (s + 1) + 15) & ~15ull;
    pbytes[i] = jobs[i].prov_cap + (((s + 1) * sizeof(int2) + 15) & ~15ull);
    jobs[i].cig_off = cig_slot ? cig_slot[i] : 0;
  }
  static const uint64_t budget = (uint64_t)otg_env_int("OTG_EDIT_ALIGN_BUDGET_MB", 2048) << 20;
  // test switch, bit mask of the tiers that run: 1 the LDS window, 2 the global row
  static const int tiers = otg_env_int("OTG_EDIT_ALIGN_ADAPTIVE_TIERS", 3);
  const otg_adaptive::Heur H{ctx->heur_min_wf_len, ctx->heur_max_dist, ctx->heur_steps < 1 ? 1 : ctx->heur_steps};
  constexpr int CAP = 2048, WPB = 4, GW = 4;
  float ms_total = 0;
  uint32_t c0 = 0;
  while (c0 < n_tasks) {
    uint32_t c1 = c0;
    uint64_t pb = 0, ob = 0;
    int gcap = 0;
    while (c1 < n_tasks) {
      const uint64_t add_p = pbytes[c1], add_o = ((uint64_t)scores_out[c1] + 15) & ~15ull;
      if (c1 > c0 && pb + ob + add_p + add_o > budget) break;
      jobs[c1].prov_off = pb; jobs[c1].rng_off = pb + jobs[c1].prov_cap; jobs[c1].ops_off = ob;
      pb += add_p; ob += add_o;
      gcap = std::max(gcap, (int)(h_tasks[c1].pattern_len + h_tasks[c1].text_len + 3));
      ++c1;
    }
    const uint32_t n = c1 - c0;
    const uint32_t grid_g = std::min<uint32_t>((uint32_t)ctx->n_cu, (n + GW - 1) / GW);
    uint8_t* d_prov = (uint8_t*)otg_slot(ctx, SLOT_BT_POOL, pb + 64);
    uint8_t* d_ops = (uint8_t*)otg_slot(ctx, SLOT_REVOPS, ob + 64);
    AdaptiveJob* d_jobs = (AdaptiveJob*)otg_slot(ctx, SLOT_AUX1, (size_t)n_tasks * sizeof(AdaptiveJob));
    uint32_t* d_todo = (uint32_t*)otg_slot(ctx, SLOT_AUX2, (2 * (size_t)n + 16) * sizeof(uint32_t));      // the tasks | 16 counters | the LDS tier's overflow list
    uint32_t* d_len = (uint32_t*)otg_slot(ctx, SLOT_CIG_LEN, (size_t)n_tasks * sizeof(uint32_t));
    int32_t* d_stat = (int32_t*)otg_slot(ctx, SLOT_AUX3, (size_t)n_tasks * sizeof(int32_t));
    int32_t* ws = (tiers & 2) ? (int32_t*)otg_slot(ctx, SLOT_WF_WS, (size_t)grid_g * GW * (size_t)gcap * sizeof(int32_t)) : nullptr;
    if (!d_prov || !d_ops || !d_jobs || !d_todo || !d_len || !d_stat || ((tiers & 2) && !ws)) return OTG_ERR_HIP;
    // [0] [1] the tiers' tickets, [2] length of the overflow list, [3] [4] tasks finished per tier; [6] [7] [8] tickets and overflow of the
    // tasks with free ends, which follow the end-to-end ones in the todo list and in the overflow list
    uint32_t* d_cnt = d_todo + n;
    uint32_t* d_over = d_cnt + 16;
    std::vector<uint32_t> todo, todo_ef;
    for (uint32_t i = 0; i < n; ++i) (h_tasks[c0 + i].endsfree ? todo_ef : todo).push_back(c0 + i);
    const uint32_t n_e2e = (uint32_t)todo.size(), n_ef = (uint32_t)todo_ef.size();
    todo.insert(todo.end(), todo_ef.begin(), todo_ef.end());
    HIP_TRY(ctx, hipMemcpyAsync(d_jobs + c0, jobs.data() + c0, (size_t)n * sizeof(AdaptiveJob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_todo, todo.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, 16 * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_stat + c0, 0xff, (size_t)n * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (n_e2e) {
      OtgTodo in{d_todo, nullptr, n_e2e};
      if (tiers & 1) {
        const uint32_t grid = std::min<uint32_t>((uint32_t)ctx->n_cu * 4, (n_e2e + WPB - 1) / WPB);
        hipLaunchKernelGGL((edit_align_adaptive_kernel<CAP, WPB, false>), dim3(grid), dim3(WPB * 64), 0, ctx->stream,
                           d_arena, d_tasks, d_scores, d_cells, in.list, in.n, in.imm, d_jobs, d_prov, d_ops, d_cig_base, d_len, d_stat,
                           d_cnt, d_cnt + 2, d_over, d_cnt + 3, H, (int32_t*)nullptr, 0);
        in.next(d_over, d_cnt + 2);
      }
      if (tiers & 2) {
        hipLaunchKernelGGL((edit_align_adaptive_kernel<0, GW, false>), dim3(std::min<uint32_t>(grid_g, (n_e2e + GW - 1) / GW)), dim3(GW * 64), 0, ctx->stream,
                           d_arena, d_tasks, d_scores, d_cells, in.list, in.n, in.imm, d_jobs, d_prov, d_ops, d_cig_base, d_len, d_stat,
                           d_cnt + 1, d_cnt + 5, d_over, d_cnt + 4, H, ws, gcap);
      }
    }
    if (n_ef) {
      OtgTodo in{d_todo + n_e2e, nullptr, n_ef};
      uint32_t* const over_ef = d_over + n_e2e;
      if (tiers & 1) {
        const uint32_t grid = std::min<uint32_t>((uint32_t)ctx->n_cu * 4, (n_ef + WPB - 1) / WPB);
        hipLaunchKernelGGL((edit_align_adaptive_kernel<CAP, WPB, true>), dim3(grid), dim3(WPB * 64), 0, ctx->stream,
                           d_arena, d_tasks, d_scores, d_cells, in.list, in.n, in.imm, d_jobs, d_prov, d_ops, d_cig_base, d_len, d_stat,
                           d_cnt + 6, d_cnt + 8, over_ef, d_cnt + 3, H, (int32_t*)nullptr, 0);
        in.next(over_ef, d_cnt + 8);
      }
      if (tiers & 2) {
        hipLaunchKernelGGL((edit_align_adaptive_kernel<0, GW, true>), dim3(std::min<uint32_t>(grid_g, (n_ef + GW - 1) / GW)), dim3(GW * 64), 0, ctx->stream,
                           d_arena, d_tasks, d_scores, d_cells, in.list, in.n, in.imm, d_jobs, d_prov, d_ops, d_cig_base, d_len, d_stat,
                           d_cnt + 7, d_cnt + 9, over_ef, d_cnt + 4, H, ws, gcap);
      }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    std::vector<int32_t> stat(n);
    uint32_t cnt[16];
    HIP_TRY(ctx, hipMemcpyAsync(len_out + c0, d_len + c0, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(stat.data(), d_stat + c0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc2 = otg_timer_add(ctx, &ms_total, nullptr)) return rc2;
    finished[0] += cnt[3]; finished[1] += cnt[4];
    for (uint32_t i = 0; i < n; ++i)
      if (stat[i] != scores_out[c0 + i])
        return otg_fail(ctx, OTG_ERR_FATAL, "edit alignment task %u: adaptive provenance pass failed (code %d, score %d, cells %llu)", c0 + i, stat[i],
                        scores_out[c0 + i], (unsigned long long)cells_out[c0 + i]);
    c0 = c1;
  }
  if (prov_ms) *prov_ms = ms_total;
  return OTG_OK;
}

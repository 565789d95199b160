// myers_edit.hip — banded bit-parallel edit distance (Myers 1999 / Hyyrö 2003 block formulation), gfx950.
//
// Second engine behind otg_edit_distance_batch / the pipeline's distance stages.  Unit-cost edit distance has a
// unique optimum, so any exact algorithm returns what WFAlignerEdit::getAlignmentScore() returns
// (reference call sites src/analignments.cpp:70-71,88-97).  The wavefront kernel (wfa_edit.hip) costs O(s^2) and
// is unbeatable for HiFi-like pairs (s ~ 0..50); for ONT-error reads (s = 0.1..0.4 L) this kernel costs
// O(n) wave-steps regardless of s.
//
// Mapping: a GROUP of GL lanes (16, 32 or 64) per pair, 64/GL pairs per wave.  The DP matrix (pattern = rows,
// text = columns) is cut into 64-row blocks held as vertical-delta bit-vectors (Pv, Mv: 64-bit).  Lane l of a
// group owns "superblocks" l, l+GL, ... (BPL consecutive blocks each) and at time step t processes column
// j = t - B of its superblock B: the anti-diagonal skew turns the block-to-block carry (hout -> hin) into a
// one-lane rotate per step (DPP row_ror for 16-lane groups, ds_bpermute for 32, wave_ror for 64).  Only the
// Ukkonen band -KL <= i - j <= KU (KL = (K - d)/2, KU = (K + d)/2 for a global alignment, d = m - n >= 0) is evaluated; a superblock enters the band initialised as in
// Edlib (Pv = ~0, score = score_above + rows) and the block at the top of the band takes hin = +1.  With
// KL + KU <= (GL-1)*64*BPL + GL (i.e. K up to about that many rows) a lane has left its superblock before the next one (B + GL) enters the band, so
// narrow bands (within-allele pairs) run four to a wave and only wide ones need the whole wave.
// The computed score is exact iff it is <= K; otherwise the task is appended to the overflow list and handled
// by the next tier (larger group / more blocks per lane, finally the wavefront kernel).
// Pattern match masks (A, C, G, T + at most one further byte value occurring in the pattern, e.g. N) are derived from two bit-planes per
// 64-row block (myers_masks.hpp) when a lane moves to its next superblock.  The pipeline's patterns are whole reads, each compared with
// every other read of its region: their planes come from a table built once per run (read_masks_kernel; a task's first table block in the
// side array `pblk`; the reversed copies of the reassignment pass have theirs in a second region of the table, written as they are copied).
// Every other pair — the operator-level calls, reads with a byte outside A C G T —
// has them built by its wave into an L2-resident scratch before the sweep: per block one coalesced 64-byte load and one compare per symbol.
// The text of a task with table blocks is read as row codes, one per arena byte, written with the table (`codes`); every other task
// translates its text bytes through an LDS byte map.
// Richer alphabets, text-side free ends and patterns > 16384 bytes go to the wavefront kernel.
// The column step of a block (myers_step.hpp) works on 32-bit halves with three-input bit operations: what a vector instruction costs on
// gfx950 depends on its class, and the tiers are bound by vector issue.
#include "otg_common.hpp"
#include "myers_step.hpp"
#include "myers_masks.hpp"
#include <algorithm>
#include <cstdlib>

namespace {

constexpr int MAXBLK = 256;           // 64-row blocks per pattern (m <= 16384)
using u64 = unsigned long long;

__device__ __forceinline__ u64 load8(const uint8_t* p) { u64 v; __builtin_memcpy(&v, p, 8); return v; }

// lane i <- lane i-1 within its group of GL lanes (wrap-around)
template <int GL>
__device__ __forceinline__ int group_ror1(int x, int lane)
{
  if (GL == 64) return __builtin_amdgcn_update_dpp(x, x, 0x13C, 0xf, 0xf, false);   // wave_ror:1
  if (GL == 16) return __builtin_amdgcn_update_dpp(x, x, 0x121, 0xf, 0xf, false);   // row_ror:1
  const int src = (lane & ~(GL - 1)) | ((lane - 1) & (GL - 1));
  return __builtin_amdgcn_ds_bpermute(src << 2, x);
}

// W_p of SURVEY.md §8d for a finished alignment with score s (what the wavefront aligner would have evaluated):
// per score t the diagonals [max(-pbf - t, -m), min(tbf + t, n)]; the lanes of the group stride over t.
template <int GL>
__device__ u64 wfa_cells(int s, int m, int n, int pbf, int tbf, int gl)
{
  u64 w = 0;
  for (int t = gl; t <= s; t += GL) {
    const int lo = -pbf - t < -m ? -m : -pbf - t;
    const int hi = tbf + t > n ? n : tbf + t;
    w += (u64)(hi - lo + 1);
  }
  for (int off = GL / 2; off > 0; off >>= 1) w += __shfl_xor(w, off, GL);
  return w;
}

// (<1,8> sits at the edge of six waves per SIMD, 80 vector registers; the bound keeps it there: no spill, private segment 0)
template <int BPL, int GL, int WPB>
__global__ __launch_bounds__(WPB * 64, (BPL == 1 && GL == 8) ? 6 : 1) void myers_edit_kernel(
    const uint8_t* __restrict__ arena, const otg_align_task* __restrict__ tasks,
    const uint32_t* __restrict__ todo, const uint32_t* __restrict__ n_todo_ptr, uint32_t n_todo_imm,
    int32_t* __restrict__ scores, uint64_t* __restrict__ cells,
    uint32_t* __restrict__ ticket, uint32_t* __restrict__ n_overflow, uint32_t* __restrict__ overflow_list,
    otg_myers::MaskBlock* __restrict__ peq_ws, int maxblk,
    const uint32_t* __restrict__ pblk, const otg_myers::PlaneBlock* __restrict__ tab, const uint8_t* __restrict__ codes)
{
  constexpr int G = 64 / GL;            // pairs per wave
  // The text of a table task comes as row codes (one per arena byte, read_masks_kernel) instead of bytes.  The two whole-wave tiers stay on
  // the byte map: they carry 0.1 ms of a step and take scalar spills with both paths in one kernel.
  constexpr bool CODES = GL < 64;
  constexpr int SB = 64 * BPL;
  constexpr int NT = WPB * 64;
  // Match-mask table of the lane's CURRENT superblock: row (sym * BPL + q), column = thread; a lane only ever reads
  // its own column (same-wave program order, no barrier) and the row stride is a multiple of the bank count, so the
  // per-step fetch `row(symbol of this column)` is one conflict-free ds_read_b64 instead of a select tree.
  // sym: 0..3 = A C T G (code (byte >> 1) & 3), 4 = the one extra byte value of the pattern, 5 = anything else (zero).
  __shared__ u64 s_eq[6 * BPL][NT];
  // byte -> row index (sym * BPL) * 8 per lane group; text bytes are translated when a lane loads its next 8 columns.  The entry sits
  // in bits 8..15 of a 16-bit field of the translated text, where it IS the byte offset of the row in s_eq (row * NT * 8 = row * 8 << 8).
  static_assert(NT * sizeof(u64) == (8u << 8) && 5 * BPL * 8 < 256, "a row's byte offset must be its 8-bit map entry shifted by 8");
  __shared__ uint8_t s_lut[WPB * G][256];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int gl = lane & (GL - 1);       // lane within its group
  const int grp = lane / GL;
  otg_myers::MaskBlock* const peq_wave = peq_ws + (size_t)(blockIdx.x * WPB + wib) * G * (size_t)maxblk;
  const otg_myers::MaskBlock* const peq = peq_wave + (size_t)grp * (size_t)maxblk;
  const uint32_t n_todo = n_todo_ptr ? *n_todo_ptr : n_todo_imm;
  using lds_u64 = __attribute__((address_space(3))) u64;
  using lds_u8 = __attribute__((address_space(3))) uint8_t;
  volatile lds_u64* EQ = (volatile lds_u64*)&s_eq[0][0] + threadIdx.x;          // this thread's column; row r at EQ[r * NT]
  volatile lds_u8* LUT = (volatile lds_u8*)&s_lut[wib * G + grp][0];
  const uint32_t eq_addr = (uint32_t)(uintptr_t)(lds_u64*)&s_eq[0][0] + threadIdx.x * (uint32_t)sizeof(u64);     // LDS byte address of this thread's column
  {
    // static part of the tables: zero rows, ACGT entries of the byte map (the extra symbol is patched per pair)
#pragma unroll
    for (int q = 0; q < BPL; ++q) EQ[(5 * BPL + q) * NT] = 0ull;
    for (int c = gl; c < 256; c += GL) {
      LUT[c] = (uint8_t)(otg_myers::text_row_code((uint32_t)c) * BPL);
    }
  }
  int lut_other = -1;                    // byte currently mapped to row 4 in this group's map

  for (;;) {
    const uint32_t tk0 = otg_wave_atomic_add(ticket, (uint32_t)G);
    if (tk0 >= n_todo) break;
    const uint32_t tk = tk0 + (uint32_t)grp;
    const bool has_task = tk < n_todo;
    const uint32_t ti = has_task ? (todo ? todo[tk] : tk) : (todo ? todo[tk0] : tk0);
    const otg_align_task tsk = tasks[ti];
    const bool ef = tsk.endsfree != 0;
    const uint8_t* P = arena + tsk.pattern_off;
    const uint8_t* T = arena + tsk.text_off;
    int m = (int)tsk.pattern_len, n = (int)tsk.text_len;
    int pbf = ef ? tsk.pattern_begin_free : 0, pef = ef ? tsk.pattern_end_free : 0;
    bool unsupported = ef && (tsk.text_begin_free != 0 || tsk.text_end_free != 0);
    const bool swapped = !ef && m < n;
    if (swapped) { const uint8_t* q = P; P = T; T = q; const int x = m; m = n; n = x; }   // edit distance is symmetric
    if (m < n) unsupported = true;
    if (pbf > m) pbf = m;
    if (pef > m) pef = m;
    const int d = m - n;
    const int nblk = (m + 63) >> 6;
    const int nsb = (m + SB - 1) / SB;
    // Ukkonen band for the largest threshold K this lane schedule (R rows) can certify, see otg_myers_band
    // R: a lane must have left superblock B (last step SB*B + SB-1 + KL + B) before B + GL enters the band
    // (first step SB*(B+GL) - KU + B + GL)  <=>  KL + KU <= SB*(GL-1) + GL
    constexpr int R = (GL - 1) * SB + GL;
    const int K = otg_myers_threshold(R, d, pbf, pef);
    int KL, KU;
    otg_myers_band(K, d, pbf, pef, &KL, &KU);
    if (nblk > maxblk || K < d - pbf - pef || K < 1 || KL + KU > R || n < 1 || pbf > d || pef > d) unsupported = true;
    if (!has_task) unsupported = true;

    // ---- pattern planes per 64-row block: from the table when the task names its blocks there, otherwise built here by the whole wave,
    // one pair after the other: lane r of the wave holds row r of the block, a compare against a symbol is the block's mask of that symbol
    const uint32_t tblk = (pblk && tab && !unsupported && !swapped) ? pblk[ti] : otg_myers::NO_MASKS;
    const bool use_tab = tblk != otg_myers::NO_MASKS;
    // a table pattern has no extra symbol, so the row of a text byte is the same for every pair: read it from the code buffer
    const bool use_codes = CODES && codes != nullptr && use_tab;
    if (use_codes) T = codes + (T - arena);
    int other = -1;
    {
      const bool build = !unsupported && !use_tab;
      bool bad_alpha = false;
      if (__ballot(build)) {
        const u64 p_off = (u64)(P - arena);
        for (int g = 0; g < G; ++g) {
          const int src = g * GL;
          if (!__builtin_amdgcn_readlane((int)build, src)) continue;
          const u64 og = (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p_off, src) | (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(p_off >> 32), src) << 32;
          const int mg = __builtin_amdgcn_readlane(m, src);
          const int nb = (mg + 63) >> 6;
          otg_myers::MaskBlock* const pq = peq_wave + (size_t)g * (size_t)maxblk;
          int oth = -1;
          bool bad = false;
          for (int b4 = 0; b4 < nb; b4 += 4) {
            uint32_t ch[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int i = ((b4 + k) << 6) + lane; ch[k] = i < mg ? (uint32_t)arena[og + (u64)i] : 0u; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              if (b4 + k >= nb) break;
              const u64 rows = otg_myers::block_rows(mg, b4 + k);
              const uint32_t c = ch[k];
              const otg_myers::MaskBlock mk = otg_myers::block_masks([&](uint8_t v) { return __ballot(c == (uint32_t)v) & rows; },
                                                                     [&](int r) { return (uint32_t)__builtin_amdgcn_readlane((int)c, r); }, rows, &oth, &bad);
              if (lane == 0) pq[b4 + k] = mk;
            }
          }
          if (grp == g) { other = oth; bad_alpha = bad; }
        }
      }
      if (bad_alpha) unsupported = true;       // a second byte value outside A C G T: the wavefront kernel's
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (other != lut_other) {            // group-uniform
      if (gl == 0) {
        if (lut_other >= 0) LUT[lut_other] = (uint8_t)(5 * BPL * 8);
        if (other >= 0) LUT[other] = (uint8_t)(4 * BPL * 8);
      }
      lut_other = other;
    }

    // ---- skewed sweep
    int B = gl;                         // current superblock of this lane
    if (!unsupported) while (B < nsb && SB * B + SB - 1 + KL < 0) B += GL;      // (KL < 0: the band starts below diagonal 0, the superblocks above it never enter it)
    bool inited = false;
    uint32_t PvL[BPL], PvH[BPL], MvL[BPL], MvH[BPL];     // vertical deltas of the lane's blocks, as 32-bit halves (myers_step.hpp)
#pragma unroll
    for (int q = 0; q < BPL; ++q) { PvL[q] = PvH[q] = ~0u; MvL[q] = MvH[q] = 0; }
    int score = 0, hout = 0;
    int best = 0x3fffffff;
    const int i_lo = m - pef;           // the answer is min over rows i in [i_lo, m] of D[i][n]
    if (i_lo <= 0) best = n;            // D[0][n] = n
    const int t_end = unsupported ? -1 : n - 1 + nsb - 1;
    // per-superblock time window (recomputed only when the lane moves to its next superblock)
    // with u = t - t_start: in the band <=> (uint32_t)u < t_len, one unsigned compare; past it <=> u >= t_len as signed numbers
    // (no window: t_len = 0 and t_start = INT_MAX, so u stays negative).  ends_sweep: the window's last column is the text's last one.
    int t_start, t_len, t_hin_stop; bool ends_sweep, exact_init;
    auto setup = [&]() {
      int jlo = SB * B - KU; if (jlo < 0) jlo = 0;
      int jhi = SB * B + SB - 1 + KL; if (jhi > n - 1) jhi = n - 1;
      exact_init = (jlo == 0);
      if (!unsupported && B < nsb && jlo <= jhi) {
        t_start = jlo + B; t_len = jhi - jlo + 1;
        int jh = SB * B - 1 + KL; if (jh > jhi) jh = jhi;
        t_hin_stop = B > 0 ? jh + B : -1;              // block above still inside the band
        ends_sweep = (jhi == n - 1);
      } else { t_start = 0x7fffffff; t_len = 0; t_hin_stop = -1; ends_sweep = false; }
    };
    setup();
    // text bytes: one unaligned 8-byte load per 8 steps and lane (prefetched 4 steps ahead); byte (t & 7) of it
    // is column (t & ~7) - B + (t & 7) = t - B
    struct Txt { uint32_t w[4]; };                      // 8 row offsets: step 2i in bits 0..15 of w[i], step 2i + 1 in bits 16..31
    auto load_group = [&](int tg) -> Txt {              // tg = first step of the group
      int a = tg - B;
      if (a > n - 1) a = n - 1;
      u64 x;
      if (a >= 0) x = load8(T + a);
      else { const int sh = -a; x = sh < 8 ? (load8(T) << (8 * sh)) : 0ull; }
      Txt c;
      if (use_codes) {
        // x holds 8 codes (8 x row index, at most 40): times BPL a byte is the map entry of the other path, with no carry between bytes
        const uint32_t lo = (uint32_t)x * (uint32_t)BPL, hi = (uint32_t)(x >> 32) * (uint32_t)BPL;
        c.w[0] = __builtin_amdgcn_perm(lo, lo, 0x010c000cu); c.w[1] = __builtin_amdgcn_perm(lo, lo, 0x030c020cu);     // (byte 2i << 8) | (byte 2i+1 << 24)
        c.w[2] = __builtin_amdgcn_perm(hi, hi, 0x010c000cu); c.w[3] = __builtin_amdgcn_perm(hi, hi, 0x030c020cu);
        return c;
      }
      uint32_t r[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = LUT[(uint32_t)(x >> (8 * i)) & 0xffu];
#pragma unroll
      for (int i = 0; i < 4; ++i) c.w[i] = __builtin_amdgcn_perm(r[2 * i + 1], r[2 * i], 0x040c000cu);       // (r[2i] << 8) | (r[2i+1] << 24)
      return c;
    };
    Txt c8 = load_group(0), c8n = {{0, 0, 0, 0}};
    // D[i][n] of the rows of the lane's superblock that may end the alignment; called once the window's last column is done, if ends_sweep:
    // where the lane leaves the superblock, or after the sweep
    auto harvest = [&]() {
      const int row_top = SB * B;                     // rows row_top+1 .. row_top+SB
      if (row_top + SB >= i_lo && row_top < m) {
        int sc = score;
#pragma unroll
        for (int q = BPL - 1; q >= 0; --q) {
          const u64 pv = (u64)PvH[q] << 32 | PvL[q], mv = (u64)MvH[q] << 32 | MvL[q];
#pragma unroll 1
          for (int r = 63; r >= 0; --r) {
            const int i = row_top + 64 * q + r + 1;
            if (i <= m && i >= i_lo && i >= 1 && sc < best) best = sc;
            sc -= (int)((pv >> r) & 1ull) - (int)((mv >> r) & 1ull);
          }
        }
      }
    };
    // the wave runs until its longest pair is done
    int t_end_w = t_end;
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(t_end_w, off); t_end_w = o > t_end_w ? o : t_end_w; }
    t_end_w = __builtin_amdgcn_readfirstlane(t_end_w);
    // one column per step; unrolled by the 8 columns of a translated text group so that every byte position is static
    auto step = [&](const int t, const int ph) {
      // values of lane-1 (within the group) after its previous step
      const int up_score = group_ror1<GL>(score, lane);
      const int up_hout = group_ror1<GL>(hout, lane);
      bool switched = false;
      if (t - t_start >= t_len) {       // this superblock left the band: move to the next one owned by the lane
        if (ends_sweep) harvest();
        B += GL; inited = false; setup();
        c8 = load_group(t - ph);
        if (ph >= 4) c8n = load_group(t - ph + 8);
        switched = true;
      }
      if (ph == 4) c8n = load_group(t + 4);
      else if (ph == 0 && t > 0 && !switched) c8 = c8n;     // (after a switch c8 is already this group's text; c8n still belongs to the old superblock)
      if ((uint32_t)(t - t_start) < (uint32_t)t_len) {
        if (!inited) {
#pragma unroll
          for (int q = 0; q < BPL; ++q) {
            const int b = B * BPL + q;
            otg_myers::MaskBlock mk = {0ull, 0ull, 0ull, 0ull};
            if (b < nblk) {
              if (tblk != otg_myers::NO_MASKS) { const otg_myers::PlaneBlock pb = tab[tblk + (uint32_t)b]; mk.b0 = pb.b0; mk.b1 = pb.b1; mk.ok = otg_myers::block_rows(m, b); }
              else mk = peq[b];
            }
            uint64_t rows5[5];                            // A C T G X, the order of the code
            otg_myers::rows_from_planes(mk.b0, mk.b1, mk.ok, mk.ex, rows5);
#pragma unroll
            for (int y = 0; y < 5; ++y) EQ[(y * BPL + q) * NT] = rows5[y];
            MvL[q] = MvH[q] = 0;
            u64 pv0 = ~0ull;
            if (exact_init) {
              // true first column: D[i][0] = max(0, i - pbf)  ->  vertical delta +1 for rows i > pbf
              const int r0 = b << 6;                       // row i = r0 + bit + 1
              const int z = pbf - r0;                      // bits [0, z) are 0
              pv0 = z <= 0 ? ~0ull : (z >= 64 ? 0ull : (~0ull << z));
            }
            PvL[q] = (uint32_t)pv0; PvH[q] = (uint32_t)(pv0 >> 32);
          }
          if (exact_init) { const int rows = SB * (B + 1); score = rows > pbf ? rows - pbf : 0; }
          else score = (up_score - up_hout) + SB;
          inited = true;
        }
        // LDS address of the mask row of this column's text byte, in this thread's column
        const uint32_t rowa = ((ph & 1) ? c8.w[ph >> 1] >> 16 : c8.w[ph >> 1] & 0xff00u) + eq_addr;
        int hin = t <= t_hin_stop ? up_hout : 1;
#pragma unroll
        for (int q = 0; q < BPL; ++q) {
          const u64 Eq = *(volatile lds_u64*)(uintptr_t)(rowa + (uint32_t)(q * NT * sizeof(u64)));
          hin = otg_myers::block_step(PvL[q], PvH[q], MvL[q], MvH[q], (uint32_t)Eq, (uint32_t)(Eq >> 32), hin);
        }
        hout = hin;
        score += hout;
      }
    };
    for (int t8 = 0; t8 <= t_end_w; t8 += 8) {
      step(t8 + 0, 0); step(t8 + 1, 1); step(t8 + 2, 2); step(t8 + 3, 3);
      step(t8 + 4, 4); step(t8 + 5, 5); step(t8 + 6, 6); step(t8 + 7, 7);
    }
    if (ends_sweep) harvest();          // the lane's last superblock ended with the sweep
    for (int off = GL / 2; off > 0; off >>= 1) { const int o = __shfl_xor(best, off, GL); best = o < best ? o : best; }
    const bool ok = !unsupported && best <= K;
    u64 w = 0;
    // a mirrored task (_pad bit 0: both sequences reversed by the pipeline) reports the cells of the un-reversed alignment: its free
    // prefixes are this task's free suffixes
    const bool mirrored = (tsk._pad & 1) != 0;
    if (cells) w = wfa_cells<GL>(ok ? best : -1, (int)tsk.pattern_len, (int)tsk.text_len, ef ? (mirrored ? tsk.pattern_end_free : tsk.pattern_begin_free) : 0,
                                 ef ? (mirrored ? tsk.text_end_free : tsk.text_begin_free) : 0, gl);
    if (has_task && gl == 0) {
      if (ok) { scores[ti] = best; if (cells) cells[ti] = w; }
      else if (overflow_list) { const uint32_t q = atomicAdd(n_overflow, 1u); overflow_list[q] = ti; }
      else scores[ti] = -1;
    }
  }
}

// The per-read table: one wave per read, lane r holds row r of a block.  Block b of read i (64 bases from its CURRENT seq_off: realignment has
// moved it by now) lands at tab[first_blk[i] + b]; first_blk was laid out from the submitted lengths, which realignment only shortens.  A read
// with a byte outside A C G T, and a read outside every region (its range was never checked against the arena), gets NO_MASKS in read_blk:
// its pairs build their masks themselves.  The read's row codes go to codes + seq_off (nullable).
__global__ __launch_bounds__(256) void read_masks_kernel(const uint8_t* __restrict__ arena, const otg_read* __restrict__ reads, const uint32_t* __restrict__ read_region,
                                                         uint32_t n_reads, const uint32_t* __restrict__ first_blk, otg_myers::PlaneBlock* __restrict__ tab,
                                                         uint32_t* __restrict__ read_blk, uint8_t* __restrict__ codes)
{
  const int lane = threadIdx.x & 63;
  const uint32_t nw = gridDim.x * (blockDim.x >> 6);
  for (uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_reads; i += nw) {
    if (read_region[i] == 0xffffffffu) { if (lane == 0) read_blk[i] = otg_myers::NO_MASKS; continue; }
    const uint8_t* const S = arena + reads[i].seq_off;
    const int m = (int)reads[i].seq_len;
    if (codes) otg_myers::wave_read_codes<false>(S, m, lane, nullptr, codes + reads[i].seq_off);
    const bool flagged = otg_myers::wave_read_planes([&](int j) { return S[j]; }, m, lane, tab + first_blk[i]);
    if (lane == 0) read_blk[i] = flagged ? otg_myers::NO_MASKS : first_blk[i];
  }
}

template <int BPL, int GL>
int launch_one(otg_ctx* ctx, const uint8_t* d_arena, const otg_align_task* d_tasks, const uint32_t* d_todo,
               const uint32_t* d_n_todo, uint32_t n_tasks, int32_t* d_scores, uint64_t* d_cells,
               uint32_t* ticket, uint32_t* n_overflow, uint32_t* overflow_list, const uint32_t* d_pblk, const otg_myers::PlaneBlock* d_masks, const uint8_t* d_codes)
{
  constexpr int WPB = 4, G = 64 / GL;
  int maxblk = (int)((ctx->max_seq_len + 63) / 64) + 1;
  if (maxblk > MAXBLK) maxblk = MAXBLK;
  uint32_t want = (n_tasks + WPB * G - 1) / (WPB * G);
  // persistent blocks: exactly as many as are resident at once (VGPR / LDS limits differ per instantiation)
  static int per_cu = 0;
  if (per_cu == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, myers_edit_kernel<BPL, GL, WPB>, WPB * 64, 0) != hipSuccess || nb < 1) nb = 4;
    per_cu = nb > 8 ? 8 : nb;
  }
  const uint32_t grid_max = (uint32_t)ctx->n_cu * 8;      // sizes the scratch (upper bound of per_cu)
  const uint32_t grid_res = (uint32_t)ctx->n_cu * (uint32_t)per_cu;
  uint32_t grid = grid_res < want ? grid_res : want;
  if (grid == 0) return OTG_OK;
  otg_myers::MaskBlock* ws = (otg_myers::MaskBlock*)otg_slot(ctx, SLOT_AUX8, (size_t)grid_max * WPB * 8 * (size_t)MAXBLK * sizeof(otg_myers::MaskBlock));   // up to 8 pairs per wave
  if (!ws) return OTG_ERR_HIP;
  hipLaunchKernelGGL((myers_edit_kernel<BPL, GL, WPB>), dim3(grid), dim3(WPB * 64), 0, ctx->stream, d_arena, d_tasks, d_todo, d_n_todo, n_tasks,
                     d_scores, d_cells, ticket, n_overflow, overflow_list, ws, maxblk, d_pblk, d_masks, d_codes);
  return OTG_OK;
}

} // namespace

// One tier of the bit-parallel engine: tasks from (d_todo, d_n_todo) (or all n_tasks when d_todo is null);
// tasks it cannot finish exactly are appended to overflow_list / n_overflow.
// tier (OTG_MYERS_TIERS of them): 0 = 8-lane groups x 1 block per lane (8 pairs / wave); then 8 / 16 / 32 / 64-lane groups x 2 blocks per lane
//       (two blocks share the per-column overhead of a lane: ~14 % fewer SIMD cycles per row than one block per lane), with a three-block step
//       between the 8- and 16-lane and between the 16- and 32-lane ones (<3,8> = 1352 rows at 0.7 x the cost of <2,16>, <3,16> = 2896 rows at
//       0.7 x the cost of <2,32>: a pair pays for the band of its tier, not for its own); last = whole wave x 4 blocks per lane.
int otg_launch_myers(otg_ctx* ctx, int tier, const uint8_t* d_arena, const otg_align_task* d_tasks, const uint32_t* d_todo,
                     const uint32_t* d_n_todo, uint32_t n_tasks, int32_t* d_scores, uint64_t* d_cells,
                     uint32_t* ticket, uint32_t* n_overflow, uint32_t* overflow_list, const uint32_t* d_pblk, const otg_myers::PlaneBlock* d_masks, const uint8_t* d_codes)
{
  int rc;
  switch (tier) {
    case 0: rc = launch_one<1, 8>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
    case 1: rc = launch_one<2, 8>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
    case 2: rc = launch_one<3, 8>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
    case 3: rc = launch_one<2, 16>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
    case 4: rc = launch_one<3, 16>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
    case 5: rc = launch_one<2, 32>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
    case 6: rc = launch_one<2, 64>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
    default: rc = launch_one<4, 64>(ctx, d_arena, d_tasks, d_todo, d_n_todo, n_tasks, d_scores, d_cells, ticket, n_overflow, overflow_list, d_pblk, d_masks, d_codes); break;
  }
  if (rc) return rc;
  HIP_TRY(ctx, hipGetLastError());
  return OTG_OK;
}

// The per-read plane table of a resident batch (read_masks_kernel): d_first_blk[i] = first table block of read i, d_read_blk[i] = the same
// or NO_MASKS on return.
int otg_launch_read_masks(otg_ctx* ctx, const uint8_t* d_arena, const otg_read* d_reads, const uint32_t* d_read_region, uint32_t n_reads,
                          const uint32_t* d_first_blk, otg_myers::PlaneBlock* d_masks, uint32_t* d_read_blk, uint8_t* d_codes)
{
  if (n_reads == 0) return OTG_OK;
  const uint32_t grid = std::min<uint32_t>((n_reads + 3) / 4, (uint32_t)ctx->n_cu * 32);
  hipLaunchKernelGGL(read_masks_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_arena, d_reads, d_read_region, n_reads, d_first_blk, d_masks, d_read_blk, d_codes);
  HIP_TRY(ctx, hipGetLastError());
  return OTG_OK;
}

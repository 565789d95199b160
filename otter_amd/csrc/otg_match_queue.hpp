// otg_match_queue.hpp — the match-run queue of the wavefront kernels' extend step and its drain ("The extend step").
//
// A sweep probes 8 bytes (32 packed bases) per diagonal; a diagonal whose probe matched in full is pushed to a wave-compacted queue in LDS,
// and the drain extends the queued runs pass by pass, so that no lane waits for the slowest diagonal of its chunk.  Used by wfa_edit.hip,
// wfa_affine.hip and wfa_adaptive.hip; wfa_affine_reg.hip keeps its own (its entries carry the offset and it writes a patch table).
#pragma once
#include "otg_common.hpp"

namespace otg_mq {

struct Seqs { const uint8_t* P; const uint8_t* T; int pl, tl; };      // the pair: pattern, text and their lengths
struct Probe { int m, full; };                                        // bases matched, and the count that means "the whole probe matched"

// Appends `entry` of every lane in `mm` (the ballot of `more`) behind the queue's first qn entries, in lane order.  Wave-uniform control flow.
template <class Q>
__device__ __forceinline__ void push(Q* queue, int& qn, unsigned long long mm, bool more, int entry)
{
  if (more) {
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
    queue[qn + rank] = entry;
  }
  qn += __builtin_popcountll(mm);
}

// The byte probes of a drain pass: 16 bytes in the first pass (most queued runs end there), 64 from then on.
__device__ __forceinline__ Probe probe_bytes(const Seqs& s, int pass, int v, int h, int rem)
{
  if (pass == 0) return {otg_match16(s.P, s.T, v, h, rem), 16};
  return {otg_match64(s.P, s.T, v, h, rem), 64};
}

// Extends every queued run to its end and leaves the queue empty.  A pass re-reads the queue 64 entries at a time, probes, stores the new
// offsets and re-compacts the runs that outlived the probe in place (the write cursor never passes the read cursor).  WAVE_STEP: once no more
// than four runs are left after the first pass, the whole wave extends them one at a time, 512 bytes per iteration (tandem-repeat reads have
// exact runs of hundreds of bases).  What differs between the kernels comes in as
//   diag(e)           the diagonal k of queue entry e (lo + e, kbase + e: whatever the kernel's pushes stored);
//   load(k), store(k, h)   the offset of diagonal k, wherever the kernel keeps its wavefront;
//   probe(pass, v, h, rem) -> Probe   equal bases from pattern position v / text position h on, at most rem;
//   fence()           at the head of every pass, where another lane than the one that stored an offset reads it through memory (HBM rows);
//   final(h, k) -> bool   diagonal k is fully extended at offset h: called per lane under the lane's own condition in a pass, with wave-uniform
//                     values in the wave-wide step.  The lanes that answered true come back as a lane mask (all lanes for the wave-wide step).
template <bool WAVE_STEP, class Q, class Diag, class Load, class Store, class ProbeFn, class Fence, class Final>
__device__ __forceinline__ unsigned long long drain(Q* queue, int& qn, int lane, const Seqs& s, Diag diag, Load load, Store store, ProbeFn probe,
                                                    Fence fence, Final final)
{
  unsigned long long finm = 0ull;
  int pass = 0;
  while (qn > 0) {
    fence();
    if (WAVE_STEP && qn <= 4 && pass > 0) {
      for (int q = 0; q < qn; ++q) {
        const int k = diag(__builtin_amdgcn_readfirstlane((int)queue[q]));
        int h = __builtin_amdgcn_readfirstlane(load(k));
        const int v = h - k;
        const int rem = s.pl - v < s.tl - h ? s.pl - v : s.tl - h;
        h += otg_wave_match(s.P, s.T, v, h, rem, lane);
        store(k, h);                              // the same value from every lane
        if (final(h, k)) finm = ~0ull;
      }
      qn = 0;
      break;
    }
    int wq = 0;
    for (int q0 = 0; q0 < qn; q0 += 64) {
      const bool act = q0 + lane < qn;
      int e = 0;
      bool more = false, fin = false;
      if (act) {
        e = (int)queue[q0 + lane];
        const int k = diag(e);
        int h = load(k), v = h - k;
        const Probe p = probe(pass, v, h, s.pl - v < s.tl - h ? s.pl - v : s.tl - h);
        v += p.m; h += p.m;
        more = p.m == p.full && v < s.pl && h < s.tl;
        store(k, h);
        if (!more) fin = final(h, k);
      }
      finm |= __ballot(fin);
      push(queue, wq, __ballot(more), more, e);
    }
    qn = wq; ++pass;
  }
  return finm;
}

} // namespace otg_mq

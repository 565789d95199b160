// genotype_edit.hip — the sequence-dissimilarity matrix of `otter genotype` under OTG_GT_METRIC_EDIT: what align_anreads
// (reference: src/analignments.cpp:62-72) computes for two spanning sequences, for every pair of alleles of a region, in the condensed layout
// genotype_kernel (cluster.hip) clusters.  Four steps on the stream, no host round trip between them:
//   1. K_allele_hash     a 64-bit hash per allele, one wave per allele, 16-byte loads;
//      K_allele_classes  cls[a] = the smallest allele of the region with a's bytes: equal hash and length only nominate, a byte compare decides;
//   2. K_allele_pair_tasks  one end-to-end task per pair of class representatives at the pair's own slot, its denominator, the slot on a todo list;
//   3. the exact edit tier chain (otg_launch_edit_todo) on that list, whatever heuristic the context is set to;
//   4. K_allele_dist_epilogue  every pair of the region reads the score of its two classes: 0.0 inside a class, score / max(len) across.
// A cohort repeats few sequences many times, so the alignments go from A (A - 1) / 2 to C(distinct, 2) per region.
#include "otg_common.hpp"
#include "otg_chain.hpp"
#include <algorithm>

namespace {

__device__ __forceinline__ size_t didx(int N, int r, int c) { return (size_t)((((long long)(2 * N - 3 - r)) * r) >> 1) + c - 1; } // r < c

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// counters of one launch (SLOT_GTE_CLS, behind the hashes and classes)
struct GteCounters { uint32_t n_todo, n_trivial, failed, fail_region_inv; };

// one wave per allele; a lane takes 16 consecutive bytes per 1024-byte tile from ONE 16-byte load (the arena ends in 64 bytes of slack; what lies
// past the allele is masked off).  Every 8-byte word is mixed with its position and the words are summed: the order of the sum does not matter.
__global__ __launch_bounds__(256) void K_allele_hash(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                     const uint32_t* __restrict__ seq_len, uint32_t na, uint64_t* __restrict__ hash)
{
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t a = wave; a < na; a += n_waves) {
    const uint8_t* s = arena + seq_off[a];
    const uint32_t n = seq_len[a];
    uint64_t acc = 0;
    for (uint32_t j0 = 16u * lane; j0 < n; j0 += 1024u) {
      uint64_t w[2];
      __builtin_memcpy(w, s + j0, 16);
      const uint32_t rem = n - j0;
      if (rem < 8u) { w[0] &= (1ull << (8 * rem)) - 1ull; w[1] = 0; }
      else if (rem < 16u) w[1] &= (1ull << (8 * (rem - 8u))) - 1ull;
      const uint64_t pos = (uint64_t)(j0 >> 3);
      acc += mix64(w[0] + 0x9e3779b97f4a7c15ull * (pos + 1)) + mix64(w[1] + 0x9e3779b97f4a7c15ull * (pos + 2));
    }
    uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)hi, off) << 32) | (uint32_t)__shfl_xor((int)lo, off);
      acc += o;
      lo = (uint32_t)acc; hi = (uint32_t)(acc >> 32);
    }
    if (lane == 0) hash[a] = mix64(acc ^ (uint64_t)n);
  }
}

// equal bytes?  (same length n; 8 bytes per load, the tail masked: reads at most 7 bytes past the sequences)
__device__ __forceinline__ bool same_bytes(const uint8_t* x, const uint8_t* y, uint32_t n)
{
  uint32_t q = 0;
  for (; q + 8 <= n; q += 8) if (otg_load8(x + q) != otg_load8(y + q)) return false;
  if (q < n) {
    const uint64_t m = (1ull << (8 * (n - q))) - 1ull;
    if ((otg_load8(x + q) ^ otg_load8(y + q)) & m) return false;
  }
  return true;
}

// one block per region, one thread per allele: the first earlier allele with the same hash, length AND bytes (region-local index); itself if none
__global__ __launch_bounds__(256) void K_allele_classes(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ seq_off,
                                                        const uint32_t* __restrict__ seq_len, const uint32_t* __restrict__ first_allele,
                                                        const uint32_t* __restrict__ n_alleles, uint32_t n_regions,
                                                        const uint64_t* __restrict__ hash, uint32_t* __restrict__ cls)
{
  for (uint32_t r = blockIdx.x; r < n_regions; r += gridDim.x) {
    const uint32_t A = n_alleles[r], f = first_allele[r];
    for (uint32_t a = threadIdx.x; a < A; a += blockDim.x) {
      const uint64_t h = hash[f + a];
      const uint32_t n = seq_len[f + a];
      const uint8_t* s = arena + seq_off[f + a];
      uint32_t c = a;
      for (uint32_t b = 0; b < a; ++b) {
        if (hash[f + b] != h || seq_len[f + b] != n) continue;
        if (same_bytes(arena + seq_off[f + b], s, n)) { c = b; break; }
      }
      cls[f + a] = c;
    }
  }
}

// one block per region: the pairs i < j of class representatives.  The pattern is the longer sequence, allele i on equal length
// (align_anreads, src/analignments.cpp:62-72).  An empty sequence against L bases costs L: scored here, not aligned.
__global__ __launch_bounds__(256) void K_allele_pair_tasks(const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ seq_len,
                                                           const uint32_t* __restrict__ first_allele, const uint32_t* __restrict__ n_alleles,
                                                           uint32_t n_regions, const uint64_t* __restrict__ pair_off, const uint32_t* __restrict__ cls,
                                                           otg_align_task* __restrict__ tasks, uint32_t* __restrict__ den, int32_t* __restrict__ scores,
                                                           uint32_t* __restrict__ todo, GteCounters* __restrict__ cnt)
{
  for (uint32_t r = blockIdx.x; r < n_regions; r += gridDim.x) {
    const int A = (int)n_alleles[r];
    if (A < 2) continue;
    const uint32_t f = first_allele[r];
    const uint64_t base = pair_off[r];
    for (int i = 0; i < A - 1; ++i) {
      if (cls[f + i] != (uint32_t)i) continue;
      const uint32_t li = seq_len[f + i];
      const uint64_t oi = seq_off[f + i];
      for (int j = i + 1 + (int)threadIdx.x; j < A; j += (int)blockDim.x) {
        if (cls[f + j] != (uint32_t)j) continue;
        const uint32_t lj = seq_len[f + j];
        const uint64_t oj = seq_off[f + j];
        const uint64_t slot = base + didx(A, i, j);
        const bool ip = li >= lj;
        otg_align_task t;
        t.pattern_off = ip ? oi : oj; t.text_off = ip ? oj : oi;
        t.pattern_len = ip ? li : lj; t.text_len = ip ? lj : li;
        t.pattern_begin_free = t.pattern_end_free = t.text_begin_free = t.text_end_free = 0;
        t.endsfree = 0; t._pad = 0;
        tasks[slot] = t;
        den[slot] = t.pattern_len;
        if (t.text_len == 0) { scores[slot] = (int32_t)t.pattern_len; atomicAdd(&cnt->n_trivial, 1u); }
        else todo[atomicAdd(&cnt->n_todo, 1u)] = (uint32_t)slot;
      }
    }
  }
}

// one block per region: every pair takes the distance of its two classes (the same bytes, the same lengths, an exact distance: which member
// of a class was aligned does not matter).  A negative score — the chain gave up — flags the call.
__global__ __launch_bounds__(256) void K_allele_dist_epilogue(const uint32_t* __restrict__ first_allele, const uint32_t* __restrict__ n_alleles,
                                                              uint32_t n_regions, const uint64_t* __restrict__ pair_off, const uint32_t* __restrict__ cls,
                                                              const int32_t* __restrict__ scores, const uint32_t* __restrict__ den,
                                                              double* __restrict__ de, GteCounters* __restrict__ cnt)
{
  for (uint32_t r = blockIdx.x; r < n_regions; r += gridDim.x) {
    const int A = (int)n_alleles[r];
    if (A < 2) continue;
    const uint32_t f = first_allele[r];
    const uint64_t base = pair_off[r];
    for (int i = 0; i < A - 1; ++i) {
      const int ci = (int)cls[f + i];
      for (int j = i + 1 + (int)threadIdx.x; j < A; j += (int)blockDim.x) {
        const int cj = (int)cls[f + j];
        double d = 0.0;
        if (ci != cj) {
          const uint64_t slot = base + (ci < cj ? didx(A, ci, cj) : didx(A, cj, ci));
          const int32_t s = scores[slot];
          if (s < 0) { cnt->failed = 1u; atomicMax(&cnt->fail_region_inv, 0xffffffffu - r); }
          d = s / (double)den[slot];
        }
        de[base + didx(A, i, j)] = d;
      }
    }
  }
}

__global__ __launch_bounds__(256) void K_max_u32(const uint32_t* __restrict__ v, uint64_t n, uint32_t* __restrict__ out)
{
  uint32_t m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) m = v[i] > m ? v[i] : m;
  m = (uint32_t)otg_wave_max_i32((int)(m & 0x7fffffffu));        // lengths stay below 2^31
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

} // namespace

int otg_genotype_metric_fits(otg_ctx* ctx, const char* who, int metric, uint64_t n_pairs)
{
  if (metric != OTG_GT_METRIC_LENGTH && metric != OTG_GT_METRIC_EDIT)
    return otg_fail(ctx, OTG_ERR_ARG, "%s: unknown genotype metric %d (OTG_GT_METRIC_LENGTH = 0, OTG_GT_METRIC_EDIT = 1)", who, metric);
  if (metric == OTG_GT_METRIC_EDIT && n_pairs >= ((uint64_t)1 << 32))
    return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: batch too large: split it (pair slots %llu)", who, (unsigned long long)n_pairs);
  return OTG_OK;
}

int otg_device_max_u32(otg_ctx* ctx, const uint32_t* d_v, uint64_t n, uint32_t* out)
{
  *out = 0;
  if (n == 0) return OTG_OK;
  uint32_t* d_m = (uint32_t*)otg_slot(ctx, SLOT_GTE_CLS, 16);
  if (!d_m) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemsetAsync(d_m, 0, 4, ctx->stream));
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 4);
  hipLaunchKernelGGL(K_max_u32, dim3(grid), dim3(256), 0, ctx->stream, d_v, n, d_m);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(out, d_m, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OTG_OK;
}

// Enqueues steps 1-4 on the context's stream; the matrix lands in SLOT_P20, where otg_launch_genotype reads it.  n_pairs < 2^32
// (otg_genotype_metric_fits); max_len = the longest allele.  What the launch left for the host (alignments run, the failure flag) is read by
// otg_genotype_metric_finish once the stream has been waited for.
int otg_launch_genotype_edit_matrix(otg_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_first,
                                    const uint32_t* d_n, uint32_t n_regions, const uint64_t* d_poff, uint64_t n_pairs, uint64_t na, uint32_t max_len)
{
  ctx->gt_edit_ran = false;
  if (n_regions == 0 || n_pairs == 0) return OTG_OK;
  const size_t cls_bytes = (na + 1) * 8 + (((na + 1) * 4 + 15) & ~(size_t)15);
  char* cb = (char*)otg_slot(ctx, SLOT_GTE_CLS, cls_bytes + sizeof(GteCounters));
  otg_align_task* d_tasks = (otg_align_task*)otg_slot(ctx, SLOT_GTE_TASKS, (size_t)n_pairs * sizeof(otg_align_task));
  int32_t* d_scores = (int32_t*)otg_slot(ctx, SLOT_GTE_SCORES, (size_t)n_pairs * 4);
  uint32_t* d_den = (uint32_t*)otg_slot(ctx, SLOT_GTE_DEN, (size_t)n_pairs * 4);
  uint32_t* d_todo = (uint32_t*)otg_slot(ctx, SLOT_GTE_TODO, (size_t)n_pairs * 4);
  double* d_de = (double*)otg_slot(ctx, SLOT_P20, (n_pairs + 1) * 8);
  if (!cb || !d_tasks || !d_scores || !d_den || !d_todo || !d_de) return OTG_ERR_HIP;
  uint64_t* d_hash = (uint64_t*)cb;
  uint32_t* d_cls = (uint32_t*)(cb + (na + 1) * 8);
  GteCounters* d_cnt = (GteCounters*)(cb + cls_bytes);
  ctx->gt_edit_cnt_off = cls_bytes;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, sizeof(GteCounters), st));
  const uint32_t g_reg = std::min<uint32_t>(n_regions, (uint32_t)ctx->n_cu * 8);
  const uint32_t g_hash = (uint32_t)std::min<uint64_t>((na + 3) / 4, (uint64_t)ctx->n_cu * 16);
  hipLaunchKernelGGL(K_allele_hash, dim3(g_hash), dim3(256), 0, st, d_arena, d_off, d_len, (uint32_t)na, d_hash);
  hipLaunchKernelGGL(K_allele_classes, dim3(g_reg), dim3(256), 0, st, d_arena, d_off, d_len, d_first, d_n, n_regions, (const uint64_t*)d_hash, d_cls);
  hipLaunchKernelGGL(K_allele_pair_tasks, dim3(g_reg), dim3(256), 0, st, d_off, d_len, d_first, d_n, n_regions, d_poff, (const uint32_t*)d_cls,
                     d_tasks, d_den, d_scores, d_todo, d_cnt);
  HIP_TRY(ctx, hipGetLastError());
  // always the exact chain: under wfadaptive a score depends on which sequence is the pattern, so the matrix would not be a function of the
  // two sequences and the classes would not stand for their members
  const int heur = ctx->heur_strategy, kind = ctx->edit_pass_kind;
  const uint32_t batch_max = ctx->max_seq_len;
  ctx->heur_strategy = OTG_HEURISTIC_NONE; ctx->edit_pass_kind = 0; ctx->max_seq_len = std::max<uint32_t>(max_len, 1);
  const int rc = otg_launch_edit_todo(ctx, d_arena, d_tasks, d_todo, &d_cnt->n_todo, (uint32_t)n_pairs, d_scores, nullptr, nullptr, nullptr, nullptr, nullptr);
  ctx->heur_strategy = heur; ctx->edit_pass_kind = kind; ctx->max_seq_len = batch_max;
  if (rc) return rc;
  hipLaunchKernelGGL(K_allele_dist_epilogue, dim3(g_reg), dim3(256), 0, st, d_first, d_n, n_regions, d_poff, (const uint32_t*)d_cls,
                     (const int32_t*)d_scores, (const uint32_t*)d_den, d_de, d_cnt);
  HIP_TRY(ctx, hipGetLastError());
  ctx->gt_edit_ran = true;
  return OTG_OK;
}

// After the stream has been waited for: the times of the two parts (ev0 .. ev2 .. ev1, as otg_genotype_resident recorded them), the number of
// alignments, and the failure of the call when the chain gave a pair up.
int otg_genotype_metric_finish(otg_ctx* ctx, int metric, uint64_t* n_aligned)
{
  if (n_aligned) *n_aligned = 0;
  float all = 0, align = 0;
  HIP_TRY(ctx, hipEventElapsedTime(&all, ctx->ev0, ctx->ev1));
  if (metric == OTG_GT_METRIC_EDIT) HIP_TRY(ctx, hipEventElapsedTime(&align, ctx->ev0, ctx->ev2));
  ctx->last_kernel_ms = all;
  ctx->last_gt_align_ms = align; ctx->last_gt_cluster_ms = (double)all - (double)align;
  if (metric != OTG_GT_METRIC_EDIT || !ctx->gt_edit_ran) return OTG_OK;
  const DevBuf& b = ctx->pool[SLOT_GTE_CLS];
  GteCounters h;
  HIP_TRY(ctx, hipMemcpy(&h, (const char*)b.p + ctx->gt_edit_cnt_off, sizeof(h), hipMemcpyDeviceToHost));
  if (n_aligned) *n_aligned = (uint64_t)h.n_todo + h.n_trivial;
  if (h.failed)
    return otg_fail(ctx, OTG_ERR_CAPACITY, "region %u: an allele pair is beyond the capacity of the edit aligner", 0xffffffffu - h.fail_region_inv);
  return OTG_OK;
}

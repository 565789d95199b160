// unitset.hip — unit sets from the alleles (otg_unitset_repeats, otg_unitset_locus): the repeat units of a region, discovered from the repeat
// structure of its alleles and handed to the locus mode without the alleles leaving HBM.  The reference has no counterpart;
// include/otter_gpu.h states the rule.
//
//   us_candidates  one wave per allele, over its repeat segments: the unit's codes into LDS, the smallest rotation by a tournament (rotation
//                  starts strided over the lanes, then a butterfly), the hash of the rotated codes; one candidate per segment, at the
//                  segment's own index, so a group's candidates are one stretch of the list.
//   us_vote        one workgroup per group (one wave for groups of up to US_SMALL_SEGS segments, four above; both kernels are launched over
//                  all groups and a workgroup leaves at once when the group is the other kernel's).  The class table lies in LDS: a slot
//                  is claimed by one compare-and-swap with the candidate's index, a hash match is confirmed on the rotated bases, weight
//                  and segments go by LDS adds, the representative by one 64-bit maximum (otg_unitset_core.hpp).  Then the largest weight,
//                  and sixteen rounds of "the best class not yet ranked" by a tree over the workgroup.
//   us_tasks       the ranked representatives as rows and units of the unit alignment, in place: a repeat segment holds at least two copies
//                  of its unit, so u u is the first 2 p bases of the representative's segment; the pair tasks (c, d), d ranked before c.
//   (otg_unitalign_resident on those lists: its kernels are untouched)
//   us_select_groups  one thread per group: the redundancy flags from the pair records, the selection under the unit and lane budget.
//   us_write       one wave per group: the unit records, offsets and bytes at the scanned positions.
#include "otg_common.hpp"
#include "otg_scan.hpp"
#include "otg_unitset_core.hpp"
#include <algorithm>
#include <cstdlib>

// cohort.hip: do the alleles of the open cohort batch still lie at d_arena (regrouped, clustered, rows built)?
bool otg_cohort_holds_rows(otg_ctx* ctx, const uint8_t* d_arena);

namespace {

using namespace otg_unitset_core;

constexpr uint32_t US_T = 256;

__global__ __launch_bounds__(64) void us_candidates(OtgRows rows, const uint64_t* __restrict__ seg_off, const otg_repeat_seg* __restrict__ segs, uint32_t hash_bits,
                                                   UsCand* __restrict__ cands)
{
  __shared__ uint8_t code_s[OTG_UNITALIGN_MAX_UNIT];
  const uint32_t a = blockIdx.x, lane = threadIdx.x;
  const uint64_t off = rows.off[a];
  const uint32_t L = rows.len[a];
  for (uint64_t k = seg_off[a]; k < seg_off[a + 1]; ++k) {
    const otg_repeat_seg g = segs[k];
    const uint32_t p = g.period;
    if (p == 0u || p > OTG_UNITALIGN_MAX_UNIT || g.begin > L || p > L - g.begin) {       // (the last two never hold for a segment of the parse)
      if (lane == 0u) { UsCand c; c.hash = 0; c.pos = 0; c.p = c.rot = c.length = c.allele = c.begin = c.pad = 0u; cands[k] = c; }
      continue;
    }
    for (uint32_t j = lane; j < p; j += 64u) code_s[j] = (uint8_t)mo_code(rows.arena[off + g.begin + j]);
    __syncthreads();
    uint32_t best = us_rot_lane(code_s, p, lane);
    for (uint32_t d = 1; d < 64u; d <<= 1) best = us_rot_pick(code_s, p, best, (uint32_t)__shfl_xor((int)best, (int)d));
    if (lane == 0u) {
      UsCand c;
      c.hash = us_hash(code_s, p, best, hash_bits);
      c.pos = off + g.begin; c.p = p; c.rot = best; c.length = g.length; c.allele = a; c.begin = g.begin; c.pad = 0u;
      cands[k] = c;
    }
    __syncthreads();
  }
}

struct UsLdsCas {
  __device__ __forceinline__ uint32_t operator()(uint32_t* p, uint32_t expected, uint32_t desired) const { return atomicCAS(p, expected, desired); }
};

struct UsVoteIn {
  OtgRows rows; const uint64_t* seg_off; const uint32_t* group_first; const UsCand* cands; otg_unitset_params q;
};

template <uint32_t NS, uint32_t T, bool SMALL>
__global__ __launch_bounds__(T) void us_vote(UsVoteIn in, otg_unitset* __restrict__ sets, UsEntry* __restrict__ entries, uint32_t* __restrict__ rank_p)
{
  __shared__ unsigned long long weight_s[NS], rep_s[NS], top_s, total_s;
  __shared__ uint32_t slot_s[NS], segs_s[NS], taken_s[(NS + 31u) / 32u], red_s[T], rank_s[OTG_UNITSET_TOP], ncls_s, over_s;
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const uint32_t a0 = in.group_first[g], a1 = in.group_first[g + 1];
  const uint64_t s0 = in.seg_off[a0], cnt64 = in.seg_off[a1] - s0;
  if (SMALL ? cnt64 > US_SMALL_SEGS : cnt64 <= US_SMALL_SEGS) return;              // the other kernel's group
  const bool huge = cnt64 > 0x7ffffff0ull;                                         // a slot could not hold a candidate's index
  const uint32_t cnt = huge ? 0u : (uint32_t)cnt64;
  const UsCand* cands = in.cands + s0;
  const uint8_t* arena = in.rows.arena;
  for (uint32_t h = tid; h < NS; h += T) { weight_s[h] = 0ull; rep_s[h] = 0ull; slot_s[h] = 0u; segs_s[h] = 0u; }
  for (uint32_t h = tid; h < (NS + 31u) / 32u; h += T) taken_s[h] = 0u;
  if (tid == 0u) { top_s = 0ull; total_s = 0ull; ncls_s = 0u; over_s = 0u; }
  __syncthreads();
  // ---- the classes
  for (uint32_t i = tid; i < cnt; i += T) {
    const UsCand c = cands[i];
    if (c.p == 0u) continue;
    atomicAdd(&total_s, (unsigned long long)c.length);
    const uint32_t r = us_table_insert(slot_s, NS, cands, i, arena, UsLdsCas{});
    if (r == US_NONE) { over_s = 1u; continue; }
    const uint32_t h = r & ~US_FRESH;
    if (r & US_FRESH) atomicAdd(&ncls_s, 1u);
    atomicAdd(&weight_s[h], (unsigned long long)c.length);
    atomicAdd(&segs_s[h], 1u);
    atomicMax(&rep_s[h], (unsigned long long)us_rep_key(c.length, c.allele, c.begin));
  }
  __syncthreads();
  const bool overflow = huge || over_s != 0u || ncls_s > OTG_UNITSET_MAX_CLASSES;
  // ---- the largest weight, then the ranked classes one by one
  for (uint32_t h = tid; h < NS; h += T)
    if (slot_s[h]) atomicMax(&top_s, weight_s[h]);
  __syncthreads();
  const uint64_t top = top_s;
  uint32_t n_ranked = 0;
  for (uint32_t round = 0; round < OTG_UNITSET_TOP && !overflow; ++round) {
    uint32_t best = US_NONE;
    for (uint32_t h = tid; h < NS; h += T) {
      if (!slot_s[h] || ((taken_s[h >> 5] >> (h & 31u)) & 1u) || !us_eligible(weight_s[h], top, in.q)) continue;
      if (best == US_NONE) { best = h; continue; }
      const UsCand x = cands[slot_s[h] - 1u], y = cands[slot_s[best] - 1u];
      if (us_before(arena, weight_s[h], x.p, x.pos, x.rot, weight_s[best], y.p, y.pos, y.rot)) best = h;
    }
    red_s[tid] = best;
    __syncthreads();
    for (uint32_t d = T / 2u; d > 0u; d >>= 1) {
      if (tid < d) {
        const uint32_t u = red_s[tid], v = red_s[tid + d];
        uint32_t w = u;
        if (u == US_NONE) w = v;
        else if (v != US_NONE) {
          const UsCand x = cands[slot_s[v] - 1u], y = cands[slot_s[u] - 1u];
          if (us_before(arena, weight_s[v], x.p, x.pos, x.rot, weight_s[u], y.p, y.pos, y.rot)) w = v;
        }
        red_s[tid] = w;
      }
      __syncthreads();
    }
    const uint32_t win = red_s[0];
    if (win == US_NONE) break;                                                     // the same word for every thread
    if (tid == 0u) { rank_s[round] = win; taken_s[win >> 5] |= 1u << (win & 31u); }
    n_ranked = round + 1u;
    __syncthreads();
  }
  __syncthreads();
  if (tid < n_ranked) {
    const uint32_t h = rank_s[tid];
    const uint64_t key = rep_s[h];
    UsEntry e;
    e.weight = weight_s[h]; e.segments = segs_s[h]; e.p = cands[slot_s[h] - 1u].p;
    e.pos = in.rows.off[us_rep_allele(key)] + us_rep_begin(key);
    entries[(size_t)g * OTG_UNITSET_TOP + tid] = e;
    rank_p[(size_t)g * OTG_UNITSET_TOP + tid] = e.p;
  }
  if (tid == 0u) {
    otg_unitset s;
    s.n_units = 0u; s.n_classes = overflow ? OTG_UNITSET_MAX_CLASSES + 1u : ncls_s; s.n_ranked = n_ranked;
    s.flags = overflow ? OTG_UNITSET_OVERFLOW : 0u; s.weight_total = total_s;
    sets[g] = s;
  }
}

struct UsRanked { const otg_unitset* s; __device__ __forceinline__ uint64_t operator()(uint32_t g) const { return s[g].n_ranked; } };
struct UsPairs { const otg_unitset* s; __device__ __forceinline__ uint64_t operator()(uint32_t g) const { return us_pairs(s[g].n_ranked); } };
struct UsUnits { const otg_unitset* s; __device__ __forceinline__ uint64_t operator()(uint32_t g) const { return s[g].n_units; } };

__global__ __launch_bounds__(US_T) void us_tasks(uint32_t n_groups, const otg_unitset* __restrict__ sets, const UsEntry* __restrict__ entries,
                                                const uint64_t* __restrict__ rank_first, const uint64_t* __restrict__ pair_first, uint64_t* __restrict__ row_off,
                                                uint32_t* __restrict__ row_len, uint32_t* __restrict__ unit_len, uint32_t* __restrict__ task_seq,
                                                uint32_t* __restrict__ task_unit)
{
  const uint32_t g = blockIdx.x * US_T + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t nr = sets[g].n_ranked;
  const uint64_t r0 = rank_first[g], p0 = pair_first[g];
  for (uint32_t c = 0; c < nr; ++c) {
    const UsEntry e = entries[(size_t)g * OTG_UNITSET_TOP + c];
    row_off[r0 + c] = e.pos; row_len[r0 + c] = 2u * e.p; unit_len[r0 + c] = e.p;
    for (uint32_t d = 0; d < c; ++d) {
      task_seq[p0 + us_pair_index(c, d)] = (uint32_t)(r0 + c);
      task_unit[p0 + us_pair_index(c, d)] = (uint32_t)(r0 + d);
    }
  }
}

__global__ __launch_bounds__(US_T) void us_select_groups(uint32_t n_groups, otg_unitset_params q, otg_unitset* __restrict__ sets, const uint32_t* __restrict__ rank_p,
                                                        const uint64_t* __restrict__ pair_first, const otg_unitalign* __restrict__ pairs, uint32_t* __restrict__ sel,
                                                        uint32_t* __restrict__ group_bytes)
{
  const uint32_t g = blockIdx.x * US_T + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t nr = sets[g].n_ranked;
  const uint32_t* p = rank_p + (size_t)g * OTG_UNITSET_TOP;
  const uint64_t p0 = pair_first[g];
  uint32_t redundant = 0u;
  for (uint32_t c = 1; c < nr; ++c)
    for (uint32_t d = 0; d < c; ++d)
      if (us_explained(pairs[p0 + us_pair_index(c, d)].edits, p[c], q)) redundant |= 1u << c;
  uint32_t* mine = sel + (size_t)g * OTG_UNITPARSE_MAX_UNITS;
  const uint32_t taken = us_select(p, nr, redundant, mine);
  uint32_t bytes = 0;
  for (uint32_t k = 0; k < taken; ++k) bytes += p[mine[k]];
  group_bytes[g] = bytes;
  sets[g].n_units = taken;
  if (taken == 0u) sets[g].flags |= OTG_UNITSET_NONE;
}

__global__ __launch_bounds__(64) void us_write(OtgRows rows, const otg_unitset* __restrict__ sets, const UsEntry* __restrict__ entries, const uint32_t* __restrict__ sel,
                                              const uint64_t* __restrict__ set_first, const uint64_t* __restrict__ byte_first, otg_unitset_unit* __restrict__ units,
                                              uint64_t* __restrict__ unit_off, uint32_t* __restrict__ unit_len, uint8_t* __restrict__ bytes)
{
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  const uint32_t K = sets[g].n_units;
  const uint64_t k0 = set_first[g];
  uint64_t b = byte_first[g];
  for (uint32_t k = 0; k < K; ++k) {
    const UsEntry e = entries[(size_t)g * OTG_UNITSET_TOP + sel[(size_t)g * OTG_UNITPARSE_MAX_UNITS + k]];
    if (lane == 0u) {
      otg_unitset_unit u;
      u.weight = e.weight; u.segments = e.segments; u.length = e.p;
      units[k0 + k] = u; unit_off[k0 + k] = b; unit_len[k0 + k] = e.p;
    }
    for (uint32_t j = lane; j < e.p; j += 64u) {
      const uint32_t c = mo_code(rows.arena[e.pos + j]);
      bytes[b + j] = c == 0u ? 'A' : c == 1u ? 'C' : c == 2u ? 'G' : c == 3u ? 'T' : 'N';
    }
    b += e.p;
  }
}

// allele i of the repeat call: amap[i] = the tasks before it, bit 31 set when it is a task itself
__global__ __launch_bounds__(US_T) void us_spread(uint32_t n, const uint32_t* __restrict__ amap, const otg_locus* __restrict__ task_rec, const uint64_t* __restrict__ task_off,
                                                 otg_locus* __restrict__ out, uint64_t* __restrict__ off_out)
{
  const uint32_t i = blockIdx.x * US_T + threadIdx.x;
  if (i > n) return;
  const uint32_t m = amap[i], t = m & 0x7fffffffu;
  off_out[i] = task_off[t];
  if (i == n) return;
  otg_locus rec;
  if (m >> 31) rec = task_rec[t];
  else { rec.score = rec.begin = rec.end = rec.edits = rec.switches = rec.unit_bases = rec.n_segments = 0u; rec.flags = OTG_UNITSET_LOCUS_NO_SET; }
  out[i] = rec;
}

uint32_t us_hash_bits()
{
  static const uint32_t bits = [] {
    const char* e = getenv("OTG_UNITSET_HASH_BITS");
    const long v = e && *e ? strtol(e, nullptr, 10) : 64;
    return (uint32_t)(v >= 1 && v <= 64 ? v : 64);
  }();
  return bits;
}

// are the alleles of the latest repeat call still where it read them: the context's own copy, or the rows of the cohort batch?
bool us_rows_live(otg_ctx* ctx)
{
  const uint8_t* a = ctx->last_repeat_rows.arena;
  return a && (a == (const uint8_t*)ctx->pool[SLOT_REPEAT_SEQ].p || otg_cohort_holds_rows(ctx, a));
}

} // namespace

extern "C" void otg_unitset_params_default(otg_unitset_params* params)
{
  if (!params) return;
  params->min_bases = 12u; params->min_permille = 50u; params->redundant_permille = 100u; params->reserved = 0u;
}

extern "C" int otg_unitset_repeats(otg_ctx* ctx, const uint32_t* group_first, uint32_t n_groups, const otg_unitset_params* params, otg_unitset* sets,
                                   uint64_t* set_first, uint64_t* n_units, uint64_t* unit_bytes)
{
  otg_unitset_params q;
  if (params) q = *params;
  else otg_unitset_params_default(&q);
  if (!us_params_ok(q))
    return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_repeats: params (min_bases %u, min_permille %u, redundant_permille %u, reserved %u) outside 1..%u, 0..1000, 0..1000, 0",
                    q.min_bases, q.min_permille, q.redundant_permille, q.reserved, 1u << 24);
  if (!group_first) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_repeats: NULL group_first");
  if (n_groups > (1u << 24)) return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_unitset_repeats: %u groups in one call, at most %u", n_groups, 1u << 24);
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_unitset_repeats: no context (no HIP device?)");
  ctx->last_unitset = otg_ctx::UnitsetLast{};
  if (n_units) *n_units = 0;
  if (unit_bytes) *unit_bytes = 0;
  if (!ctx->last_repeat.valid) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_repeats: no repeat results on this context");
  const uint32_t n = ctx->last_repeat.n, G = n_groups;
  if (group_first[0] != 0u || group_first[G] != n)
    return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_repeats: group_first runs from %u to %u, the latest repeat call has alleles 0 to %u", group_first[0], group_first[G], n);
  for (uint32_t g = 0; g < G; ++g)
    if (group_first[g] > group_first[g + 1])
      return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_repeats: group_first[%u] = %u lies above group_first[%u] = %u", g, group_first[g], g + 1, group_first[g + 1]);
  if (!us_rows_live(ctx)) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_repeats: the alleles of the latest repeat call are no longer on the device");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const OtgRows rows = ctx->last_repeat_rows;
  const uint64_t total_segs = ctx->last_repeat.total;
  const uint8_t* rp_res = (const uint8_t*)ctx->pool[SLOT_REPEAT_RES].p;
  const uint64_t* d_segoff = (const uint64_t*)(rp_res + (size_t)n * sizeof(otg_repeat_sum));
  const otg_repeat_seg* d_segs = (const otg_repeat_seg*)ctx->pool[SLOT_REPEAT_SEGS].p;
  // WORK: entries (G x TOP) | rank_first, pair_first (u64, G + 1 each) | four totals | rank_p (u32, G x TOP) | sel (u32, G x MAX_UNITS) | group_bytes (u32, G) | group_first (u32, G + 1)
  const size_t work_bytes = (size_t)G * OTG_UNITSET_TOP * sizeof(UsEntry) + ((size_t)2 * (G + 1) + 4) * 8 +
                            ((size_t)G * (OTG_UNITSET_TOP + OTG_UNITPARSE_MAX_UNITS + 2) + 1) * 4;
  uint8_t* d_work = (uint8_t*)otg_slot(ctx, SLOT_UNITSET_WORK, work_bytes);
  UsCand* d_cands = (UsCand*)otg_slot(ctx, SLOT_UNITSET_CAND, (size_t)total_segs * sizeof(UsCand));
  // RES: the sets | set_first (u64, G + 1) | byte_first (u64, G + 1)
  uint8_t* d_res = (uint8_t*)otg_slot(ctx, SLOT_UNITSET_RES, (size_t)G * sizeof(otg_unitset) + (size_t)2 * (G + 1) * 8);
  if (!d_work || !d_cands || !d_res) return OTG_ERR_HIP;
  UsEntry* d_entries = (UsEntry*)d_work;
  uint64_t* d_rank_first = (uint64_t*)(d_entries + (size_t)G * OTG_UNITSET_TOP);
  uint64_t* d_pair_first = d_rank_first + (G + 1);
  uint64_t* d_tot = d_pair_first + (G + 1);
  uint32_t* d_rank_p = (uint32_t*)(d_tot + 4);
  uint32_t* d_sel = d_rank_p + (size_t)G * OTG_UNITSET_TOP;
  uint32_t* d_gbytes = d_sel + (size_t)G * OTG_UNITPARSE_MAX_UNITS;
  uint32_t* d_gf = d_gbytes + G;
  otg_unitset* d_sets = (otg_unitset*)d_res;
  uint64_t* d_set_first = (uint64_t*)(d_res + (size_t)G * sizeof(otg_unitset));
  uint64_t* d_byte_first = d_set_first + (G + 1);
  HIP_TRY(ctx, hipMemcpyAsync(d_gf, group_first, ((size_t)G + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_tot, 0, 32, ctx->stream));
  const uint32_t ggrid = (G + US_T - 1) / US_T;
  // ---- candidates and vote
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(us_candidates, dim3(n), dim3(64), 0, ctx->stream, rows, d_segoff, d_segs, us_hash_bits(), d_cands);
  const UsVoteIn vin{rows, d_segoff, d_gf, d_cands, q};
  hipLaunchKernelGGL((us_vote<US_SLOTS_SMALL, 64u, true>), dim3(G), dim3(64), 0, ctx->stream, vin, d_sets, d_entries, d_rank_p);
  hipLaunchKernelGGL((us_vote<US_SLOTS_BIG, US_T, false>), dim3(G), dim3(US_T), 0, ctx->stream, vin, d_sets, d_entries, d_rank_p);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, UsRanked>), dim3(1), dim3(1024), 0, ctx->stream, UsRanked{d_sets}, G, d_rank_first, d_tot);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, UsPairs>), dim3(1), dim3(1024), 0, ctx->stream, UsPairs{d_sets}, G, d_pair_first, d_tot + 1);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  uint64_t tot[4] = {0, 0, 0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float vote_ms = 0.f, tail_ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&vote_ms, ctx->ev0, ctx->ev1));
  // ---- the redundancy test: ranked class c twice in a row against the representative of every class ranked before it
  const uint64_t R = tot[0], P = tot[1];
  double align_ms = 0.0;
  const otg_unitalign* d_pairs = nullptr;
  if (P) {
    // TASKS: row_off (u64, R) | row_len, unit_len (u32, R each) | task_seq, task_unit (u32, P each)
    uint8_t* d_tasks = (uint8_t*)otg_slot(ctx, SLOT_UNITSET_TASKS, (size_t)R * 16 + (size_t)P * 8);
    otg_unitalign* d_pair_out = (otg_unitalign*)otg_slot(ctx, SLOT_UNITSET_PAIRS, (size_t)P * sizeof(otg_unitalign));
    if (!d_tasks || !d_pair_out) return OTG_ERR_HIP;
    uint64_t* d_row_off = (uint64_t*)d_tasks;
    uint32_t* d_row_len = (uint32_t*)(d_row_off + R);
    uint32_t* d_unit_len = d_row_len + R;
    uint32_t* d_task_seq = d_unit_len + R;
    uint32_t* d_task_unit = d_task_seq + P;
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));              // (the unit alignment below takes both events for itself: read this one first)
    hipLaunchKernelGGL(us_tasks, dim3(ggrid), dim3(US_T), 0, ctx->stream, G, d_sets, d_entries, d_rank_first, d_pair_first, d_row_off, d_row_len, d_unit_len, d_task_seq,
                       d_task_unit);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float tasks_ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&tasks_ms, ctx->ev0, ctx->ev1));
    align_ms += (double)tasks_ms;
    const OtgRows doubled{rows.arena, d_row_off, d_row_len};
    const OtgUnitSource reps{rows.arena, d_row_off, d_unit_len, nullptr, 0u};
    for (uint64_t first = 0; first < P; first += 1u << 24) {                       // the unit alignment takes 2^24 tasks per call
      const uint32_t count = (uint32_t)std::min<uint64_t>(P - first, 1u << 24);
      if (int rc = otg_unitalign_resident(ctx, "otg_unitset_repeats", doubled, reps, d_task_seq + first, d_task_unit + first, count, nullptr)) return rc;
      align_ms += ctx->last_unitalign_ms;
      HIP_TRY(ctx, hipMemcpyAsync(d_pair_out + first, ctx->pool[SLOT_UNITALIGN_OUT].p, (size_t)count * sizeof(otg_unitalign), hipMemcpyDeviceToDevice, ctx->stream));
    }
    d_pairs = d_pair_out;
  }
  // ---- the select, the offsets, the units
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(us_select_groups, dim3(ggrid), dim3(US_T), 0, ctx->stream, G, q, d_sets, d_rank_p, d_pair_first, d_pairs, d_sel, d_gbytes);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, UsUnits>), dim3(1), dim3(1024), 0, ctx->stream, UsUnits{d_sets}, G, d_set_first, d_tot + 2);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, OtgScanPtr<uint32_t>>), dim3(1), dim3(1024), 0, ctx->stream, OtgScanPtr<uint32_t>{d_gbytes}, G, d_byte_first,
                     d_tot + 3);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(tot + 2, d_tot + 2, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t U = tot[2], B = tot[3];
  // UNITS: the unit records (U) | unit_off (u64, U) | unit_len (u32, U) | the bytes
  uint8_t* d_units = (uint8_t*)otg_slot(ctx, SLOT_UNITSET_UNITS, (size_t)U * (sizeof(otg_unitset_unit) + 12) + B + 16);
  if (!d_units) return OTG_ERR_HIP;
  otg_unitset_unit* d_urec = (otg_unitset_unit*)d_units;
  uint64_t* d_uoff = (uint64_t*)(d_urec + U);
  uint32_t* d_ulen = (uint32_t*)(d_uoff + U);
  uint8_t* d_ubytes = (uint8_t*)(d_ulen + U);
  if (U) hipLaunchKernelGGL(us_write, dim3(G), dim3(64), 0, ctx->stream, rows, d_sets, d_entries, d_sel, d_set_first, d_byte_first, d_urec, d_uoff, d_ulen, d_ubytes);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  if (sets && G) HIP_TRY(ctx, hipMemcpyAsync(sets, d_sets, (size_t)G * sizeof(otg_unitset), hipMemcpyDeviceToHost, ctx->stream));
  if (set_first) HIP_TRY(ctx, hipMemcpyAsync(set_first, d_set_first, ((size_t)G + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&tail_ms, ctx->ev0, ctx->ev1));
  otg_ctx::UnitsetLast& last = ctx->last_unitset;
  last.n_groups = G; last.n_alleles = n; last.n_units = U; last.unit_bytes = B; last.repeat_serial = ctx->repeat_serial; last.valid = true;
  last.ms[0] = vote_ms; last.ms[1] = align_ms + (double)tail_ms;
  last.group_first.assign(group_first, group_first + G + 1);
  if (n_units) *n_units = U;
  if (unit_bytes) *unit_bytes = B;
  return OTG_OK;
}

extern "C" int otg_unitset_collect(otg_ctx* ctx, otg_unitset_unit* units, uint64_t* unit_off, uint32_t* unit_len, uint64_t unit_capacity, uint8_t* unit_arena,
                                   uint64_t arena_capacity)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_collect: NULL context");
  const otg_ctx::UnitsetLast& last = ctx->last_unitset;
  if (!last.valid) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_collect: no unit set results on this context");
  const uint64_t U = last.n_units, B = last.unit_bytes;
  if (unit_capacity < U || arena_capacity < B)
    return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_unitset_collect: capacities %llu units and %llu bytes, the latest call has %llu units and %llu bytes",
                    (unsigned long long)unit_capacity, (unsigned long long)arena_capacity, (unsigned long long)U, (unsigned long long)B);
  if (U == 0) return OTG_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint8_t* d = (const uint8_t*)ctx->pool[SLOT_UNITSET_UNITS].p;
  const size_t rec = (size_t)U * sizeof(otg_unitset_unit);
  if (units) HIP_TRY(ctx, hipMemcpyAsync(units, d, rec, hipMemcpyDeviceToHost, ctx->stream));
  if (unit_off) HIP_TRY(ctx, hipMemcpyAsync(unit_off, d + rec, (size_t)U * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (unit_len) HIP_TRY(ctx, hipMemcpyAsync(unit_len, d + rec + (size_t)U * 8, (size_t)U * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (unit_arena) HIP_TRY(ctx, hipMemcpyAsync(unit_arena, d + rec + (size_t)U * 12, (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OTG_OK;
}

extern "C" int otg_unitset_device_results(otg_ctx* ctx, uint32_t* n_groups, const otg_unitset** sets, const uint64_t** set_first, uint64_t* n_units,
                                          const otg_unitset_unit** units, const uint64_t** unit_off, const uint32_t** unit_len, const uint8_t** unit_arena,
                                          uint64_t* unit_bytes)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_device_results: NULL context");
  const otg_ctx::UnitsetLast& last = ctx->last_unitset;
  if (!last.valid) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_device_results: no unit set results on this context");
  const uint8_t* res = (const uint8_t*)ctx->pool[SLOT_UNITSET_RES].p;
  const uint8_t* d = (const uint8_t*)ctx->pool[SLOT_UNITSET_UNITS].p;
  const size_t rec = (size_t)last.n_units * sizeof(otg_unitset_unit);
  if (n_groups) *n_groups = last.n_groups;
  if (sets) *sets = (const otg_unitset*)res;
  if (set_first) *set_first = (const uint64_t*)(res + (size_t)last.n_groups * sizeof(otg_unitset));
  if (n_units) *n_units = last.n_units;
  if (units) *units = (const otg_unitset_unit*)d;
  if (unit_off) *unit_off = (const uint64_t*)(d + rec);
  if (unit_len) *unit_len = (const uint32_t*)(d + rec + (size_t)last.n_units * 8);
  if (unit_arena) *unit_arena = d + rec + (size_t)last.n_units * 12;
  if (unit_bytes) *unit_bytes = last.unit_bytes;
  return OTG_OK;
}

extern "C" int otg_unitset_last_ms(otg_ctx* ctx, double* vote_ms, double* select_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_last_ms: NULL context");
  if (vote_ms) *vote_ms = ctx->last_unitset.ms[0];
  if (select_ms) *select_ms = ctx->last_unitset.ms[1];
  return OTG_OK;
}

extern "C" int otg_unitset_locus(otg_ctx* ctx, const otg_tract_params* params, otg_locus* out, uint64_t* seg_off, uint64_t* n_segments)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_unitset_locus: no context (no HIP device?)");
  otg_tract_params q;
  if (int rc = otg_tract_args(ctx, "otg_unitset_locus", params, &q)) return rc;
  const otg_ctx::UnitsetLast& last = ctx->last_unitset;
  if (!last.valid) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_locus: no unit set results on this context");
  if (!ctx->last_repeat.valid || last.repeat_serial != ctx->repeat_serial || last.n_alleles != ctx->last_repeat.n)
    return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_locus: a repeat call lies between the discovery and this call");
  if (!us_rows_live(ctx)) return otg_fail(ctx, OTG_ERR_ARG, "otg_unitset_locus: the alleles of the latest repeat call are no longer on the device");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t n = last.n_alleles, G = last.n_groups;
  const uint64_t U = last.n_units, B = last.unit_bytes;
  const OtgRows rows = ctx->last_repeat_rows;
  // the sets are small (at most 8 units and 256 bases a group): they go through the host into the locus mode as a caller's would
  std::vector<uint64_t> set_first((size_t)G + 1), unit_off(U);
  std::vector<uint32_t> unit_len(U);
  std::vector<uint8_t> bytes(B);
  {
    const uint8_t* res = (const uint8_t*)ctx->pool[SLOT_UNITSET_RES].p;
    const uint8_t* d = (const uint8_t*)ctx->pool[SLOT_UNITSET_UNITS].p;
    const size_t rec = (size_t)U * sizeof(otg_unitset_unit);
    HIP_TRY(ctx, hipMemcpyAsync(set_first.data(), res + (size_t)G * sizeof(otg_unitset), ((size_t)G + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (U) {
      HIP_TRY(ctx, hipMemcpyAsync(unit_off.data(), d + rec, (size_t)U * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(unit_len.data(), d + rec + (size_t)U * 8, (size_t)U * 4, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(bytes.data(), d + rec + (size_t)U * 12, (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  // the groups with a set, in order, are the sets of the locus call (an empty set is refused there); their units are contiguous already
  std::vector<uint64_t> live_first;
  std::vector<uint32_t> task_seq, task_set, amap((size_t)n + 1);
  for (uint32_t g = 0; g < G; ++g) {
    const bool has = set_first[g + 1] > set_first[g];
    if (has) live_first.push_back(set_first[g]);
    for (uint32_t a = last.group_first[g]; a < last.group_first[g + 1]; ++a) {
      amap[a] = (uint32_t)task_seq.size() | (has ? 0x80000000u : 0u);
      if (has) { task_seq.push_back(a); task_set.push_back((uint32_t)live_first.size() - 1u); }
    }
  }
  const uint32_t T = (uint32_t)task_seq.size(), n_sets = (uint32_t)live_first.size();
  amap[n] = T;
  live_first.push_back(U);
  uint64_t total = 0;
  if (int rc = otg_locus_resident(ctx, "otg_unitset_locus", rows, nullptr, n, bytes.data(), B, unit_off.data(), unit_len.data(), (uint32_t)U, live_first.data(), n_sets,
                                  task_seq.data(), task_set.data(), T, q, nullptr, nullptr, &total))
    return rc;
  const OtgSegLast tasks = ctx->last_locus;                          // (all zero without a task)
  ctx->last_locus = OtgSegLast{};
  // the task records and offsets aside, then spread over the alleles into the slot the locus entries read
  const size_t t_bytes = (size_t)T * sizeof(otg_locus) + ((size_t)T + 1) * 8;
  uint8_t* d_tmp = (uint8_t*)otg_slot(ctx, SLOT_UNITSET_LOCUS, t_bytes + ((size_t)n + 1) * 4);
  if (!d_tmp) return OTG_ERR_HIP;
  if (T) HIP_TRY(ctx, hipMemcpyAsync(d_tmp, ctx->pool[SLOT_LOCUS_OUT].p, t_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  else HIP_TRY(ctx, hipMemsetAsync(d_tmp, 0, t_bytes, ctx->stream));
  uint32_t* d_amap = (uint32_t*)(d_tmp + t_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(d_amap, amap.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                    // growing the slot below may free what the copy reads
  uint8_t* d_res = (uint8_t*)otg_slot(ctx, SLOT_LOCUS_OUT, (size_t)n * sizeof(otg_locus) + ((size_t)n + 1) * 8);
  if (!d_res) return OTG_ERR_HIP;
  otg_locus* d_out = (otg_locus*)d_res;
  uint64_t* d_off_out = (uint64_t*)(d_res + (size_t)n * sizeof(otg_locus));
  hipLaunchKernelGGL(us_spread, dim3((n + 1 + US_T - 1) / US_T), dim3(US_T), 0, ctx->stream, n, d_amap, (const otg_locus*)d_tmp,
                     (const uint64_t*)(d_tmp + (size_t)T * sizeof(otg_locus)), d_out, d_off_out);
  HIP_TRY(ctx, hipGetLastError());
  if (out) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)n * sizeof(otg_locus), hipMemcpyDeviceToHost, ctx->stream));
  if (seg_off) HIP_TRY(ctx, hipMemcpyAsync(seg_off, d_off_out, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->last_locus = OtgSegLast{n, total, true, {tasks.ms[0], tasks.ms[1]}};
  if (n_segments) *n_segments = total;
  return OTG_OK;
}

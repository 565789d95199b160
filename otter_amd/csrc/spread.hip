// spread.hip — the spread operator (otg_assemble_spread): per consensus allele of an assemble batch, the order statistics of the repeat length
// among the reads that voted for it.  The reference has no counterpart; include/otter_gpu.h states the rule.
//
// Everything is read where otg_assemble_run left it (otg_pipeline_view): sp_rows turns the device otg_read array and the device otg_allele
// array into rows (off, len) over the reads' arena and over the consensus arena, as cohort_rows does for a cohort; only the reads' lengths,
// spanning flags and labels and the allele records come to the host, which builds the two task lists otg_locus_resident plans from.  The
// consensus alleles are parsed first; the context keeps only the latest locus results, so sp_ref copies ref_bases, the flag and the per-unit
// sums into the spread's own slot before the reads' call runs.  The reads' call goes last and its records stay behind for the caller.
// sp_stats then takes one wave per allele: it walks the region's contiguous reads 64 at a time, a lane holding the value of its read or
// SP_ABSENT when the read is no member, and finds the quantiles by selection on the value bits (otg_spread_core.hpp): no sort buffer, no
// LDS, no cap on the depth.  Regions of up to 64 SP_REG_STRIDES reads keep the series in registers, one stride per register; deeper ones
// re-read the records on every pass.
#include "otg_common.hpp"
#include "otg_spread_core.hpp"
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

using namespace otg_spread_core;

constexpr uint32_t SP_T = 256;
constexpr uint32_t SP_NONE = OTG_SPREAD_NONE;
constexpr uint32_t SP_TOTAL = 0xffffffffu;                        // the series of the whole set, not of one unit

__device__ __forceinline__ uint32_t sp_span(const otg_read& r) { return (r.spanning_l && r.spanning_r) ? 1u : 0u; }
__device__ __forceinline__ uint32_t sp_span(const otg_allele&) { return 1u; }

// the rows the descriptors name; span (nullable): both spanning flags
template <typename Rec>
__global__ __launch_bounds__(SP_T) void sp_rows(const Rec* __restrict__ recs, uint32_t n, uint64_t* __restrict__ off, uint32_t* __restrict__ len, uint32_t* __restrict__ span)
{
  const uint32_t i = blockIdx.x * SP_T + threadIdx.x;
  if (i >= n) return;
  const Rec r = recs[i];
  off[i] = r.seq_off; len[i] = r.seq_len;
  if (span) span[i] = sp_span(r);
}

// the read records: the row, the label and the task the host gave the read
__global__ __launch_bounds__(SP_T) void sp_reads(uint32_t n, const uint64_t* __restrict__ off, const uint32_t* __restrict__ len, const int32_t* __restrict__ labels,
                                                const uint32_t* __restrict__ task, otg_spread_read* __restrict__ out)
{
  const uint32_t i = blockIdx.x * SP_T + threadIdx.x;
  if (i >= n) return;
  otg_spread_read r;
  r.seq_off = off[i]; r.seq_len = len[i]; r.label = labels[i]; r.task = task[i]; r.counted = r.task != SP_NONE ? 1u : 0u;
  out[i] = r;
}

// the records before the statistics: zeros, and of the consensus allele's own locus record ref_bases, the per-unit sums and the flag
__global__ __launch_bounds__(SP_T) void sp_ref(uint32_t na, const uint32_t* __restrict__ a_task, const uint64_t* __restrict__ unit_off, const otg_locus* __restrict__ loci,
                                              const uint64_t* __restrict__ seg_off, const otg_unitparse_seg* __restrict__ segs, otg_spread* __restrict__ out,
                                              otg_spread_unit* __restrict__ units)
{
  const uint32_t a = blockIdx.x * SP_T + threadIdx.x;
  if (a >= na) return;
  otg_spread rec;
  memset(&rec, 0, sizeof rec);
  const uint32_t t = a_task[a];
  const uint64_t u0 = unit_off[a], K = unit_off[a + 1] - u0;
  if (t == SP_NONE) {
    rec.flags = OTG_SPREAD_NO_SET;
  } else {
    const bool has = loci[t].flags == 0u;
    rec.ref_bases = has ? loci[t].unit_bases : 0u;
    rec.flags = has ? 0u : OTG_SPREAD_REF_NONE;
    for (uint64_t k = 0; k < K; ++k) {
      otg_spread_unit u;
      memset(&u, 0, sizeof u);
      if (has)
        for (uint64_t g = seg_off[t]; g < seg_off[t + 1]; ++g) u.ref_bases += segs[g].unit == (uint32_t)k ? segs[g].unit_bases : 0u;
      units[u0 + k] = u;
    }
  }
  out[a] = rec;
}

struct SpIn {
  const otg_region* regions; const otg_allele* alleles; const int32_t* labels; const uint32_t* task;
  const otg_locus* loci; const uint64_t* seg_off; const otg_unitparse_seg* segs; const uint64_t* unit_off;
};

// the wave of otg_spread_core.hpp: a lane's own register per stride, the count by ballot
struct SpWave {
  using Vec = uint32_t;
  __device__ __forceinline__ uint32_t count_le(uint32_t v, uint32_t x) const { return (uint32_t)__popcll(__ballot(v <= x)); }
};

// the task of read i of the region when it is counted and carries the label, else SP_NONE
__device__ __forceinline__ uint32_t sp_task(const SpIn& in, uint32_t f, uint32_t n, int32_t label, uint32_t i)
{
  if (i >= n) return SP_NONE;
  const uint32_t t = in.task[f + i];
  return (t != SP_NONE && in.labels[f + i] == label) ? t : SP_NONE;
}
// the value of the read with task t for series u (a unit of the set, or SP_TOTAL); SP_ABSENT when the read is no member
__device__ __forceinline__ uint32_t sp_value(const SpIn& in, uint32_t t, uint32_t u)
{
  if (t == SP_NONE || in.loci[t].flags != 0u) return SP_ABSENT;
  if (u == SP_TOTAL) return in.loci[t].unit_bases;
  uint32_t sum = 0u;
  for (uint64_t g = in.seg_off[t]; g < in.seg_off[t + 1]; ++g) sum += in.segs[g].unit == u ? in.segs[g].unit_bases : 0u;
  return sum;
}
struct SpLoad {
  const SpIn& in; uint32_t f, n; int32_t label; uint32_t lane, u;
  __device__ __forceinline__ uint32_t operator()(uint32_t s) const { return sp_value(in, sp_task(in, f, n, label, s * 64u + lane), u); }
};

__device__ __forceinline__ uint64_t sp_wave_sum(uint64_t x)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
  return x;
}

// the five quantiles of series u; REG: the region has at most SP_REG_STRIDES strides
template <bool REG>
__device__ __forceinline__ void sp_series(const SpIn& in, uint32_t f, uint32_t n, int32_t label, uint32_t lane, uint32_t u, uint32_t m, uint32_t (&q)[5])
{
  const SpWave w{};
  SpLoad load{in, f, n, label, lane, u};
  if constexpr (REG) {
    uint32_t v[SP_REG_STRIDES];
#pragma unroll
    for (int s = 0; s < SP_REG_STRIDES; ++s) v[s] = load((uint32_t)s);          // (a stride past the region is SP_ABSENT)
    sp_quantiles_reg<SpWave, SP_REG_STRIDES>(w, v, m, q);
  } else {
    sp_quantiles_load<SpWave, SpLoad>(w, load, (n + 63u) / 64u, m, q);
  }
}

// one wave per allele; every branch below is wave-uniform
template <bool REG>
__global__ __launch_bounds__(64) void sp_stats(SpIn in, uint32_t na, const uint32_t* __restrict__ list, uint32_t count, otg_spread* __restrict__ out,
                                              otg_spread_unit* __restrict__ units)
{
  if (blockIdx.x >= count) return;
  const uint32_t a = list[blockIdx.x], lane = threadIdx.x;
  if (a >= na) return;
  otg_spread rec = out[a];                                          // sp_ref's: ref_bases and the flag
  if (rec.flags & OTG_SPREAD_NO_SET) return;
  const otg_allele al = in.alleles[a];
  const uint32_t f = in.regions[al.region].first_read, n = in.regions[al.region].n_reads;
  const int32_t label = al.label;
  const bool with_ref = !(rec.flags & OTG_SPREAD_REF_NONE);
  const uint32_t ref = rec.ref_bases;
  uint32_t n_reads = 0u, m = 0u, nb = 0u, nab = 0u;
  uint64_t sb = 0u, sa = 0u;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const uint32_t i = i0 + lane;
    const uint32_t t = sp_task(in, f, n, label, i);
    const uint32_t v = sp_value(in, t, SP_TOTAL);
    const bool member = v != SP_ABSENT;
    n_reads += (uint32_t)__popcll(__ballot(t != SP_NONE));
    m += (uint32_t)__popcll(__ballot(member));
    const bool below = member && with_ref && v < ref, above = member && with_ref && v > ref;
    nb += (uint32_t)__popcll(__ballot(below));
    nab += (uint32_t)__popcll(__ballot(above));
    sb += below ? (uint64_t)(ref - v) : 0ull;
    sa += above ? (uint64_t)(v - ref) : 0ull;
  }
  rec.n_reads = n_reads; rec.n_called = m; rec.n_below = nb; rec.n_above = nab;
  rec.sum_below = sp_wave_sum(sb); rec.sum_above = sp_wave_sum(sa);
  if (m == 0u) rec.flags |= OTG_SPREAD_NO_CALLS;
  sp_series<REG>(in, f, n, label, lane, SP_TOTAL, m, rec.q);
  if (lane == 0u) out[a] = rec;
  const uint64_t u0 = in.unit_off[a];
  const uint32_t K = (uint32_t)(in.unit_off[a + 1] - u0);
  for (uint32_t k = 0; k < K; ++k) {
    uint32_t q[5];
    sp_series<REG>(in, f, n, label, lane, k, m, q);
    if (lane == 0u) {
#pragma unroll
      for (int j = 0; j < 5; ++j) units[u0 + k].q[j] = q[j];
    }
  }
}

bool sp_force_reread()
{
  static const bool on = [] { const char* e = getenv("OTG_SPREAD_REREAD"); return e && *e && strcmp(e, "0") != 0; }();
  return on;
}

// HIP-event time of what was enqueued since sp_tick
int sp_tick(otg_ctx* ctx) { HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream)); return OTG_OK; }
int sp_tock(otg_ctx* ctx, double* ms)
{
  float t = 0.f;
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->ev0, ctx->ev1));
  *ms += (double)t;
  return OTG_OK;
}

} // namespace

extern "C" int otg_assemble_spread(otg_ctx* ctx, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off, const uint32_t* unit_len, uint32_t n_units,
                                   const uint64_t* set_first, uint32_t n_sets, const uint32_t* region_set, uint32_t n_regions, const otg_tract_params* params,
                                   otg_spread* out, uint64_t* unit_off_out, uint64_t* n_unit_records)
{
  const char* who = "otg_assemble_spread";
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "%s: no context (no HIP device?)", who);
  otg_tract_params q;
  if (int rc = otg_tract_args(ctx, who, params, &q)) return rc;
  OtgAssembleView v;
  if (!otg_pipeline_view(ctx, &v)) return otg_fail(ctx, OTG_ERR_ARG, "%s: no completed run on this context", who);
  if (n_regions != v.n_regions) return otg_fail(ctx, OTG_ERR_ARG, "%s: %u regions, the latest run has %u", who, n_regions, v.n_regions);
  if (n_regions && !region_set) return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL argument", who);
  if (int rc = otg_unitparse_check(ctx, who, 0u, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, nullptr, nullptr, 0u)) return rc;
  for (uint32_t r = 0; r < n_regions; ++r)
    if (region_set[r] != SP_NONE && region_set[r] >= n_sets)
      return otg_fail(ctx, OTG_ERR_ARG, "%s: region %u names set %u of %u", who, r, region_set[r], n_sets);
  ctx->last_spread = otg_ctx::SpreadLast{};
  ctx->last_locus.valid = false;
  if (n_unit_records) *n_unit_records = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t NR = v.n_reads, NG = v.n_regions, NA = v.n_alleles;
  hipStream_t st = ctx->stream;
  // ---- what the host needs of the batch: the region results, the allele records, and per read its label, length and spanning flags
  std::vector<otg_region_result> rr(NG);
  std::vector<otg_allele> al(NA);
  std::vector<int32_t> labels(NR);
  std::vector<uint32_t> r_len(NR), r_span(NR);
  // META: r_off (u64, NR) | a_off (u64, NA) | r_len, r_span, r_task (u32, NR each) | a_len, a_task (u32, NA each) | the alleles with statistics (u32, NA)
  uint8_t* d_meta = (uint8_t*)otg_slot(ctx, SLOT_SPREAD_META, (size_t)NR * 20 + (size_t)NA * 20 + 16);
  otg_spread_read* d_reads = (otg_spread_read*)otg_slot(ctx, SLOT_SPREAD_READS, (size_t)NR * sizeof(otg_spread_read) + 16);
  if (!d_meta || !d_reads) return OTG_ERR_HIP;
  uint64_t* d_roff = (uint64_t*)d_meta;
  uint64_t* d_aoff = d_roff + NR;
  uint32_t* d_rlen = (uint32_t*)(d_aoff + NA);
  uint32_t* d_rspan = d_rlen + NR;
  uint32_t* d_rtask = d_rspan + NR;
  uint32_t* d_alen = d_rtask + NR;
  uint32_t* d_atask = d_alen + NA;
  uint32_t* d_list = d_atask + NA;
  double ms_glue = 0.0, ms_reads = 0.0, ms_cons = 0.0, ms_stats = 0.0;
  if (int rc = sp_tick(ctx)) return rc;
  if (NR) hipLaunchKernelGGL((sp_rows<otg_read>), dim3((NR + SP_T - 1) / SP_T), dim3(SP_T), 0, st, v.reads, NR, d_roff, d_rlen, d_rspan);
  if (NA) hipLaunchKernelGGL((sp_rows<otg_allele>), dim3((NA + SP_T - 1) / SP_T), dim3(SP_T), 0, st, v.alleles, NA, d_aoff, d_alen, (uint32_t*)nullptr);
  if (int rc = sp_tock(ctx, &ms_glue)) return rc;
  if (v.results && NG) HIP_TRY(ctx, hipMemcpyAsync(rr.data(), v.results, (size_t)NG * sizeof(otg_region_result), hipMemcpyDeviceToHost, st));
  else for (auto& r : rr) { memset(&r, 0, sizeof r); r.status = OTG_REGION_EMPTY; }
  if (NA) HIP_TRY(ctx, hipMemcpyAsync(al.data(), v.alleles, (size_t)NA * sizeof(otg_allele), hipMemcpyDeviceToHost, st));
  if (NR) {
    HIP_TRY(ctx, hipMemcpyAsync(labels.data(), v.labels, (size_t)NR * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(r_len.data(), d_rlen, (size_t)NR * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(r_span.data(), d_rspan, (size_t)NR * 4, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  // ---- the task lists: the counted reads in read order, the alleles of regions with a set in record order
  std::vector<uint32_t> r_task(NR, SP_NONE), rt_seq, rt_set, a_task(NA, SP_NONE), at_seq, at_set, a_len(NA), list_reg, list_load;
  for (uint32_t r = 0; r < NG; ++r) {
    if (rr[r].status != OTG_REGION_OK || region_set[r] == SP_NONE) continue;
    const otg_region& g = v.h_regions[r];
    for (uint32_t i = g.first_read; i < g.first_read + g.n_reads; ++i)
      if (labels[i] >= 0 && r_span[i]) { r_task[i] = (uint32_t)rt_seq.size(); rt_seq.push_back(i); rt_set.push_back(region_set[r]); }
  }
  std::vector<uint64_t> h_unit_off((size_t)NA + 1, 0);
  const bool reread = sp_force_reread();
  for (uint32_t a = 0; a < NA; ++a) {
    a_len[a] = al[a].seq_len;
    if (al[a].region >= NG) return otg_fail(ctx, OTG_ERR_FATAL, "%s: allele %u names region %u of %u", who, a, al[a].region, NG);
    const uint32_t s = region_set[al[a].region];
    h_unit_off[a + 1] = h_unit_off[a];
    if (s == SP_NONE) continue;
    a_task[a] = (uint32_t)at_seq.size(); at_seq.push_back(a); at_set.push_back(s);
    h_unit_off[a + 1] += set_first[s + 1] - set_first[s];
    ((!reread && v.h_regions[al[a].region].n_reads <= 64u * SP_REG_STRIDES) ? list_reg : list_load).push_back(a);
  }
  const uint64_t NU = h_unit_off[NA];
  // OUT: the records | unit_off (u64, NA + 1) | the unit records
  uint8_t* d_res = (uint8_t*)otg_slot(ctx, SLOT_SPREAD_OUT, (size_t)NA * sizeof(otg_spread) + ((size_t)NA + 1) * 8 + (size_t)NU * sizeof(otg_spread_unit) + 16);
  if (!d_res) return OTG_ERR_HIP;
  otg_spread* d_out = (otg_spread*)d_res;
  uint64_t* d_unit_off = (uint64_t*)(d_res + (size_t)NA * sizeof(otg_spread));
  otg_spread_unit* d_units = (otg_spread_unit*)(d_unit_off + NA + 1);
  HIP_TRY(ctx, hipMemcpyAsync(d_unit_off, h_unit_off.data(), ((size_t)NA + 1) * 8, hipMemcpyHostToDevice, st));
  if (NR) HIP_TRY(ctx, hipMemcpyAsync(d_rtask, r_task.data(), (size_t)NR * 4, hipMemcpyHostToDevice, st));
  if (NA) HIP_TRY(ctx, hipMemcpyAsync(d_atask, a_task.data(), (size_t)NA * 4, hipMemcpyHostToDevice, st));
  if (!list_reg.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_list, list_reg.data(), list_reg.size() * 4, hipMemcpyHostToDevice, st));
  if (!list_load.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_list + list_reg.size(), list_load.data(), list_load.size() * 4, hipMemcpyHostToDevice, st));
  // ---- the consensus alleles first: their results move into the spread's own slot before the reads' call replaces them
  const uint32_t n_at = (uint32_t)at_seq.size(), n_rt = (uint32_t)rt_seq.size();
  if (int rc = otg_locus_resident(ctx, who, OtgRows{v.seqs, d_aoff, d_alen}, a_len.data(), NA, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets,
                                  at_seq.data(), at_set.data(), n_at, q, nullptr, nullptr, nullptr))
    return rc;
  ms_cons = n_at ? ctx->last_locus.ms[0] : 0.0;
  if (NA) {
    const uint8_t* res = (const uint8_t*)ctx->pool[SLOT_LOCUS_OUT].p;
    if (int rc = sp_tick(ctx)) return rc;
    hipLaunchKernelGGL(sp_ref, dim3((NA + SP_T - 1) / SP_T), dim3(SP_T), 0, st, NA, (const uint32_t*)d_atask, (const uint64_t*)d_unit_off, (const otg_locus*)res,
                       (const uint64_t*)(res + (size_t)n_at * sizeof(otg_locus)), (const otg_unitparse_seg*)ctx->pool[SLOT_UNITPARSE_SEGS].p, d_out, d_units);
    if (int rc = sp_tock(ctx, &ms_glue)) return rc;
  }
  // ---- the reads last: their records stay on the context
  if (int rc = otg_locus_resident(ctx, who, OtgRows{v.arena, d_roff, d_rlen}, r_len.data(), NR, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets,
                                  rt_seq.data(), rt_set.data(), n_rt, q, nullptr, nullptr, nullptr))
    return rc;
  ms_reads = n_rt ? ctx->last_locus.ms[0] : 0.0;
  if (int rc = sp_tick(ctx)) return rc;
  if (NR) hipLaunchKernelGGL(sp_reads, dim3((NR + SP_T - 1) / SP_T), dim3(SP_T), 0, st, NR, (const uint64_t*)d_roff, (const uint32_t*)d_rlen, v.labels, (const uint32_t*)d_rtask, d_reads);
  if (int rc = sp_tock(ctx, &ms_glue)) return rc;
  {
    const uint8_t* res = (const uint8_t*)ctx->pool[SLOT_LOCUS_OUT].p;
    const SpIn in{v.regions, v.alleles, v.labels, d_rtask, (const otg_locus*)res, (const uint64_t*)(res + (size_t)n_rt * sizeof(otg_locus)),
                  (const otg_unitparse_seg*)ctx->pool[SLOT_UNITPARSE_SEGS].p, d_unit_off};
    if (int rc = sp_tick(ctx)) return rc;
    if (!list_reg.empty())
      hipLaunchKernelGGL((sp_stats<true>), dim3((uint32_t)list_reg.size()), dim3(64), 0, st, in, NA, (const uint32_t*)d_list, (uint32_t)list_reg.size(), d_out, d_units);
    if (!list_load.empty())
      hipLaunchKernelGGL((sp_stats<false>), dim3((uint32_t)list_load.size()), dim3(64), 0, st, in, NA, (const uint32_t*)(d_list + list_reg.size()), (uint32_t)list_load.size(),
                         d_out, d_units);
    if (int rc = sp_tock(ctx, &ms_stats)) return rc;
  }
  if (out && NA) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)NA * sizeof(otg_spread), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (unit_off_out) memcpy(unit_off_out, h_unit_off.data(), ((size_t)NA + 1) * 8);
  if (n_unit_records) *n_unit_records = NU;
  ctx->last_spread.n_alleles = NA; ctx->last_spread.n_reads = NR; ctx->last_spread.n_units = NU; ctx->last_spread.valid = true;
  ctx->last_spread.ms[0] = ms_glue + ms_reads + ms_cons + ms_stats; ctx->last_spread.ms[1] = ms_reads; ctx->last_spread.ms[2] = ms_cons; ctx->last_spread.ms[3] = ms_stats;
  return OTG_OK;
}

extern "C" int otg_spread_collect(otg_ctx* ctx, otg_spread_unit* units, uint64_t capacity)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_spread_collect: NULL context");
  const otg_ctx::SpreadLast& last = ctx->last_spread;
  if (!last.valid) return otg_fail(ctx, OTG_ERR_ARG, "otg_spread_collect: no spread results on this context");
  if (capacity < last.n_units || (last.n_units && !units))
    return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_spread_collect: capacity %llu, the latest call has %llu unit records", (unsigned long long)capacity, (unsigned long long)last.n_units);
  if (last.n_units == 0) return OTG_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint8_t* res = (const uint8_t*)ctx->pool[SLOT_SPREAD_OUT].p;
  HIP_TRY(ctx, hipMemcpyAsync(units, res + (size_t)last.n_alleles * sizeof(otg_spread) + ((size_t)last.n_alleles + 1) * 8, (size_t)last.n_units * sizeof(otg_spread_unit),
                              hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OTG_OK;
}

extern "C" int otg_spread_collect_reads(otg_ctx* ctx, otg_spread_read* reads, uint32_t capacity)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_spread_collect_reads: NULL context");
  const otg_ctx::SpreadLast& last = ctx->last_spread;
  if (!last.valid) return otg_fail(ctx, OTG_ERR_ARG, "otg_spread_collect_reads: no spread results on this context");
  if (capacity < last.n_reads || (last.n_reads && !reads))
    return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_spread_collect_reads: capacity %u, the latest call has %u reads", capacity, last.n_reads);
  if (last.n_reads == 0) return OTG_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(reads, ctx->pool[SLOT_SPREAD_READS].p, (size_t)last.n_reads * sizeof(otg_spread_read), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OTG_OK;
}

extern "C" int otg_spread_device_results(otg_ctx* ctx, uint32_t* n_alleles, const otg_spread** records, const uint64_t** unit_off, uint64_t* n_unit_records,
                                         const otg_spread_unit** units, uint32_t* n_reads, const otg_spread_read** reads)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_spread_device_results: NULL context");
  const otg_ctx::SpreadLast& last = ctx->last_spread;
  if (!last.valid) return otg_fail(ctx, OTG_ERR_ARG, "otg_spread_device_results: no spread results on this context");
  const uint8_t* res = (const uint8_t*)ctx->pool[SLOT_SPREAD_OUT].p;
  const uint8_t* off = res + (size_t)last.n_alleles * sizeof(otg_spread);
  if (n_alleles) *n_alleles = last.n_alleles;
  if (records) *records = (const otg_spread*)res;
  if (unit_off) *unit_off = (const uint64_t*)off;
  if (n_unit_records) *n_unit_records = last.n_units;
  if (units) *units = (const otg_spread_unit*)(off + ((size_t)last.n_alleles + 1) * 8);
  if (n_reads) *n_reads = last.n_reads;
  if (reads) *reads = (const otg_spread_read*)ctx->pool[SLOT_SPREAD_READS].p;
  return OTG_OK;
}

extern "C" int otg_spread_last_ms(otg_ctx* ctx, double* ms, double* reads_ms, double* consensus_ms, double* stats_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_spread_last_ms: NULL context");
  if (ms) *ms = ctx->last_spread.ms[0];
  if (reads_ms) *reads_ms = ctx->last_spread.ms[1];
  if (consensus_ms) *consensus_ms = ctx->last_spread.ms[2];
  if (stats_ms) *stats_ms = ctx->last_spread.ms[3];
  return OTG_OK;
}

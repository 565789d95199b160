// cohort.hip — the bridge between `otter assemble` and `otter genotype` on the device.
//
// The reference's cohort workflow runs `otter assemble` per sample, merges the per-sample allele BAMs and runs `otter genotype` on the merge
// (src/assemble.cpp:143-149 writes the records, src/anseqs.cpp:462-524 reads them back, src/genotype.cpp:85-101 groups them per region and
// appends the reference allele).  Here the alleles of a batch of B regions never leave HBM between the two commands:
//   stage    after otg_assemble_run of sample s: its otg_allele records (tagged with the sample) and allele bytes are copied device to device
//            into the staging area, its per-region allele counts into row s of an S x B table;
//   regroup  a scan over the table and a gather write what genotype_kernel consumes — arena, seq_off, seq_len, first_allele, n_alleles —
//            region-major, sample-major inside a region (the order the BAMs were given), alleles of a sample in label order, the reference
//            allele last with sample index S (OTTER_INTREF, src/genotype.cpp:186-188); a region without sample alleles has no reference
//            allele either (src/genotype.cpp:90); a zero-length allele becomes "N" (src/anseqs.cpp:505-507);
//   cluster  otg_genotype_resident (the launch part of otg_genotype_cluster_batch) on those buffers;
//   collect  D2H of the results, the allele records and the regrouped bytes for the VCF text;
//   rows     after the clustering, the alleles of every VCF line in column order (the rows of `otter vcf2mat` on that VCF) and the GT numbers of
//            every sample, selected on the device; the k-mer tiers (kmer_usage.hip) read those rows in the regrouped arena, in place.
#include "otg_common.hpp"
#include "otg_scan.hpp"
#include <algorithm>

struct Cohort {
  uint32_t B = 0, S = 0;
  bool open = false, regrouped = false, clustered = false;
  std::vector<uint8_t> staged;                       // per sample
  uint64_t n_staged = 0, staged_bytes = 0;           // totals of the staged runs (known on the host from otg_assemble_result_sizes)
  DevBuf stg_al, stg_seq, cnt, sfirst;               // staging: records, bytes, S x B counts, S x B index of the first staged record
  DevBuf ref_seq, ref_off, ref_len;                  // reference alleles of the batch
  DevBuf n_al, first, pairs, pair_off, src_of, seq_len, seq_off, smp, meta, arena, gt, hsd, ngt;
  DevBuf row_first, row_allele, row_off, row_len, sample_gt;   // the row list of otg_kmer_cohort_rows
  bool rows_built = false;
  uint32_t n_rows = 0;
  std::vector<uint32_t> h_first, h_n_al;
  std::vector<uint64_t> h_pair_off;
  uint32_t na = 0;
  uint64_t seq_bytes = 0;
  DevBuf* all[25] = {&stg_al, &stg_seq, &cnt, &sfirst, &ref_seq, &ref_off, &ref_len, &n_al, &first, &pairs, &pair_off, &src_of, &seq_len, &seq_off,
                     &smp, &meta, &arena, &gt, &hsd, &ngt, &row_first, &row_allele, &row_off, &row_len, &sample_gt};
};

void otg_cohort_free(otg_ctx* ctx)
{
  if (!ctx || !ctx->cohort) return;
  for (DevBuf* b : ctx->cohort->all) if (b->p) (void)hipFree(b->p);
  delete ctx->cohort;
  ctx->cohort = nullptr;
}

namespace {

constexpr uint32_t REF_FLAG = 0x80000000u;           // src_of entry of a reference allele: REF_FLAG | region

// grow-only buffer of the staging area; the first `keep` bytes survive a re-allocation (device-to-device)
int grow(otg_ctx* ctx, DevBuf& b, size_t bytes, size_t keep = 0)
{
  if (bytes == 0) bytes = 16;
  if (b.cap >= bytes) return OTG_OK;
  const size_t want = bytes + (bytes >> 1) + 256;
  void* q = nullptr;
  HIP_TRY(ctx, hipMalloc(&q, want));
  if (b.p) {
    if (keep) HIP_TRY(ctx, hipMemcpyAsync(q, b.p, std::min(keep, b.cap), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(b.p));
  }
  b.p = q; b.cap = want;
  return OTG_OK;
}

// ---- stage: the records of one run, tagged with their sample, and its row of the count table
__global__ void cohort_stage_kernel(const otg_region_result* __restrict__ rr, const otg_allele* __restrict__ al, uint32_t n_regions, uint32_t n_al,
                                    uint32_t sample, uint32_t a_base, uint64_t byte_base, otg_allele* __restrict__ stg,
                                    uint32_t* __restrict__ cnt_row, uint32_t* __restrict__ sfirst_row)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_regions) {
    const otg_region_result R = rr[i];
    const bool ok = (uint64_t)R.first_allele + R.n_alleles <= n_al;      // (a record range outside the run's table is dropped, never followed)
    cnt_row[i] = ok ? R.n_alleles : 0u;
    sfirst_row[i] = a_base + (ok ? R.first_allele : 0u);
  }
  if (i < n_al) {
    otg_allele a = al[i];
    a.seq_off += byte_base;
    a.label = (int32_t)sample;
    stg[a_base + i] = a;
  }
}

// ---- regroup 1: alleles and allele pairs per region
__global__ void cohort_region_counts_kernel(const uint32_t* __restrict__ cnt, uint32_t B, uint32_t S, uint32_t* __restrict__ n_al, uint64_t* __restrict__ pairs)
{
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  uint32_t tot = 0;
  for (uint32_t s = 0; s < S; ++s) tot += cnt[(size_t)s * B + r];
  const uint32_t A = tot ? tot + 1u : 0u;                                // + the reference allele, only where a sample has an allele
  n_al[r] = A;
  pairs[r] = (uint64_t)A * (A ? A - 1u : 0u) / 2u;
}

// ---- regroup 2 / 4: exclusive scans of the counts (otg_scan_kernel, otg_scan.hpp)

// ---- regroup 3: the place of every allele in its region (sample-major, reference last): source record, output length, sample index
__global__ void cohort_place_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ sfirst, uint32_t B, uint32_t S,
                                    const uint32_t* __restrict__ first, const uint32_t* __restrict__ n_al, const otg_allele* __restrict__ stg,
                                    uint32_t n_staged, const uint32_t* __restrict__ ref_len, uint32_t na_cap,
                                    uint32_t* __restrict__ src_of, uint32_t* __restrict__ seq_len, int32_t* __restrict__ smp)
{
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B || n_al[r] == 0) return;
  uint32_t dst = first[r];
  for (uint32_t s = 0; s < S; ++s) {
    const uint32_t c = cnt[(size_t)s * B + r], f = sfirst[(size_t)s * B + r];
    for (uint32_t k = 0; k < c; ++k, ++dst) {
      if (dst >= na_cap || f + k >= n_staged) continue;
      const uint32_t L = stg[f + k].seq_len;
      src_of[dst] = f + k;
      seq_len[dst] = L ? L : 1u;                     // a zero-length allele is read back as "N"
      smp[dst] = (int32_t)s;
    }
  }
  if (dst < na_cap) { src_of[dst] = REF_FLAG | r; seq_len[dst] = ref_len[r]; smp[dst] = (int32_t)S; }
}

__device__ __forceinline__ uint4 cohort_load16(const uint8_t* p) { uint4 v; __builtin_memcpy(&v, p, 16); return v; }

// ---- regroup 5: one wave per allele moves its bytes (16 per lane per step; the destination is brought to a 16-byte boundary first) and
// lane 0 writes its record in the regrouped order
__global__ void __launch_bounds__(256) cohort_gather_kernel(const uint32_t* __restrict__ src_of, const uint32_t* __restrict__ seq_len, const uint64_t* __restrict__ seq_off,
                                                            const int32_t* __restrict__ smp, uint32_t na, const otg_allele* __restrict__ stg,
                                                            const uint8_t* __restrict__ stg_seq, const uint8_t* __restrict__ ref_seq, const uint64_t* __restrict__ ref_off,
                                                            uint8_t* __restrict__ arena, otg_allele* __restrict__ meta)
{
  const uint32_t a = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (a >= na) return;
  const uint32_t src = src_of[a];
  uint32_t n = seq_len[a];
  const uint64_t off = seq_off[a];
  otg_allele rec;
  const uint8_t* s;
  if (src & REF_FLAG) {
    // ANALLELE(refseq): coverage 1 / 1 / 1, se 0, ic 1, no haplotag (src/genotype.cpp:101)
    const uint32_t r = src & ~REF_FLAG;
    rec.scov = 1; rec.acov = 1; rec.tcov = 1; rec.se = 0.0f; rec.ic = 1; rec.ps = -1; rec.hp = -1; rec.region = r;
    s = ref_seq + ref_off[r];
  } else {
    rec = stg[src];
    s = stg_seq + rec.seq_off;
    if (rec.seq_len == 0) {
      if (lane == 0) arena[off] = (uint8_t)'N';
      n = 0;
    }
  }
  uint8_t* d = arena + off;
  if (lane == 0) { rec.seq_off = off; rec.seq_len = seq_len[a]; rec.label = smp[a]; meta[a] = rec; }
  uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  if (head > n) head = n;
  if (lane < head) d[lane] = s[lane];
  s += head; d += head; n -= head;
  const uint32_t nvec = n >> 4;
  for (uint32_t i = lane; i < nvec; i += 64u) *reinterpret_cast<uint4*>(d + (size_t)i * 16u) = cohort_load16(s + (size_t)i * 16u);
  const uint32_t tail = n & 15u;
  if (lane < tail) d[(size_t)nvec * 16u + lane] = s[(size_t)nvec * 16u + lane];
}

// ---- rows 1: the rows of a region = the alleles of its VCF line: n_gt where it has alleles (scanned into row_first)
struct CohortRowCount {
  const uint32_t* n_al; const int32_t* ngt;
  __device__ __forceinline__ uint32_t operator()(uint32_t r) const
  {
    const uint32_t na = n_al[r];
    const int32_t g = ngt[r];
    return na == 0 || g <= 0 ? 0u : ((uint32_t)g < na ? (uint32_t)g : na);        // (there are never more clusters than alleles)
  }
};

// ---- rows 2: one thread per allele a, the i-th of its region r (meta[a].region).  With i < rows of r it writes row row_first[r] + i of the VCF
// line's column order (src/genotype.cpp:149-153, emit.hip): row 0 the reference allele — the last of the region, not reps[0] —, row i >= 1 the
// representative reps[i - 1] (i <= ref_gt) or reps[i].  As a sample's allele it writes the sample's GT numbers: inside a region the alleles are
// sample-major, so the first of a sample is the one whose predecessor has another sample (or that opens the region), its last the one whose
// successor has another sample (the reference allele, smp == S, closes every region): no atomics.
__global__ void __launch_bounds__(256) cohort_rows_kernel(const otg_allele* __restrict__ meta, const int32_t* __restrict__ smp, uint32_t na, uint32_t B, uint32_t S,
                                                          const uint32_t* __restrict__ first, const uint32_t* __restrict__ n_al, const int32_t* __restrict__ gt,
                                                          const int32_t* __restrict__ reps, const uint32_t* __restrict__ row_first,
                                                          const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ seq_len,
                                                          uint32_t* __restrict__ row_allele, uint64_t* __restrict__ row_off, uint32_t* __restrict__ row_len,
                                                          int32_t* __restrict__ sample_gt)
{
  const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= na) return;
  const uint32_t r = meta[a].region;
  if (r >= B) return;
  const uint32_t a0 = first[r], n = n_al[r];
  if (a < a0 || a - a0 >= n) return;
  const uint32_t i = a - a0, ref_i = n - 1u;
  const int32_t ref_gt = gt[a0 + ref_i];
  const uint32_t rows = row_first[r + 1] - row_first[r];
  if (i < rows) {
    uint32_t pick = ref_i;
    if (i > 0) {
      const int32_t rep = reps[a0 + ((int32_t)i <= ref_gt ? i - 1u : i)];
      pick = rep >= 0 && (uint32_t)rep < n ? (uint32_t)rep : ref_i;
    }
    const uint32_t row = row_first[r] + i, al = a0 + pick;
    row_allele[row] = al; row_off[row] = seq_off[al]; row_len[row] = seq_len[al];
  }
  const int32_t s = smp[a];
  if (s < 0 || (uint32_t)s >= S) return;                                  // the reference allele is nobody's genotype
  const int32_t g = gt[a];
  const int32_t g2 = g == ref_gt ? 0 : (g < ref_gt ? g + 1 : g);
  int32_t* out = sample_gt + ((size_t)r * S + (uint32_t)s) * 2u;
  if (i == 0 || smp[a - 1] != s) out[0] = g2;
  if (i + 1 >= n || smp[a + 1] != s) out[1] = g2;
}

Cohort* cohort_of(otg_ctx* ctx, const char* who)
{
  if (!ctx) { otg_fail(nullptr, OTG_ERR_NO_DEVICE, "%s: no context (no HIP device?)", who); return nullptr; }
  if (!ctx->cohort || !ctx->cohort->open) { otg_fail(ctx, OTG_ERR_ARG, "%s: no cohort batch is open on this context (otg_cohort_begin)", who); return nullptr; }
  return ctx->cohort;
}

// builds the row list once per clustering
int cohort_build_rows(otg_ctx* ctx, Cohort& c, const char* who)
{
  if (!c.clustered) return otg_fail(ctx, OTG_ERR_ARG, "%s: the batch has not been clustered (otg_cohort_genotype)", who);
  if (c.rows_built) return OTG_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t B = c.B, na = c.na;
  const size_t cells = (size_t)B * c.S * 2;
  int rc = OTG_OK;
  if ((rc = grow(ctx, c.row_first, ((size_t)B + 1) * 4)) || (rc = grow(ctx, c.row_allele, ((size_t)na + 1) * 4)) || (rc = grow(ctx, c.row_off, ((size_t)na + 1) * 8)) ||
      (rc = grow(ctx, c.row_len, ((size_t)na + 1) * 4)) || (rc = grow(ctx, c.sample_gt, cells * 4)))
    return rc;
  hipStream_t st = ctx->stream;
  c.n_rows = 0;
  HIP_TRY(ctx, hipMemsetAsync(c.row_first.p, 0, ((size_t)B + 1) * 4, st));
  if (cells) HIP_TRY(ctx, hipMemsetAsync(c.sample_gt.p, 0xff, cells * 4, st));          // -1: ./. and the regions without alleles
  if (B && na) {
    hipLaunchKernelGGL((otg_scan_kernel<uint32_t, uint32_t, CohortRowCount>), dim3(1), dim3(1024), 0, st, CohortRowCount{(const uint32_t*)c.n_al.p, (const int32_t*)c.ngt.p}, B,
                       (uint32_t*)c.row_first.p, (uint32_t*)nullptr);
    const int32_t* d_gt = (const int32_t*)c.gt.p;
    hipLaunchKernelGGL(cohort_rows_kernel, dim3((na + 255) / 256), dim3(256), 0, st, (const otg_allele*)c.meta.p, (const int32_t*)c.smp.p, na, B, c.S, (const uint32_t*)c.first.p,
                       (const uint32_t*)c.n_al.p, d_gt, d_gt + 3 * ((size_t)na + 1), (const uint32_t*)c.row_first.p, (const uint64_t*)c.seq_off.p, (const uint32_t*)c.seq_len.p,
                       (uint32_t*)c.row_allele.p, (uint64_t*)c.row_off.p, (uint32_t*)c.row_len.p, (int32_t*)c.sample_gt.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&c.n_rows, (const uint32_t*)c.row_first.p + B, 4, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (c.n_rows > na) return otg_fail(ctx, OTG_ERR_FATAL, "%s: %u rows of %u alleles", who, c.n_rows, na);
  c.rows_built = true;
  return OTG_OK;
}

// the row operators (otg_*_cohort): the open, clustered batch or the refusal; then, behind the operator's own argument check, rows
// [row_begin, row_begin + n) of it
int cohort_clustered(otg_ctx* ctx, const char* who, Cohort** out)
{
  Cohort* cp = cohort_of(ctx, who);
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  if (!cp->clustered) return otg_fail(ctx, OTG_ERR_ARG, "%s: the batch has not been clustered (otg_cohort_genotype)", who);
  *out = cp;
  return OTG_OK;
}
int cohort_rows(otg_ctx* ctx, Cohort& c, const char* who, uint32_t row_begin, uint32_t n, OtgRows* rows)
{
  if (int rc = cohort_build_rows(ctx, c, who)) return rc;
  if ((uint64_t)row_begin + n > c.n_rows) return otg_fail(ctx, OTG_ERR_ARG, "%s: rows %u .. %llu of %u", who, row_begin, (unsigned long long)row_begin + n, c.n_rows);
  *rows = OtgRows{(const uint8_t*)c.arena.p, (const uint64_t*)c.row_off.p + row_begin, (const uint32_t*)c.row_len.p + row_begin};
  return OTG_OK;
}

} // namespace

extern "C" {

int otg_cohort_begin(otg_ctx* ctx, uint32_t n_regions, uint32_t n_samples)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_cohort_begin: no context (no HIP device?)");
  if (n_samples == 0) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_begin: zero samples");
  if (n_regions >= REF_FLAG || (uint64_t)n_regions * n_samples > (1ull << 31)) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_begin: %u regions x %u samples is too large a batch", n_regions, n_samples);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->cohort) ctx->cohort = new Cohort();
  Cohort& c = *ctx->cohort;
  c.B = n_regions; c.S = n_samples;
  c.staged.assign(n_samples, 0);
  c.n_staged = 0; c.staged_bytes = 0; c.na = 0; c.seq_bytes = 0;
  c.regrouped = c.clustered = c.rows_built = false;
  const size_t cells = (size_t)n_regions * n_samples;
  if (int rc = grow(ctx, c.cnt, cells * 4)) return rc;
  if (int rc = grow(ctx, c.sfirst, cells * 4)) return rc;
  // a sample that is never staged, or whose run was empty, has no alleles
  HIP_TRY(ctx, hipMemsetAsync(c.cnt.p, 0, std::max<size_t>(cells * 4, 16), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(c.sfirst.p, 0, std::max<size_t>(cells * 4, 16), ctx->stream));
  c.open = true;
  return OTG_OK;
}

int otg_cohort_stage(otg_ctx* ctx, otg_ctx* src_ctx, uint32_t sample)
{
  Cohort* cp = cohort_of(ctx, "otg_cohort_stage");
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  Cohort& c = *cp;
  if (!src_ctx) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_stage: no source context");
  if (src_ctx->device != ctx->device) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_stage: the source context is on device %d, the cohort on device %d", src_ctx->device, ctx->device);
  if (sample >= c.S) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_stage: sample %u of %u", sample, c.S);
  if (c.staged[sample]) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_stage: sample %u is staged already", sample);
  if (c.regrouped) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_stage: the batch has been regrouped already");
  const int64_t run_regions = otg_pipeline_run_regions(src_ctx);
  if (run_regions < 0) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_stage: the source context has no completed otg_assemble_run");
  if ((uint64_t)run_regions != c.B) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_stage: the run of sample %u has %lld regions, the cohort batch %u", sample, (long long)run_regions, c.B);
  uint32_t na = 0; uint64_t sb = 0;
  const otg_region_result* d_rr = nullptr; const otg_allele* d_al = nullptr; const uint8_t* d_seq = nullptr;
  if (otg_assemble_result_sizes(src_ctx, &na, &sb) != OTG_OK || otg_assemble_device_results(src_ctx, &d_rr, &d_al, &d_seq) != OTG_OK)      // synchronises the run's stream
    return otg_fail(ctx, OTG_ERR_HIP, "otg_cohort_stage: %s", otg_last_error(src_ctx));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  c.staged[sample] = 1;
  if (!d_rr || !d_al || na == 0 || c.B == 0) return OTG_OK;                   // an empty run: its row of the table stays zero
  if (c.n_staged + na >= REF_FLAG) return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_cohort_stage: more than 2^31 staged alleles");
  if (int rc = grow(ctx, c.stg_al, (size_t)(c.n_staged + na) * sizeof(otg_allele), (size_t)c.n_staged * sizeof(otg_allele))) return rc;
  if (int rc = grow(ctx, c.stg_seq, (size_t)(c.staged_bytes + sb) + 64, (size_t)c.staged_bytes)) return rc;
  if (sb && d_seq) HIP_TRY(ctx, hipMemcpyAsync((uint8_t*)c.stg_seq.p + c.staged_bytes, d_seq, sb, hipMemcpyDeviceToDevice, ctx->stream));
  const uint32_t n = std::max<uint32_t>(na, c.B);
  hipLaunchKernelGGL(cohort_stage_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_rr, d_al, c.B, na, sample, (uint32_t)c.n_staged, c.staged_bytes,
                     (otg_allele*)c.stg_al.p, (uint32_t*)c.cnt.p + (size_t)sample * c.B, (uint32_t*)c.sfirst.p + (size_t)sample * c.B);
  HIP_TRY(ctx, hipGetLastError());
  // the source context is free to run its next batch once this returns
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  c.n_staged += na; c.staged_bytes += sb;
  return OTG_OK;
}

int otg_cohort_regroup(otg_ctx* ctx, const uint8_t* ref_arena, uint64_t ref_bytes, const uint64_t* ref_off, const uint32_t* ref_len)
{
  Cohort* cp = cohort_of(ctx, "otg_cohort_regroup");
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  Cohort& c = *cp;
  if (c.B && (!ref_off || !ref_len || (ref_bytes && !ref_arena))) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_regroup: NULL argument");
  for (uint32_t s = 0; s < c.S; ++s) if (!c.staged[s]) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_regroup: sample %u has not been staged", s);
  uint64_t ref_total = 0;
  for (uint32_t r = 0; r < c.B; ++r) {
    if (ref_off[r] + ref_len[r] > ref_bytes) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_regroup: reference allele of region %u outside the arena", r);
    ref_total += ref_len[r];
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  c.regrouped = c.clustered = c.rows_built = false;
  const uint32_t B = c.B;
  c.h_first.assign((size_t)B + 1, 0); c.h_n_al.assign(B, 0); c.h_pair_off.assign((size_t)B + 1, 0);
  c.na = 0; c.seq_bytes = 0;
  if (B == 0) { c.regrouped = true; return OTG_OK; }
  // upper bounds known on the host: every staged allele once (a zero-length one grows to one byte), one reference allele per region
  const uint64_t na_cap = c.n_staged + B, bytes_cap = c.staged_bytes + c.n_staged + ref_total;
  if (na_cap >= REF_FLAG) return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_cohort_regroup: more than 2^31 alleles");
  int rc = OTG_OK;
  if ((rc = grow(ctx, c.ref_seq, ref_bytes + 64)) || (rc = grow(ctx, c.ref_off, (size_t)B * 8)) || (rc = grow(ctx, c.ref_len, (size_t)B * 4)) ||
      (rc = grow(ctx, c.n_al, (size_t)B * 4)) || (rc = grow(ctx, c.first, ((size_t)B + 1) * 4)) || (rc = grow(ctx, c.pairs, (size_t)B * 8)) ||
      (rc = grow(ctx, c.pair_off, ((size_t)B + 1) * 8)) || (rc = grow(ctx, c.src_of, (na_cap + 1) * 4)) || (rc = grow(ctx, c.seq_len, (na_cap + 1) * 4)) ||
      (rc = grow(ctx, c.seq_off, (na_cap + 2) * 8)) || (rc = grow(ctx, c.smp, (na_cap + 1) * 4)) || (rc = grow(ctx, c.meta, (na_cap + 1) * sizeof(otg_allele))) ||
      (rc = grow(ctx, c.arena, bytes_cap + 128)) || (rc = grow(ctx, c.stg_al, 64)) || (rc = grow(ctx, c.stg_seq, 64)))
    return rc;
  hipStream_t st = ctx->stream;
  if (ref_bytes) HIP_TRY(ctx, hipMemcpyAsync(c.ref_seq.p, ref_arena, ref_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(c.ref_off.p, ref_off, (size_t)B * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(c.ref_len.p, ref_len, (size_t)B * 4, hipMemcpyHostToDevice, st));
  // Invariant: the regrouped arena ends in 128 zeroed bytes.  The k-mer tiers (kmer_usage.hip, ku_segment) read up to 32 bytes past an allele's
  // last window, the clustering up to 64; past the last allele those reads stay inside this allocation and see zeros.
  HIP_TRY(ctx, hipMemsetAsync(c.arena.p, 0, bytes_cap + 128, st));
  HIP_TRY(ctx, hipMemsetAsync(c.seq_len.p, 0, (na_cap + 1) * 4, st));
  HIP_TRY(ctx, hipMemsetAsync(c.src_of.p, 0, (na_cap + 1) * 4, st));
  const dim3 gB((B + 255) / 256), b256(256);
  hipLaunchKernelGGL(cohort_region_counts_kernel, gB, b256, 0, st, (const uint32_t*)c.cnt.p, B, c.S, (uint32_t*)c.n_al.p, (uint64_t*)c.pairs.p);
  hipLaunchKernelGGL((otg_scan_kernel<uint32_t, uint32_t, OtgScanPtr<uint32_t>>), dim3(1), dim3(1024), 0, st, OtgScanPtr<uint32_t>{(const uint32_t*)c.n_al.p}, B, (uint32_t*)c.first.p, (uint32_t*)nullptr);
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, OtgScanPtr<uint64_t>>), dim3(1), dim3(1024), 0, st, OtgScanPtr<uint64_t>{(const uint64_t*)c.pairs.p}, B, (uint64_t*)c.pair_off.p, (uint64_t*)nullptr);
  hipLaunchKernelGGL(cohort_place_kernel, gB, b256, 0, st, (const uint32_t*)c.cnt.p, (const uint32_t*)c.sfirst.p, B, c.S, (const uint32_t*)c.first.p,
                     (const uint32_t*)c.n_al.p, (const otg_allele*)c.stg_al.p, (uint32_t)c.n_staged, (const uint32_t*)c.ref_len.p, (uint32_t)na_cap,
                     (uint32_t*)c.src_of.p, (uint32_t*)c.seq_len.p, (int32_t*)c.smp.p);
  HIP_TRY(ctx, hipGetLastError());
  // what the host needs for the launch of the clustering: alleles per region (wide routing) and the pair offsets (workspace size)
  HIP_TRY(ctx, hipMemcpyAsync(c.h_first.data(), c.first.p, ((size_t)B + 1) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(c.h_pair_off.data(), c.pair_off.p, ((size_t)B + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const uint32_t na = c.h_first[B];
  if (na > na_cap) return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_cohort_regroup: %u alleles regrouped, %llu staged", na, (unsigned long long)na_cap);
  for (uint32_t r = 0; r < B; ++r) c.h_n_al[r] = c.h_first[r + 1] - c.h_first[r];
  hipLaunchKernelGGL((otg_scan_kernel<uint64_t, uint64_t, OtgScanPtr<uint32_t>>), dim3(1), dim3(1024), 0, st, OtgScanPtr<uint32_t>{(const uint32_t*)c.seq_len.p}, na, (uint64_t*)c.seq_off.p, (uint64_t*)nullptr);
  if (na)
    hipLaunchKernelGGL(cohort_gather_kernel, dim3((na + 3) / 4), dim3(256), 0, st, (const uint32_t*)c.src_of.p, (const uint32_t*)c.seq_len.p, (const uint64_t*)c.seq_off.p,
                       (const int32_t*)c.smp.p, na, (const otg_allele*)c.stg_al.p, (const uint8_t*)c.stg_seq.p, (const uint8_t*)c.ref_seq.p, (const uint64_t*)c.ref_off.p,
                       (uint8_t*)c.arena.p, (otg_allele*)c.meta.p);
  HIP_TRY(ctx, hipGetLastError());
  uint64_t total = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&total, (const uint64_t*)c.seq_off.p + na, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (total > bytes_cap) return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_cohort_regroup: %llu allele bytes regrouped, room for %llu", (unsigned long long)total, (unsigned long long)bytes_cap);
  c.na = na; c.seq_bytes = total;
  c.regrouped = true;
  return OTG_OK;
}

int otg_cohort_genotype(otg_ctx* ctx, const otg_params* params) { return otg_genotype_cohort_metric(ctx, params, OTG_GT_METRIC_LENGTH); }

int otg_genotype_cohort_metric(otg_ctx* ctx, const otg_params* params, int32_t metric)
{
  Cohort* cp = cohort_of(ctx, "otg_cohort_genotype");
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  Cohort& c = *cp;
  if (!params) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_genotype: NULL argument");
  if (!c.regrouped) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_genotype: the batch has not been regrouped (otg_cohort_regroup)");
  if (int rc0 = otg_genotype_metric_fits(ctx, "otg_cohort_genotype", metric, c.B ? c.h_pair_off[c.B] : 0)) return rc0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  c.clustered = c.rows_built = false;
  const uint32_t B = c.B;
  const uint64_t na = c.na;
  int rc = OTG_OK;
  if ((rc = grow(ctx, c.gt, (na + 1) * 4 * 4)) || (rc = grow(ctx, c.hsd, (na + 1) * 8)) || (rc = grow(ctx, c.ngt, (size_t)(B + 1) * 2 * 4))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(c.ngt.p, 0, (size_t)(B + 1) * 2 * 4, ctx->stream));
  if (B && na) {
    uint32_t max_len = 0;      // the edit chain sizes its last tier from the longest sequence: the lengths exist on the device only
    if (metric == OTG_GT_METRIC_EDIT && (rc = otg_device_max_u32(ctx, (const uint32_t*)c.seq_len.p, na, &max_len))) return rc;
    rc = otg_genotype_resident(ctx, params, (const uint8_t*)c.arena.p, (const uint64_t*)c.seq_off.p, (const uint32_t*)c.seq_len.p, (const uint32_t*)c.first.p,
                               (const uint32_t*)c.n_al.p, c.h_n_al.data(), B, (const uint64_t*)c.pair_off.p, c.h_pair_off[B], na, (int32_t*)c.gt.p,
                               (double*)c.hsd.p, (int32_t*)c.ngt.p, nullptr, metric, max_len);
    if (rc) return rc;
    std::vector<int32_t> h_err(B);
    HIP_TRY(ctx, hipMemcpyAsync(h_err.data(), (const int32_t*)c.ngt.p + B, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = otg_genotype_metric_finish(ctx, metric, nullptr))) return rc;
    for (uint32_t r = 0; r < B; ++r)
      if (h_err[r]) return otg_fail(ctx, OTG_ERR_CAPACITY, "region %u: %u alleles, more than the clustering workspace was sized for", r, c.h_n_al[r]);
  } else HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  c.clustered = true;
  return OTG_OK;
}

int otg_cohort_result_sizes(otg_ctx* ctx, uint32_t* n_alleles, uint64_t* seq_bytes)
{
  Cohort* cp = cohort_of(ctx, "otg_cohort_result_sizes");
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  if (!cp->regrouped) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_result_sizes: the batch has not been regrouped");
  if (n_alleles) *n_alleles = cp->na;
  if (seq_bytes) *seq_bytes = cp->seq_bytes;
  return OTG_OK;
}

int otg_cohort_collect(otg_ctx* ctx, uint32_t* first_allele_out, otg_allele* alleles_out, uint32_t allele_capacity, int32_t* sample_out,
                       uint64_t* seq_off_out, uint32_t* seq_len_out, uint8_t* seq_out, uint64_t seq_capacity,
                       int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out, int32_t* n_gt_out, int32_t* reps_out)
{
  Cohort* cp = cohort_of(ctx, "otg_cohort_collect");
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  Cohort& c = *cp;
  if (!c.regrouped) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_collect: the batch has not been regrouped");
  const bool want_gt = gt_out || gt_l_out || gt_k_out || hsd_out || n_gt_out || reps_out;
  if (want_gt && !c.clustered) return otg_fail(ctx, OTG_ERR_ARG, "otg_cohort_collect: the batch has not been clustered (otg_cohort_genotype)");
  const uint64_t na = c.na;
  if (((alleles_out || sample_out || seq_off_out || seq_len_out || gt_out || gt_l_out || gt_k_out || hsd_out || reps_out) && allele_capacity < na) ||
      (seq_out && seq_capacity < c.seq_bytes))
    return otg_fail(ctx, OTG_ERR_CAPACITY, "otg_cohort_collect: output buffers too small (%u alleles, %llu bytes)", c.na, (unsigned long long)c.seq_bytes);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (first_allele_out) memcpy(first_allele_out, c.h_first.data(), ((size_t)c.B + 1) * 4);
  if (n_gt_out && c.B) HIP_TRY(ctx, hipMemcpyAsync(n_gt_out, c.ngt.p, (size_t)c.B * 4, hipMemcpyDeviceToHost, st));
  if (na) {
    if (alleles_out) HIP_TRY(ctx, hipMemcpyAsync(alleles_out, c.meta.p, na * sizeof(otg_allele), hipMemcpyDeviceToHost, st));
    if (sample_out) HIP_TRY(ctx, hipMemcpyAsync(sample_out, c.smp.p, na * 4, hipMemcpyDeviceToHost, st));
    if (seq_off_out) HIP_TRY(ctx, hipMemcpyAsync(seq_off_out, c.seq_off.p, na * 8, hipMemcpyDeviceToHost, st));
    if (seq_len_out) HIP_TRY(ctx, hipMemcpyAsync(seq_len_out, c.seq_len.p, na * 4, hipMemcpyDeviceToHost, st));
    if (seq_out && c.seq_bytes) HIP_TRY(ctx, hipMemcpyAsync(seq_out, c.arena.p, c.seq_bytes, hipMemcpyDeviceToHost, st));
    const int32_t* d_gt = (const int32_t*)c.gt.p;
    if (gt_out) HIP_TRY(ctx, hipMemcpyAsync(gt_out, d_gt, na * 4, hipMemcpyDeviceToHost, st));
    if (gt_l_out) HIP_TRY(ctx, hipMemcpyAsync(gt_l_out, d_gt + (na + 1), na * 4, hipMemcpyDeviceToHost, st));
    if (gt_k_out) HIP_TRY(ctx, hipMemcpyAsync(gt_k_out, d_gt + 2 * (na + 1), na * 4, hipMemcpyDeviceToHost, st));
    if (reps_out) HIP_TRY(ctx, hipMemcpyAsync(reps_out, d_gt + 3 * (na + 1), na * 4, hipMemcpyDeviceToHost, st));
    if (hsd_out) HIP_TRY(ctx, hipMemcpyAsync(hsd_out, c.hsd.p, na * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OTG_OK;
}

int otg_kmer_cohort_rows(otg_ctx* ctx, uint32_t* n_rows, uint32_t* row_first_out, uint32_t* row_allele_out, int32_t* sample_gt_out)
{
  Cohort* cp = cohort_of(ctx, "otg_kmer_cohort_rows");
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  Cohort& c = *cp;
  if (int rc = cohort_build_rows(ctx, c, "otg_kmer_cohort_rows")) return rc;
  if (n_rows) *n_rows = c.n_rows;
  hipStream_t st = ctx->stream;
  const size_t cells = (size_t)c.B * c.S * 2;
  if (row_first_out) HIP_TRY(ctx, hipMemcpyAsync(row_first_out, c.row_first.p, ((size_t)c.B + 1) * 4, hipMemcpyDeviceToHost, st));
  if (row_allele_out && c.n_rows) HIP_TRY(ctx, hipMemcpyAsync(row_allele_out, c.row_allele.p, (size_t)c.n_rows * 4, hipMemcpyDeviceToHost, st));
  if (sample_gt_out && cells) HIP_TRY(ctx, hipMemcpyAsync(sample_gt_out, c.sample_gt.p, cells * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OTG_OK;
}

int otg_kmer_cohort_device_rows(otg_ctx* ctx, uint32_t* n_rows, const uint32_t** row_first, const uint32_t** row_allele, const int32_t** sample_gt)
{
  Cohort* cp = cohort_of(ctx, "otg_kmer_cohort_device_rows");
  if (!cp) return ctx ? OTG_ERR_ARG : OTG_ERR_NO_DEVICE;
  Cohort& c = *cp;
  if (int rc = cohort_build_rows(ctx, c, "otg_kmer_cohort_device_rows")) return rc;
  if (n_rows) *n_rows = c.n_rows;
  if (row_first) *row_first = (const uint32_t*)c.row_first.p;
  if (row_allele) *row_allele = (const uint32_t*)c.row_allele.p;
  if (sample_gt) *sample_gt = (const int32_t*)c.sample_gt.p;
  return OTG_OK;
}

int otg_kmer_cohort_usage(otg_ctx* ctx, int32_t k, uint32_t row_begin, uint32_t n, double* usage_out, double* gc_out, double* hsd_out)
{
  Cohort* c = nullptr;
  OtgRows rows;
  if (int rc = cohort_clustered(ctx, "otg_kmer_cohort_usage", &c)) return rc;
  if (k < 1 || k > OTG_KMER_MAX) return otg_fail(ctx, OTG_ERR_ARG, "otg_kmer_cohort_usage: k = %d outside 1..%d", k, OTG_KMER_MAX);
  if (int rc = cohort_rows(ctx, *c, "otg_kmer_cohort_usage", row_begin, n, &rows)) return rc;
  if (int rc = otg_kmer_usage_fits(ctx, "otg_kmer_cohort_usage", n, k)) return rc;
  return otg_kmer_usage_resident(ctx, "otg_kmer_cohort_usage", rows, nullptr, n, k, usage_out, gc_out, hsd_out);
}

int otg_motif_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, uint32_t max_period, uint32_t slack, otg_motif* out, uint8_t* unit_out, uint32_t unit_stride)
{
  Cohort* c = nullptr;
  OtgRows rows;
  if (int rc = cohort_clustered(ctx, "otg_motif_cohort", &c)) return rc;
  if (int rc = otg_motif_args(ctx, "otg_motif_cohort", max_period, slack)) return rc;
  if (int rc = cohort_rows(ctx, *c, "otg_motif_cohort", row_begin, n, &rows)) return rc;
  uint32_t max_len = 0;      // the row lengths exist on the device only
  if (n)
    if (int rc = otg_device_max_u32(ctx, rows.len, n, &max_len)) return rc;
  if (int rc = otg_motif_stride_fits(ctx, "otg_motif_cohort", max_len, max_period, unit_stride)) return rc;
  return otg_motif_resident(ctx, "otg_motif_cohort", rows, n, max_period, slack, out, unit_out, unit_stride);
}

int otg_repeat_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, uint32_t max_period, uint32_t min_copies, uint32_t min_span, otg_repeat_sum* sums,
                      uint64_t* seg_off, uint64_t* n_segments)
{
  Cohort* c = nullptr;
  OtgRows rows;
  if (int rc = cohort_clustered(ctx, "otg_repeat_cohort", &c)) return rc;
  if (int rc = otg_repeat_args(ctx, "otg_repeat_cohort", max_period, min_copies, min_span)) return rc;
  if (int rc = cohort_rows(ctx, *c, "otg_repeat_cohort", row_begin, n, &rows)) return rc;
  return otg_repeat_resident(ctx, "otg_repeat_cohort", rows, n, max_period, min_copies, min_span, sums, seg_off, n_segments);
}

int otg_unitalign_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                         const uint32_t* unit_len, uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks, otg_unitalign* out)
{
  Cohort* c = nullptr;
  OtgRows rows;
  if (int rc = cohort_clustered(ctx, "otg_unitalign_cohort", &c)) return rc;
  if (int rc = cohort_rows(ctx, *c, "otg_unitalign_cohort", row_begin, n, &rows)) return rc;
  if (!unit_arena && !n_units) {                                   // the units of the latest otg_motif_cohort, which stay where they are
    if (ctx->last_motif_n == 0 || ctx->last_motif_rows.arena != rows.arena || ctx->last_motif_rows.off != rows.off || ctx->last_motif_n != n)
      return otg_fail(ctx, OTG_ERR_ARG, "otg_unitalign_cohort: the latest motif call on this context was not otg_motif_cohort over rows %u .. %llu", row_begin,
                      (unsigned long long)row_begin + n);
    return otg_unitalign_motifs(ctx, out);
  }
  if (int rc = otg_unitalign_check(ctx, "otg_unitalign_cohort", n, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks)) return rc;
  ctx->last_unitalign_ms = 0.0; ctx->last_unitalign_n = 0;
  if (n_tasks == 0) return OTG_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  OtgUnitSource units;
  const uint32_t *d_ts = nullptr, *d_tu = nullptr;
  if (int rc = otg_unitalign_upload(ctx, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks, &units, &d_ts, &d_tu)) return rc;
  return otg_unitalign_resident(ctx, "otg_unitalign_cohort", rows, units, d_ts, d_tu, n_tasks, out);
}

int otg_tract_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                     const uint32_t* unit_len, uint32_t n_units, const uint32_t* task_seq, const uint32_t* task_unit, uint32_t n_tasks,
                     const otg_tract_params* params, otg_tract* out)
{
  Cohort* c = nullptr;
  OtgRows rows;
  otg_tract_params q;
  if (int rc = cohort_clustered(ctx, "otg_tract_cohort", &c)) return rc;
  if (int rc = otg_tract_args(ctx, "otg_tract_cohort", params, &q)) return rc;
  if (int rc = cohort_rows(ctx, *c, "otg_tract_cohort", row_begin, n, &rows)) return rc;
  if (!unit_arena && !n_units) {                                   // the units of the latest otg_motif_cohort, which stay where they are
    if (ctx->last_motif_n == 0 || ctx->last_motif_rows.arena != rows.arena || ctx->last_motif_rows.off != rows.off || ctx->last_motif_n != n)
      return otg_fail(ctx, OTG_ERR_ARG, "otg_tract_cohort: the latest motif call on this context was not otg_motif_cohort over rows %u .. %llu", row_begin,
                      (unsigned long long)row_begin + n);
    return otg_tract_motifs(ctx, &q, out);
  }
  if (int rc = otg_unitalign_check(ctx, "otg_tract_cohort", n, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks)) return rc;
  if (n_tasks == 0) return otg_tract_resident(ctx, "otg_tract_cohort", rows, OtgUnitSource{nullptr, nullptr, nullptr, nullptr, 0u}, nullptr, nullptr, 0, q, out);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  OtgUnitSource units;
  const uint32_t *d_ts = nullptr, *d_tu = nullptr;
  if (int rc = otg_unitalign_upload(ctx, unit_arena, unit_bytes, unit_off, unit_len, n_units, task_seq, task_unit, n_tasks, &units, &d_ts, &d_tu, SLOT_TRACT_UNITS)) return rc;
  return otg_tract_resident(ctx, "otg_tract_cohort", rows, units, d_ts, d_tu, n_tasks, q, out);
}

int otg_unitparse_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                         const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                         const uint32_t* task_set, uint32_t n_tasks, otg_unitparse_sum* sums, uint64_t* seg_off, uint64_t* n_segments)
{
  Cohort* c = nullptr;
  OtgRows rows;
  if (int rc = cohort_clustered(ctx, "otg_unitparse_cohort", &c)) return rc;
  if (int rc = cohort_rows(ctx, *c, "otg_unitparse_cohort", row_begin, n, &rows)) return rc;
  if (int rc = otg_unitparse_check(ctx, "otg_unitparse_cohort", n, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set, n_tasks))
    return rc;
  return otg_unitparse_resident(ctx, "otg_unitparse_cohort", rows, nullptr, n, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set,
                                n_tasks, sums, seg_off, n_segments);
}

int otg_locus_cohort(otg_ctx* ctx, uint32_t row_begin, uint32_t n, const uint8_t* unit_arena, uint64_t unit_bytes, const uint64_t* unit_off,
                     const uint32_t* unit_len, uint32_t n_units, const uint64_t* set_first, uint32_t n_sets, const uint32_t* task_seq,
                     const uint32_t* task_set, uint32_t n_tasks, const otg_tract_params* params, otg_locus* out, uint64_t* seg_off, uint64_t* n_segments)
{
  Cohort* c = nullptr;
  OtgRows rows;
  otg_tract_params q;
  if (int rc = cohort_clustered(ctx, "otg_locus_cohort", &c)) return rc;
  if (int rc = otg_tract_args(ctx, "otg_locus_cohort", params, &q)) return rc;
  if (int rc = cohort_rows(ctx, *c, "otg_locus_cohort", row_begin, n, &rows)) return rc;
  if (int rc = otg_unitparse_check(ctx, "otg_locus_cohort", n, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set, n_tasks))
    return rc;
  return otg_locus_resident(ctx, "otg_locus_cohort", rows, nullptr, n, unit_arena, unit_bytes, unit_off, unit_len, n_units, set_first, n_sets, task_seq, task_set, n_tasks,
                            q, out, seg_off, n_segments);
}

int otg_cohort_end(otg_ctx* ctx)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_cohort_end: no context");
  if (ctx->cohort) { ctx->cohort->open = false; ctx->cohort->regrouped = ctx->cohort->clustered = ctx->cohort->rows_built = false; }      // the buffers stay for the next batch (otg_destroy frees them)
  return OTG_OK;
}

} // extern "C"

// unitalign.hip: do the rows a motif call read at d_arena still lie there?
bool otg_cohort_holds_rows(otg_ctx* ctx, const uint8_t* d_arena)
{
  const Cohort* c = ctx ? ctx->cohort : nullptr;
  return c && c->open && c->clustered && c->rows_built && d_arena && (const uint8_t*)c->arena.p == d_arena;
}

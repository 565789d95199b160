// dispatch.hip — the per-region dispatcher of `otter assemble` as host code of the library.
//
// Reference: assemble() / assemble_process() (src/assemble.cpp:39-179) with BS::thread_pool::parallelize_loop
// (src/BS_thread_pool.hpp:175-200): the BED list is cut into contiguous blocks, one per worker thread; every worker opens its own BAM /
// FASTA handle, walks its block region by region (ingest -> the five hot-path calls -> emit under a mutex).
//
// Here a worker is a GPU.  The BED list is cut into one contiguous shard per device (the same static split), and every shard is cut into
// bounded BATCHES of regions that flow through three stages running concurrently on host threads:
//     ingest (otg_ingest_regions on T host threads, + reference flanks with -r)          -> queue (depth 2)
//     hot path (otg_assemble_submit / run / collect; two contexts per device, so the upload of batch k+1 overlaps the kernels of batch k)
//     emit (otg_emit_alleles / otg_emit_reads) + the caller's write callback, strictly in BED order
// Memory is bounded by the batch size, not by the BED file; output order is the BED order whatever the number of devices or batches
// (the reference's order with -t 1; with -t > 1 the reference prints in completion order).
#include "otg_common.hpp"
#include "otg_compare.hpp"
#include "otg_dispatch_queue.hpp"
#include "otg_vcf2mat.hpp"
#include "otg_motif.hpp"
#include "otg_repeat.hpp"
#include "otg_unitalign.hpp"
#include "otg_locus.hpp"
#include "otg_unitset.hpp"
#include "otg_spread.hpp"
#include "otg_tract.hpp"
#include "otg_unitparse.hpp"
#include "otg_unitparse_core.hpp"
#include <cmath>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>

namespace {

// The two large buffers of a batch — read sequences and read table — are plain uninitialised memory: a std::vector would zero-fill its
// ~200 KB per region on the ingest thread before the readers overwrite it (measured: a fresh batch of 1 000 regions was ingested in 66 ms,
// a recycled one in 32), while pages touched first by the readers themselves are mapped by 16 threads side by side.
template <class T> struct HostBuf {
  T* p = nullptr; size_t n = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { free(p); }
  T* data() { return p; }
  const T* data() const { return p; }
  size_t size() const { return n; }
  // at least `want` elements; the first `keep` stay what they were, the rest is undefined
  void resize(size_t want, size_t keep = 0) {
    if (want <= n) return;
    T* q = (T*)malloc(want * sizeof(T));
    if (!q) throw std::bad_alloc();
    if (keep && p) memcpy(q, p, std::min(keep, n) * sizeof(T));
    free(p);
    p = q; n = want;
  }
};

struct Batch {
  uint32_t index = 0;                   // batch number inside its shard
  uint32_t first = 0, n = 0;            // BED range [first, first + n)
  HostBuf<uint8_t> arena;
  HostBuf<otg_read> reads;
  std::vector<otg_region> regions;
  std::vector<otg_read_meta> meta;      // --reads-only
  std::vector<char> names;
  uint64_t arena_used = 0;
  uint32_t n_reads = 0;
  std::string text;                     // emitted records
};

using BatchPtr = std::unique_ptr<Batch>;
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
// OTG_DISPATCH_TRACE=1: one stderr line per stage of every batch (milliseconds since the job started) — the host-side timeline of a job
const bool g_trace = getenv("OTG_DISPATCH_TRACE") != nullptr;
Clock::time_point g_trace_t0;
void trace(const char* what, uint32_t batch, uint32_t n, Clock::time_point from)
{
  if (!g_trace) return;
  fprintf(stderr, "[otg trace] %-8s batch %3u (%5u regions) %9.2f -> %9.2f ms\n", what, batch, n, std::chrono::duration<double, std::milli>(from - g_trace_t0).count(), ms_since(g_trace_t0));
}

// What the threads of one job share: its status — the first failure wins, everybody else sees rc != OTG_OK and stops — and its statistics.
struct Job {
  std::atomic<int> rc{OTG_OK};
  std::mutex err_m;
  std::string err;
  // statistics (summed over threads)
  std::mutex st_m;
  otg_job_stats st{};
  void fail(int code, const std::string& what) {
    int expected = OTG_OK;
    if (rc.compare_exchange_strong(expected, code)) { std::lock_guard<std::mutex> lk(err_m); err = what; }
  }
};

std::string last_err() { const char* e = otg_last_error(nullptr); return e ? std::string(e) : std::string(); }
std::string ctx_err(otg_ctx* ctx) { const char* e = otg_last_error(ctx); return e ? std::string(e) : std::string(); }

// Contexts survive the job: a fresh context pays for its first launches (page mapping of newly allocated workspaces, ~0.2-1 s), so a process
// that runs several jobs — or bench.py's repeated file-to-text leg — keeps them in a pool; otg_assemble_files_release() empties it.
std::mutex g_pool_m;
std::vector<std::pair<int, otg_ctx*>> g_pool;
otg_ctx* pool_acquire(int device)
{
  {
    std::lock_guard<std::mutex> lk(g_pool_m);
    for (size_t i = 0; i < g_pool.size(); ++i) if (g_pool[i].first == device) { otg_ctx* c = g_pool[i].second; g_pool.erase(g_pool.begin() + (long)i); return c; }
  }
  otg_ctx* c = nullptr;
  return otg_create(device, &c) == OTG_OK ? c : nullptr;
}
void pool_release(int device, otg_ctx* c) { std::lock_guard<std::mutex> lk(g_pool_m); g_pool.emplace_back(device, c); }

int dispatch_contexts()
{
  const char* e = getenv("OTG_DISPATCH_CONTEXTS");
  const int v = e ? atoi(e) : 2;
  return v < 1 ? 1 : (v > 4 ? 4 : v);
}
// End of a job: the pool keeps what ONE shard per device needs for the next job and destroys the rest — contexts hold multi-gigabyte aligner
// workspaces, and a caller that creates its own otg_ctx afterwards is budgeted against what is left of the device.
void pool_trim()
{
  std::lock_guard<std::mutex> lk(g_pool_m);
  const int keep = dispatch_contexts();
  std::map<int, int> seen;
  std::vector<std::pair<int, otg_ctx*>> kept;
  for (auto& p : g_pool) {
    if (++seen[p.first] <= keep) kept.push_back(p);
    else otg_destroy(p.second);
  }
  g_pool.swap(kept);
}

// Owners: a file handle closes, a pooled context goes back to the pool, when its owner leaves scope — on every path out of an entry point.
// An entry point declares them BEFORE its batch buffers and its TwoInFlight, so that the prefetch thread, which reads the handles, is joined
// first and the handles are closed after.
struct BamClose { void operator()(otg_bam* b) const { otg_bam_close(b); } };
struct FastaClose { void operator()(otg_fasta* f) const { otg_fasta_close(f); } };
struct VcfClose { void operator()(otg_vcf* v) const { otg_vcf_close(v); } };
struct PoolReturn { int device; void operator()(otg_ctx* c) const { pool_release(device, c); } };
using BamPtr = std::unique_ptr<otg_bam, BamClose>;
using FastaPtr = std::unique_ptr<otg_fasta, FastaClose>;
using VcfPtr = std::unique_ptr<otg_vcf, VcfClose>;
using PooledCtx = std::unique_ptr<otg_ctx, PoolReturn>;
// open(path, &raw) of the C interface into an owner; the owner stays empty when the call fails
template <class Ptr, class Open> int open_into(Ptr& out, Open open, const char* path)
{
  typename Ptr::pointer raw = nullptr;
  const int rc = open(path, &raw);
  out.reset(raw);
  return rc;
}
int open_bam(const char* path, BamPtr& out) { return open_into(out, otg_bam_open, path); }
int open_fasta(const char* path, FastaPtr& out) { return open_into(out, otg_fasta_open, path); }
int open_vcf(const char* path, VcfPtr& out) { return open_into(out, otg_vcf_open, path); }
PooledCtx acquire_ctx(int device) { return PooledCtx(pool_acquire(device), PoolReturn{device}); }

// The regions of a job: the BED records and the arena their chromosome names point into.
struct Bed { std::vector<otg_bed> beds; std::vector<char> chr_arena; };
int load_bed(const char* path, Bed& B)
{
  // size protocol: the first call reports the needed sizes
  uint32_t n = 0, skipped = 0; uint64_t cu = 0;
  int rc = otg_parse_bed_file(path, nullptr, 0, &n, nullptr, 0, &cu, &skipped);
  if (rc != OTG_OK && rc != OTG_ERR_CAPACITY) return rc;
  B.beds.resize((size_t)n + 1); B.chr_arena.resize((size_t)cu + 16);
  rc = otg_parse_bed_file(path, B.beds.data(), (uint32_t)B.beds.size(), &n, B.chr_arena.data(), B.chr_arena.size(), &cu, &skipped);
  if (rc != OTG_OK) return rc;
  B.beds.resize(n);
  return OTG_OK;
}

// The size protocol of the emitters: call(buf, cap, &need) with no buffer reports the size (OTG_ERR_CAPACITY from that call is not an
// error), `out` takes that size, and the second call fills it.
template <class Call> int sized_text(std::string& out, Call call)
{
  uint64_t need = 0;
  int rc = call((char*)nullptr, (uint64_t)0, &need);
  if (rc != OTG_OK && rc != OTG_ERR_CAPACITY) return rc;
  out.resize(need);
  return call(need ? &out[0] : nullptr, need, &need);
}

// SAM header of the allele records of one read group (src/assemble.cpp:167-177), its @SQ lines from the BAM's targets
int sam_header_text(otg_bam* bam, const char* read_group, int32_t offset_l, int32_t offset_r, std::string& out)
{
  const uint32_t nt = otg_bam_n_targets(bam);
  std::string names; std::vector<uint64_t> off(nt), len(nt); std::vector<uint32_t> nl(nt);
  for (uint32_t i = 0; i < nt; ++i) { uint64_t l = 0; const char* nm = otg_bam_target(bam, i, &l); off[i] = names.size(); nl[i] = (uint32_t)strlen(nm); len[i] = l; names += nm; }
  return sized_text(out, [&](char* buf, uint64_t cap, uint64_t* need) {
    return otg_emit_sam_header(names.data(), off.data(), nl.data(), len.data(), nt, read_group, offset_l, offset_r, buf, cap, need);
  });
}

// Two batches in flight: while the caller works on current(), prefetch() fills the other buffer on a thread of its own; advance() waits
// for it and makes it current.  The destructor joins the thread, so an entry point may return at any point of its loop.
template <class B>
class TwoInFlight {
 public:
  TwoInFlight() = default;
  TwoInFlight(const TwoInFlight&) = delete;
  ~TwoInFlight() { join(); }
  B& current() { return bufs_[idx_ & 1]; }
  B& other() { return bufs_[(idx_ + 1) & 1]; }
  B* begin() { return bufs_; }
  B* end() { return bufs_ + 2; }
  template <class Fill> void prefetch(Fill fill) {
    join();
    B* o = &other();
    next_ = std::thread([fill, o] { fill(*o); });
  }
  void advance() { join(); ++idx_; }
 private:
  void join() { if (next_.joinable()) next_.join(); }
  B bufs_[2];
  uint32_t idx_ = 0;
  std::thread next_;
};

// ---- stage 1: one batch of regions from the BAM (and the FASTA flanks with -r), buffers grown on OTG_ERR_CAPACITY
int ingest_batch(otg_bam* bam, otg_fasta* fasta, const Bed& bed, const otg_ingest_opts& opts, bool reads_only, int flank, Batch& b, int threads)
{
  otg_ingest_opts o = opts;
  o.threads = threads;
  const otg_bed* beds = bed.beds.data() + b.first;
  const char* chr = bed.chr_arena.data();
  b.regions.assign(b.n, otg_region{});
  size_t cap_reads = std::max<size_t>(b.reads.size(), (size_t)b.n * 48 + 256), cap_arena = std::max<size_t>(b.arena.size(), (size_t)b.n * 48 * 4096 + 4096);
  size_t cap_names = std::max<size_t>(b.names.size(), reads_only ? (size_t)b.n * 48 * 48 : 0);
  for (int attempt = 0; attempt < 4; ++attempt) {
    b.reads.resize(cap_reads); b.arena.resize(cap_arena);
    if (reads_only) { b.meta.resize(cap_reads); b.names.resize(cap_names); }
    uint64_t used = 0, nused = 0; uint32_t nr = 0;
    const int rc = reads_only
        ? otg_ingest_regions_named(bam, beds, chr, b.n, &o, b.arena.data(), b.arena.size(), &used, b.reads.data(), (uint32_t)b.reads.size(), &nr, b.regions.data(),
                                   b.meta.data(), b.names.data(), b.names.size(), &nused)
        : otg_ingest_regions(bam, beds, chr, b.n, &o, b.arena.data(), b.arena.size(), &used, b.reads.data(), (uint32_t)b.reads.size(), &nr, b.regions.data());
    if (rc == OTG_ERR_CAPACITY) {      // the counters hold the needed totals
      cap_reads = (size_t)nr + 256; cap_arena = (size_t)used + 4096 + (fasta ? (size_t)b.n * 2 * ((size_t)flank + 8) : 0); cap_names = (size_t)nused + 256;
      continue;
    }
    if (rc != OTG_OK) return rc;
    b.arena_used = used; b.n_reads = nr;
    if (fasta) {
      const size_t need = used + (size_t)b.n * 2 * ((size_t)flank + 8) + 128;
      if (b.arena.size() < need) b.arena.resize(need, (size_t)used);
      uint64_t u2 = used;
      const int rf = otg_fasta_region_flanks(fasta, beds, chr, b.n, o.offset_l, o.offset_r, flank, b.arena.data(), b.arena.size(), &u2, b.regions.data());
      if (rf != OTG_OK) return rf;
      b.arena_used = u2;
    }
    return OTG_OK;
  }
  return OTG_ERR_CAPACITY;
}

// ---- stage 2 of one batch on one context: submit -> run -> result sizes, then (where the records are wanted on the host) collect
int hot_path_on(otg_ctx* ctx, const otg_params& P, const Batch& b, uint32_t* n_alleles, uint64_t* seq_bytes)
{
  auto t0 = Clock::now();
  int rc = otg_assemble_submit(ctx, &P, b.arena.data(), b.arena_used, b.reads.data(), b.n_reads, b.regions.data(), b.n);
  trace("submit", b.index, b.n, t0);
  t0 = Clock::now();
  if (rc == OTG_OK) rc = otg_assemble_run(ctx);
  trace("run", b.index, b.n, t0);
  if (rc == OTG_OK) rc = otg_assemble_result_sizes(ctx, n_alleles, seq_bytes);
  return rc;
}
int collect_on(otg_ctx* ctx, const Batch& b, uint32_t n_alleles, uint64_t seq_bytes, std::vector<otg_region_result>& rr, std::vector<otg_allele>& al, std::vector<uint8_t>& seqs)
{
  const auto t0 = Clock::now();
  rr.resize(b.n); al.resize((size_t)n_alleles + 1); seqs.resize((size_t)seq_bytes + 64);
  const int rc = otg_assemble_collect(ctx, rr.data(), al.data(), (uint32_t)al.size(), seqs.data(), seqs.size(), nullptr);
  if (rc == OTG_OK) trace("collect", b.index, b.n, t0);
  return rc;
}
// ---- stage 3: the allele records of a collected batch, as `otter assemble -R <read_group>` prints them
int alleles_text(const Bed& bed, const Batch& b, const std::vector<otg_region_result>& rr, const std::vector<otg_allele>& al, const std::vector<uint8_t>& seqs, const char* read_group,
                 int is_fasta, std::string& out)
{
  return sized_text(out, [&](char* buf, uint64_t cap, uint64_t* need) {
    return otg_emit_alleles(bed.beds.data() + b.first, bed.chr_arena.data(), b.n, rr.data(), al.data(), seqs.data(), read_group, is_fasta, buf, cap, need);
  });
}

// otg_spread_files: the unit sets of the catalogue (one per BED record with units, the records' contiguous stretches of the unit list), the
// set of every BED record or OTG_SPREAD_NONE, and the scores
struct SpreadSets {
  std::vector<uint64_t> set_first, unit_off;
  std::vector<uint32_t> unit_len, set_of;
  std::vector<uint8_t> arena;
  uint64_t unit_bytes = 0;
  otg_tract_params q{};
};

// What otg_assemble_files' threads share besides the Job: the caller's options and the open inputs.
struct AssembleShared {
  const otg_assemble_job* j = nullptr;
  const SpreadSets* spread = nullptr;    // otg_spread_files: the emit stage writes spread rows, not allele records
  Job J;
  Bed bed;
  BamPtr bam;
  FastaPtr fasta;
};

// ---- stage 2 + 3 of one batch on one context: hot path, then the record text
int run_batch(AssembleShared& A, otg_ctx* ctx, Batch& b, std::vector<otg_region_result>& rr, std::vector<otg_allele>& al, std::vector<uint8_t>& seqs, double* ms_gpu, double* ms_emit)
{
  const otg_assemble_job& j = *A.j;
  otg_params P = j.params;
  P.realign = A.fasta ? 1 : 0;
  const char* rg = j.read_group ? j.read_group : "";
  auto t0 = Clock::now();
  if (j.reads_only) {
    // --reads-only: the reads of each region; with -r they are printed after local_realignment trimmed them (src/assemble.cpp:72-89)
    if (A.fasta && b.n_reads) {
      int rc = otg_assemble_submit(ctx, &P, b.arena.data(), b.arena_used, b.reads.data(), b.n_reads, b.regions.data(), b.n);
      if (rc == OTG_OK) rc = otg_assemble_realign(ctx);
      if (rc == OTG_OK) rc = otg_assemble_collect_reads(ctx, b.reads.data(), b.n_reads);
      if (rc != OTG_OK) return rc;
    }
    *ms_gpu += ms_since(t0);
    t0 = Clock::now();
    const int rc = sized_text(b.text, [&](char* buf, uint64_t cap, uint64_t* need) {
      return otg_emit_reads(A.bed.beds.data() + b.first, A.bed.chr_arena.data(), b.n, b.regions.data(), b.reads.data(), b.arena.data(), b.meta.data(), b.names.data(), rg, j.is_fasta,
                            P.max_cov, buf, cap, need);
    });
    *ms_emit += ms_since(t0);
    return rc;
  }
  uint32_t na = 0; uint64_t sb = 0;
  int rc = hot_path_on(ctx, P, b, &na, &sb);
  if (rc == OTG_OK) rc = collect_on(ctx, b, na, sb, rr, al, seqs);
  if (rc != OTG_OK) return rc;
  std::vector<otg_spread> sp_rec;
  std::vector<uint64_t> sp_off;
  std::vector<otg_spread_unit> sp_units;
  std::vector<uint32_t> sp_set;
  if (A.spread) {                        // the spread of the batch that has just run, on the same context; only its records come to the host
    const SpreadSets& S = *A.spread;
    sp_set.assign(S.set_of.begin() + b.first, S.set_of.begin() + b.first + b.n);
    sp_set.push_back(OTG_SPREAD_NONE);
    sp_rec.resize((size_t)na + 1); sp_off.resize((size_t)na + 2);
    uint64_t nu = 0;
    rc = otg_assemble_spread(ctx, S.arena.data(), S.unit_bytes, S.unit_off.data(), S.unit_len.data(), (uint32_t)(S.unit_off.size() - 1), S.set_first.data(),
                             (uint32_t)(S.set_first.size() - 1), sp_set.data(), b.n, &S.q, sp_rec.data(), sp_off.data(), &nu);
    if (rc != OTG_OK) return rc;
    sp_units.resize((size_t)nu + 1);
    if ((rc = otg_spread_collect(ctx, sp_units.data(), nu)) != OTG_OK) return rc;
  }
  *ms_gpu += ms_since(t0);
  t0 = Clock::now();
  if (A.spread) {
    const SpreadSets& S = *A.spread;
    b.text.clear();
    otg_spread_rows(b.text, A.bed.beds.data() + b.first, A.bed.chr_arena.data(), b.n, rr.data(), al.data(), sp_set.data(), S.set_first.data(), S.arena.data(),
                    S.unit_off.data(), S.unit_len.data(), sp_rec.data(), sp_off.data(), sp_units.data());
  } else
    rc = alleles_text(A.bed, b, rr, al, seqs, rg, j.is_fasta, b.text);
  *ms_emit += ms_since(t0);
  trace("emit", b.index, b.n, t0);
  {
    std::lock_guard<std::mutex> lk(A.J.st_m);
    A.J.st.n_alleles += na;
    for (uint32_t r = 0; r < b.n; ++r) { if (rr[r].n_alleles) ++A.J.st.n_regions_ok; if (rr[r].status == OTG_REGION_SKIP_MAXCOV) ++A.J.st.n_regions_skipped; }
  }
  return rc;
}

// Batch objects cycle between the ingest thread and the hot-path threads of a shard: their vectors keep the capacity of the batches they
// have carried (no 400 MB zero-fill per batch; at most 2 x contexts + 2 objects exist per shard).
struct BatchPool {
  std::mutex m;
  std::vector<std::unique_ptr<Batch>> free_;
  void clear() { std::lock_guard<std::mutex> lk(m); free_.clear(); }
  std::unique_ptr<Batch> get() {
    std::lock_guard<std::mutex> lk(m);
    if (free_.empty()) return std::unique_ptr<Batch>(new Batch());
    std::unique_ptr<Batch> b = std::move(free_.back());
    free_.pop_back();
    return b;
  }
  void put(std::unique_ptr<Batch> b) { b->text.clear(); std::lock_guard<std::mutex> lk(m); free_.push_back(std::move(b)); }
};

// How a shard [a, b) is cut into batches.  A size given by the caller is kept as it is.  Left to the library (batch_regions == 0): the device
// idles while the FIRST batch is being read, so the shard starts small (256, 512, 1024 regions); then full batches of 2048 — a batch costs
// ~35 ms + 64 ms per 1 000 regions, its longest alignment and its largest graph only overlap with the NEXT batch's body —; and the last
// stretch goes to the two contexts of the device as two equal halves, so that they run out of work together (ending on ever smaller batches
// instead — thirds of what is left — cost 5 % of a 10 000-region job: six small batches, each with the fixed cost of a batch).
std::vector<std::pair<uint32_t, uint32_t>> batch_plan(uint32_t a, uint32_t b, uint32_t requested)
{
  std::vector<std::pair<uint32_t, uint32_t>> plan;
  if (a >= b) return plan;
  if (requested) { for (uint32_t f = a; f < b; f += requested) plan.emplace_back(f, std::min(requested, b - f)); return plan; }
  const uint32_t per = 2048u;      // (r04, measured again on 10 000 loci: 1024 -> 10 400 regions/s, 2048 -> 11 500, 3072 -> 11 500, 4096 -> 11 300;
                                   //  on 60 000 loci: 2048 -> 12 270, 4096 -> 12 200, 8192 -> 12 020 — larger batches lower the hot path's busy time, not the wall)
  uint32_t f = a, rem = b - a;
  auto take = [&](uint32_t n) { plan.emplace_back(f, n); f += n; rem -= n; };
  for (uint32_t r = per / 8; r < per; r *= 2) if (rem > 4 * r) take(r);
  while (rem) {
    if (rem > per + per / 4) take(per);
    else if (rem > per / 2) { const uint32_t h = (rem + 1) / 2; take(h); take(rem); }
    else take(rem);
  }
  return plan;
}

// Like the contexts, batch objects outlive the job (their buffers are a few hundred megabytes each: unmapping them at the end of a job and
// mapping them again at the start of the next costs tens of milliseconds per object); otg_assemble_files_release() frees them.
BatchPool g_batches;

// ---- the devices of a job and the BED-order writer over their shards
// static contiguous split over the workers (BS::thread_pool::parallelize_loop: block = total / workers, the last takes the remainder)
std::pair<uint32_t, uint32_t> shard_bounds(uint32_t R, uint32_t W, uint32_t w)
{
  const uint32_t block = R / W;
  if (block == 0) return {std::min(w, R), std::min(w + 1, R)};
  return {w * block, w == W - 1 ? R : (w + 1) * block};
}

// One worker thread per device on its shard of the R regions, and on the calling thread the writer: shards in order, batches in order.
// worker(device, a, b, ingest threads, out) delivers the batches of [a, b) to `out`; write_step(batch, payload) hands one to the caller's
// callbacks and returns false (after J.fail) when they refuse it.  Returns the number of devices.
template <class T, class Worker, class WriteStep>
uint32_t run_shards(Job& J, const int32_t* devices, int32_t n_devices, uint32_t R, uint32_t batch_regions, int threads_total, Worker worker, WriteStep write_step)
{
  std::vector<int> devs;
  if (n_devices > 0) devs.assign(devices, devices + n_devices); else devs.push_back(0);
  const uint32_t W = (uint32_t)devs.size();
  const int threads_per = std::max(1, std::max(1, threads_total) / (int)W);
  std::vector<std::unique_ptr<OrderedOutput<T>>> outs;
  std::vector<std::thread> workers;
  for (uint32_t w = 0; w < W; ++w) {
    const std::pair<uint32_t, uint32_t> s = shard_bounds(R, W, w);
    outs.emplace_back(new OrderedOutput<T>(J.rc, (uint32_t)batch_plan(s.first, s.second, batch_regions).size()));
    workers.emplace_back(worker, devs[w], s.first, s.second, threads_per, std::ref(*outs[w]));
  }
  for (uint32_t w = 0; w < W && J.rc.load() == OTG_OK; ++w) {
    T payload;
    for (uint32_t k = 0; k < outs[w]->n_batches() && J.rc.load() == OTG_OK; ++k)
      if (!outs[w]->take(k, payload) || !write_step(k, payload)) break;
  }
  for (auto& o : outs) o->wake();
  for (auto& t : workers) t.join();
  pool_trim();
  return W;
}

// ---- one device's shard [a, b): ingest thread -> two hot-path threads -> ordered text
void shard_worker(AssembleShared& A, int device, uint32_t a, uint32_t bnd, int ingest_threads, OrderedOutput<std::string>& out)
{
  if (a >= bnd) return;                 // more devices than regions: nothing to do here (and no context to create)
  Job& J = A.J;
  const otg_assemble_job& j = *A.j;
  const std::vector<std::pair<uint32_t, uint32_t>> plan = batch_plan(a, bnd, j.batch_regions);
  // hot-path threads (one context each) per device: a batch of a few hundred regions cannot fill the device — its stages wait for their
  // longest alignment / graph — so several batches are in flight; OTG_DISPATCH_CONTEXTS overrides (1..4)
  const int n_gpu_threads = dispatch_contexts();
  BoundedQueue<BatchPtr> q_in((size_t)n_gpu_threads);
  BatchPool& recycled = g_batches;
  out.set_cap((size_t)n_gpu_threads + 1);
  double ms_ingest = 0, ms_gpu[4] = {0, 0, 0, 0}, ms_emit[4] = {0, 0, 0, 0};
  std::thread ingest([&] {
    try {
      for (uint32_t idx = 0; idx < (uint32_t)plan.size() && J.rc.load() == OTG_OK; ++idx) {
        BatchPtr b = recycled.get();
        b->index = idx; b->first = plan[idx].first; b->n = plan[idx].second;
        const auto t0 = Clock::now();
        const int rc = ingest_batch(A.bam.get(), A.fasta.get(), A.bed, j.ingest, j.reads_only != 0, j.params.flank, *b, ingest_threads);
        ms_ingest += ms_since(t0);
        trace("ingest", idx, b->n, t0);
        if (rc != OTG_OK) { J.fail(rc, "ingest: " + last_err()); break; }
        { std::lock_guard<std::mutex> lk(J.st_m); J.st.n_reads += b->n_reads; J.st.input_bytes += b->arena_used; }
        if (!q_in.push(std::move(b))) break;
      }
    } catch (const std::exception& e) { J.fail(OTG_ERR_ARG, std::string("ingest: ") + e.what()); }
    q_in.finish();
  });
  auto gpu_thread = [&](int slot) {
    PooledCtx ctx(nullptr, PoolReturn{device});
    const bool need_gpu = !j.reads_only || A.fasta;
    if (need_gpu && !(ctx = acquire_ctx(device))) { J.fail(OTG_ERR_NO_DEVICE, "otg_create: " + last_err()); q_in.abort(); return; }
    std::vector<otg_region_result> rr; std::vector<otg_allele> al; std::vector<uint8_t> seqs;
    try {
      BatchPtr b;
      while (J.rc.load() == OTG_OK && q_in.pop(b)) {
        const int rc = run_batch(A, ctx.get(), *b, rr, al, seqs, &ms_gpu[slot], &ms_emit[slot]);
        if (rc != OTG_OK) { J.fail(rc, "hot path: " + (ctx && otg_last_error(ctx.get()) ? ctx_err(ctx.get()) : last_err())); q_in.abort(); break; }
        out.deliver(b->index, std::move(b->text));
        recycled.put(std::move(b));
      }
    } catch (const std::exception& e) { J.fail(OTG_ERR_ARG, std::string("hot path: ") + e.what()); }
    if (J.rc.load() != OTG_OK) q_in.abort();               // whatever stopped the job: release the ingest thread
  };
  std::vector<std::thread> gts;
  for (int t = 0; t < n_gpu_threads; ++t) gts.emplace_back(gpu_thread, t);
  ingest.join();
  for (auto& t : gts) t.join();
  out.wake();
  std::lock_guard<std::mutex> lk(J.st_m);
  J.st.ms_ingest += ms_ingest;
  for (int t = 0; t < n_gpu_threads; ++t) { J.st.ms_hot_path += ms_gpu[t]; J.st.ms_emit += ms_emit[t]; }
}

// ---- the VCF lines of a batch (output_vcf_line, src/genotype.cpp:43-78, is a pure function of its region): contiguous slices of its n
// regions, starting at BED record `first_bed`, formatted on up to `threads` host threads into `parts` and concatenated in order into `text`.
// `first` (n + 1 entries), `n_gt` are the batch's; alleles, seqs, gt, hsd, reps are indexed by what `first` holds.  On failure *err is the
// failing slice's error text, which only the slice's own thread can read.
int emit_vcf_sliced(const Bed& bed, uint32_t first_bed, uint32_t n, const uint32_t* first, const otg_allele* alleles, const uint8_t* seqs, uint32_t n_samples, const int32_t* gt,
                    const double* hsd, const int32_t* n_gt, const int32_t* reps, int32_t offset_l, int32_t offset_r, int threads, std::vector<std::string>& parts, std::string& text,
                    std::string* err)
{
  const uint32_t nslice = (uint32_t)std::max(1, std::min<int>(threads, (int)((n + 31) / 32)));
  parts.assign(nslice, std::string());
  std::vector<int> prc(nslice, OTG_OK);
  std::vector<std::string> perr(nslice);
  auto emit_slice = [&](uint32_t sidx) {
    const uint32_t a = (uint32_t)((uint64_t)n * sidx / nslice), e = (uint32_t)((uint64_t)n * (sidx + 1) / nslice);
    std::string& out = parts[sidx];
    uint64_t bytes = (uint64_t)(e - a) * (512 + 80ull * (n_samples + 1));
    for (uint32_t i = first[a]; i < first[e]; ++i) bytes += alleles[i].seq_len + 8;          // every allele sequence could be an ALT
    uint64_t len = 0;
    int rc = OTG_ERR_CAPACITY;
    // (the estimate above is an upper bound: the second round, with the size the first one reported, is a safety net)
    for (int round = 0; round < 2 && rc == OTG_ERR_CAPACITY; ++round, bytes = len) {
      out.resize(bytes);
      rc = otg_emit_vcf_lines(bed.beds.data() + first_bed + a, bed.chr_arena.data(), e - a, first + a, alleles, seqs, n_samples, gt, hsd, n_gt + a, reps, offset_l, offset_r,
                              bytes ? &out[0] : nullptr, bytes, &len);
    }
    if (rc != OTG_OK) perr[sidx] = last_err();
    prc[sidx] = rc;
    out.resize(rc == OTG_OK ? len : 0);
  };
  if (nslice == 1) emit_slice(0);
  else {
    std::vector<std::thread> th;
    for (uint32_t sidx = 0; sidx < nslice; ++sidx) th.emplace_back(emit_slice, sidx);
    for (auto& t : th) t.join();
  }
  text.clear();
  for (uint32_t sidx = 0; sidx < nslice; ++sidx) {
    if (prc[sidx] != OTG_OK) { if (err) *err = perr[sidx]; return prc[sidx]; }
    text += parts[sidx];
  }
  return OTG_OK;
}

// ---- the cohort dispatcher (otg_cohort_files): per device shard, per batch, per sample: ingest -> hot path -> otg_cohort_stage; the thread that
// stages the last sample of a batch regroups, clusters, collects and formats it.
struct CohortText { std::string vcf, mat; std::vector<std::string> sam; };
struct CohortRef {                           // reference alleles of one batch (genotype_process, src/genotype.cpp:93-101), fetched once
  std::vector<uint8_t> arena; std::vector<uint64_t> off; std::vector<uint32_t> len;
};
struct CohortItem { BatchPtr b; uint32_t sample = 0; std::shared_ptr<CohortRef> ref; };
struct CohortSlot {                          // one batch being staged on a device: a light context of its own (a stream and the staging buffers)
  otg_ctx* ctx = nullptr;
  std::mutex m;
  std::condition_variable cv;
  int64_t batch = -1;                        // the batch it is open for (-1: free)
  int64_t next = 0;                          // the batch that may open it next (slots alternate: next += 2)
  uint32_t staged = 0;
  std::vector<std::string> sam;
};
struct CohortShared {
  const otg_cohort_job* j = nullptr;
  Job M;                                     // job status and statistics
  Bed bed;
  FastaPtr fasta;
  std::vector<BamPtr> bams;                  // one per sample
  otg_params P;
  uint32_t n_samples = 0;
};

int fetch_reference_alleles(const CohortShared& C, uint32_t first, uint32_t n, CohortRef& R)
{
  R.arena.clear(); R.off.assign(n, 0); R.len.assign(n, 0);
  std::vector<char> buf;
  for (uint32_t g = 0; g < n; ++g) {
    const otg_bed& bd = C.bed.beds[first + g];
    const int fb = (int)(uint32_t)bd.start - C.j->ingest.offset_l, fe = (int)(uint32_t)bd.end + C.j->ingest.offset_r - 1;
    uint64_t need = 0;
    buf.resize((size_t)(fe >= fb ? (long long)fe - fb + 2 : 2) + 16);
    if (otg_fasta_fetch(C.fasta.get(), C.bed.chr_arena.data() + bd.chr_off, bd.chr_len, fb, fe, buf.data(), buf.size(), &need) != OTG_OK) {
      buf.resize((size_t)need + 16);
      if (otg_fasta_fetch(C.fasta.get(), C.bed.chr_arena.data() + bd.chr_off, bd.chr_len, fb, fe, buf.data(), buf.size(), &need) != OTG_OK) return OTG_ERR_ARG;
    }
    R.off[g] = R.arena.size(); R.len[g] = (uint32_t)need;
    R.arena.insert(R.arena.end(), (const uint8_t*)buf.data(), (const uint8_t*)buf.data() + need);
  }
  R.arena.resize(R.arena.size() + 64, 0);
  return OTG_OK;
}

// Device bytes the k-mer workspace of a cohort slot context may take per range of matrix rows (usage rows, gc, hsd, tier L histograms); the
// host holds two thirds of that as the rows' doubles.  Every range costs two launches and a synchronisation, so the cap wants to be large
// next to a batch's rows at the common k (a row is 520 B at k = 3, 8 KiB at k = 5) and small next to the device: 256 MiB is half a million
// rows at k = 3 and leaves a batch in one range up to k = 7.  Above that the ranges shrink to single rows (k = 11: 48 MiB a row; k = 12 takes
// 192 MiB for its one row).  DESIGN.md §4.
constexpr uint64_t COHORT_MATRIX_WORKSPACE = 256ull << 20;

// the matrix rows of a clustered batch (otg_kmer_cohort_rows / otg_kmer_cohort_usage), formatted as vcf2mat prints them for the batch's VCF lines
int cohort_matrix_text(CohortShared& C, otg_ctx* cctx, const Batch& b, const uint32_t* first, const otg_allele* alleles, const uint8_t* seqs, uint32_t na, int threads,
                       std::string& text, double* ms_gpu, double* ms_emit)
{
  auto t0 = Clock::now();
  const int k = C.j->matrix_k;
  const uint32_t n = b.n;
  uint32_t n_rows = 0;
  std::vector<uint32_t> row_first((size_t)n + 1), row_allele((size_t)na + 1);
  int rc = otg_kmer_cohort_rows(cctx, &n_rows, row_first.data(), row_allele.data(), nullptr);
  if (rc != OTG_OK) return rc;
  *ms_gpu += ms_since(t0);
  text.clear();
  if (n_rows == 0) return OTG_OK;
  // the region strings: the ID column of the VCF line, chr:start-end
  std::string names; std::vector<uint64_t> name_off((size_t)n + 1, 0);
  for (uint32_t r = 0; r < n; ++r) {
    name_off[r] = names.size();
    if (first[r + 1] == first[r]) continue;
    const otg_bed& bd = C.bed.beds[b.first + r];
    names.append(C.bed.chr_arena.data() + bd.chr_off, bd.chr_len);
    names += ':'; names += std::to_string((uint32_t)bd.start); names += '-'; names += std::to_string((uint32_t)bd.end);
  }
  name_off[n] = names.size();
  const uint64_t bins = (1ull << (2 * k)) + 1;
  const uint64_t row_bytes = bins * 8 + 16 + (k >= 8 ? bins * 4 : 0);
  const uint32_t per = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(COHORT_MATRIX_WORKSPACE / row_bytes, 1u << 20));
  std::vector<double> usage, gc, hsd;
  std::vector<uint32_t> len;
  std::vector<otg_vcf_record> rec;
  std::vector<std::string> parts;
  uint32_t r = 0;                                                  // the region of row `lo`
  for (uint32_t lo = 0; lo < n_rows; lo += per) {
    const uint32_t m = std::min(per, n_rows - lo);
    t0 = Clock::now();
    usage.resize((size_t)m * bins); gc.resize(m); hsd.resize(m); len.resize(m);
    rc = otg_kmer_cohort_usage(cctx, k, lo, m, usage.data(), gc.data(), hsd.data());
    if (rc != OTG_OK) return rc;
    *ms_gpu += ms_since(t0);
    t0 = Clock::now();
    for (uint32_t i = 0; i < m; ++i) len[i] = alleles[row_allele[lo + i]].seq_len;
    // the records of the range: its part of every region it meets; the first may continue a region begun in the range before
    while (row_first[r + 1] <= lo) ++r;
    // The VCF prints an ALT allele that is the one byte N — a zero-length allele — as <DEL> (otg_emit_vcf_lines), and vcf2mat reads <DEL> back
    // as N only where it is the whole ALT column: beside other ALT alleles parse_alleles keeps the five characters (src/vcf2mat.cpp:30-33).
    // The row of that text: length 5, no C or G, every window in the non-ACGT bin (k <= 5) or no window at all (0 / 0), one term of diversity 1.
    for (uint32_t q = r; q < n && row_first[q] < lo + m; ++q) {
      if (row_first[q + 1] - row_first[q] < 3) continue;
      for (uint32_t row = std::max(row_first[q] + 1, lo); row < std::min(row_first[q + 1], lo + m); ++row) {
        const otg_allele& al = alleles[row_allele[row]];
        if (al.seq_len != 1 || seqs[al.seq_off] != 'N') continue;
        const uint32_t i = row - lo;
        len[i] = 5; gc[i] = 0.0; hsd[i] = 1.0;
        double* u = usage.data() + (size_t)i * bins;
        std::fill(u, u + bins, k <= 5 ? 0.0 : std::nan(""));
        if (k <= 5) u[bins - 1] = 1.0;
      }
    }
    const uint32_t index0 = lo - row_first[r];
    rec.clear();
    for (uint32_t q = r; q < n && row_first[q] < lo + m; ++q) {
      const uint32_t a0 = std::max(row_first[q], lo), a1 = std::min(row_first[q + 1], lo + m);
      if (a1 <= a0) continue;
      otg_vcf_record R;
      R.region_off = name_off[q]; R.region_len = (uint32_t)(name_off[q + 1] - name_off[q]); R.first_allele = a0 - lo; R.n_alleles = a1 - a0; R.reserved = 0;
      rec.push_back(R);
    }
    // contiguous record ranges, one per thread, appended in order
    const uint32_t nrec = (uint32_t)rec.size(), nt = (uint32_t)std::max(1, std::min<int>(threads, (int)nrec));
    parts.assign(nt, std::string());
    auto rows_of = [&](uint32_t t) {
      const uint32_t c0 = (uint32_t)((uint64_t)nrec * t / nt), c1 = (uint32_t)((uint64_t)nrec * (t + 1) / nt);
      if (c1 > c0) otg_vcf2mat_rows(parts[t], rec.data() + c0, c1 - c0, names.data(), len.data(), k, usage.data(), gc.data(), hsd.data(), c0 == 0 ? index0 : 0u);
    };
    if (nt == 1) rows_of(0);
    else {
      std::vector<std::thread> th;
      for (uint32_t t = 0; t < nt; ++t) th.emplace_back(rows_of, t);
      for (auto& t : th) t.join();
    }
    for (const std::string& p : parts) text += p;
    *ms_emit += ms_since(t0);
  }
  return OTG_OK;
}

// regroup + cluster + collect + VCF lines (+ matrix rows) of one fully staged batch
int cohort_finish_batch(CohortShared& C, otg_ctx* cctx, const Batch& b, const CohortRef& ref, int threads, std::string& text, std::string& matrix, double* ms_gpu, double* ms_emit, uint32_t* n_ok,
                        const char** step)
{
  *step = "genotype";
  auto t0 = Clock::now();
  int rc = otg_cohort_regroup(cctx, ref.arena.data(), ref.arena.size(), ref.off.data(), ref.len.data());
  if (rc == OTG_OK) rc = otg_genotype_cohort_metric(cctx, &C.P, C.j->gt_metric);
  uint32_t na = 0; uint64_t sb = 0;
  if (rc == OTG_OK) rc = otg_cohort_result_sizes(cctx, &na, &sb);
  if (rc != OTG_OK) return rc;
  const uint32_t n = b.n;
  std::vector<uint32_t> first((size_t)n + 1); std::vector<otg_allele> alleles((size_t)na + 1); std::vector<uint8_t> seqs((size_t)sb + 64);
  std::vector<int32_t> gt((size_t)na + 1), reps((size_t)na + 1), ngt((size_t)n + 1); std::vector<double> hsd((size_t)na + 1);
  rc = otg_cohort_collect(cctx, first.data(), alleles.data(), na, nullptr, nullptr, nullptr, seqs.data(), sb, gt.data(), nullptr, nullptr, hsd.data(), ngt.data(), reps.data());
  if (rc != OTG_OK) return rc;
  *ms_gpu += ms_since(t0);
  t0 = Clock::now();
  std::vector<std::string> parts;
  rc = emit_vcf_sliced(C.bed, b.first, n, first.data(), alleles.data(), seqs.data(), C.n_samples, gt.data(), hsd.data(), ngt.data(), reps.data(), C.j->ingest.offset_l,
                       C.j->ingest.offset_r, threads, parts, text, nullptr);
  if (rc != OTG_OK) return rc;
  for (uint32_t r = 0; r < n; ++r) if (first[r + 1] > first[r]) ++*n_ok;
  *ms_emit += ms_since(t0);
  *step = "matrix";
  if (C.j->matrix_write) return cohort_matrix_text(C, cctx, b, first.data(), alleles.data(), seqs.data(), na, threads, matrix, ms_gpu, ms_emit);
  return OTG_OK;
}

void cohort_shard_worker(CohortShared& C, int device, uint32_t a, uint32_t bnd, int ingest_threads, OrderedOutput<CohortText>& out)
{
  if (a >= bnd) return;
  Job& M = C.M;
  const uint32_t S = C.n_samples;
  const bool want_sam = C.j->allele_write != nullptr;
  const std::vector<std::pair<uint32_t, uint32_t>> plan = batch_plan(a, bnd, C.j->batch_regions);
  const int n_gpu_threads = dispatch_contexts();
  BoundedQueue<CohortItem> q_in((size_t)n_gpu_threads);
  BatchPool& recycled = g_batches;
  out.set_cap((size_t)n_gpu_threads + 1);
  CohortSlot slots[2];
  for (int i = 0; i < 2; ++i) {
    slots[i].next = i;
    if (otg_create(device, &slots[i].ctx) != OTG_OK) { M.fail(OTG_ERR_NO_DEVICE, "otg_create: " + last_err()); for (int k = 0; k < i; ++k) otg_destroy(slots[k].ctx); return; }
  }
  double ms_ingest = 0, ms_gpu[4] = {0, 0, 0, 0}, ms_emit[4] = {0, 0, 0, 0};
  std::thread ingest([&] {
    try {
      for (uint32_t idx = 0; idx < (uint32_t)plan.size() && M.rc.load() == OTG_OK; ++idx) {
        auto ref = std::make_shared<CohortRef>();
        const auto tr = Clock::now();
        if (fetch_reference_alleles(C, plan[idx].first, plan[idx].second, *ref) != OTG_OK) { M.fail(OTG_ERR_ARG, "cannot fetch the reference alleles: " + last_err()); break; }
        ms_ingest += ms_since(tr);
        bool stop = false;
        for (uint32_t s = 0; s < S && M.rc.load() == OTG_OK; ++s) {
          CohortItem it;
          it.b = recycled.get(); it.sample = s; it.ref = ref;
          it.b->index = idx; it.b->first = plan[idx].first; it.b->n = plan[idx].second;
          const auto t0 = Clock::now();
          const int rc = ingest_batch(C.bams[s].get(), C.fasta.get(), C.bed, C.j->ingest, false, C.P.flank, *it.b, ingest_threads);
          ms_ingest += ms_since(t0);
          trace("ingest", idx, it.b->n, t0);
          if (rc != OTG_OK) { M.fail(rc, std::string("ingest of ") + C.j->bam_paths[s] + ": " + last_err()); stop = true; break; }
          { std::lock_guard<std::mutex> lk(M.st_m); M.st.n_reads += it.b->n_reads; M.st.input_bytes += it.b->arena_used; }
          if (!q_in.push(std::move(it))) { stop = true; break; }
        }
        if (stop) break;
      }
    } catch (const std::exception& e) { M.fail(OTG_ERR_ARG, std::string("ingest: ") + e.what()); }
    q_in.finish();
  });
  auto gpu_thread = [&](int slot_idx) {
    const PooledCtx pooled = acquire_ctx(device);
    otg_ctx* ctx = pooled.get();
    if (!ctx) { M.fail(OTG_ERR_NO_DEVICE, "otg_create: " + last_err()); q_in.abort(); return; }
    std::vector<otg_region_result> rr; std::vector<otg_allele> al; std::vector<uint8_t> seqs;
    auto fail_ctx = [&](int rc, const char* what, otg_ctx* c) { M.fail(rc, std::string(what) + ": " + (c && otg_last_error(c) && otg_last_error(c)[0] ? ctx_err(c) : last_err())); q_in.abort(); };
    try {
      CohortItem it;
      while (M.rc.load() == OTG_OK && q_in.pop(it)) {
        Batch& b = *it.b;
        const uint32_t idx = b.index, s = it.sample;
        auto t0 = Clock::now();
        uint32_t na = 0; uint64_t sb = 0;
        int rc = hot_path_on(ctx, C.P, b, &na, &sb);
        if (rc != OTG_OK) { fail_ctx(rc, "hot path", ctx); break; }
        ms_gpu[slot_idx] += ms_since(t0);
        std::string sam;
        if (want_sam) {
          // the records `otter assemble -R <name>` prints for this sample and batch (otg_assemble_files' text)
          t0 = Clock::now();
          rc = collect_on(ctx, b, na, sb, rr, al, seqs);
          if (rc != OTG_OK) { fail_ctx(rc, "collect", ctx); break; }
          ms_gpu[slot_idx] += ms_since(t0);
          t0 = Clock::now();
          rc = alleles_text(C.bed, b, rr, al, seqs, C.j->sample_names[s], 0, sam);
          if (rc != OTG_OK) { fail_ctx(rc, "emit", nullptr); break; }
          ms_emit[slot_idx] += ms_since(t0);
        }
        // stage into the batch's slot; the thread that brings the last sample finishes the batch
        CohortSlot& sl = slots[idx & 1u];
        CohortText done;
        bool finished = false;
        {
          std::unique_lock<std::mutex> lk(sl.m);
          while (!(sl.batch == (int64_t)idx || (sl.batch < 0 && sl.next == (int64_t)idx) || M.rc.load() != OTG_OK)) sl.cv.wait_for(lk, std::chrono::milliseconds(50));
          if (M.rc.load() != OTG_OK) break;
          t0 = Clock::now();
          if (sl.batch < 0) {
            rc = otg_cohort_begin(sl.ctx, b.n, S);
            if (rc != OTG_OK) { fail_ctx(rc, "cohort", sl.ctx); break; }
            sl.batch = idx; sl.staged = 0; sl.sam.assign(want_sam ? S : 0, std::string());
          }
          rc = otg_cohort_stage(sl.ctx, ctx, s);
          if (rc != OTG_OK) { fail_ctx(rc, "stage", sl.ctx); break; }
          trace("stage", idx, b.n, t0);
          ms_gpu[slot_idx] += ms_since(t0);
          if (want_sam) sl.sam[s] = std::move(sam);
          { std::lock_guard<std::mutex> lk2(M.st_m); M.st.n_alleles += na; }
          if (++sl.staged == S) {
            uint32_t n_ok = 0;
            t0 = Clock::now();
            const char* step = nullptr;
            rc = cohort_finish_batch(C, sl.ctx, b, *it.ref, ingest_threads, done.vcf, done.mat, &ms_gpu[slot_idx], &ms_emit[slot_idx], &n_ok, &step);
            if (rc != OTG_OK) { fail_ctx(rc, step, sl.ctx); break; }
            trace("genotype", idx, b.n, t0);
            (void)otg_cohort_end(sl.ctx);
            done.sam = std::move(sl.sam);
            sl.sam.clear();
            { std::lock_guard<std::mutex> lk2(M.st_m); M.st.n_regions_ok += n_ok; }
            sl.batch = -1; sl.next += 2;
            finished = true;
          }
        }
        sl.cv.notify_all();
        recycled.put(std::move(it.b));
        it.ref.reset();
        if (finished) out.deliver(idx, std::move(done));
      }
    } catch (const std::exception& e) { M.fail(OTG_ERR_ARG, std::string("hot path: ") + e.what()); }
    if (M.rc.load() != OTG_OK) { q_in.abort(); for (auto& sl : slots) sl.cv.notify_all(); }
  };
  std::vector<std::thread> gts;
  for (int t = 0; t < n_gpu_threads; ++t) gts.emplace_back(gpu_thread, t);
  ingest.join();
  for (auto& t : gts) t.join();
  out.wake();
  for (auto& sl : slots) otg_destroy(sl.ctx);
  std::lock_guard<std::mutex> lk(M.st_m);
  M.st.ms_ingest += ms_ingest;
  for (int t = 0; t < n_gpu_threads; ++t) { M.st.ms_hot_path += ms_gpu[t]; M.st.ms_emit += ms_emit[t]; }
}

// One row of text per allele of a VCF, from a file to text: what otg_vcf2mat_files and otg_motifs_files share.  The BED is parsed and filters
// nothing (parse_bed_file, src/vcf2mat.cpp:50-51).  Two batches in flight: while the alleles of one are on the device (on_device(ctx, batch),
// which keeps its results) and its rows are formatted by `threads` host threads (rows(text, batch, first record, records): contiguous record
// ranges with about equal allele counts, written in file order), the next one is read on a host thread.  A batch holds at most `per` alleles;
// a record with more grows the buffers and goes through whole (the device call then reports its workspace).
struct VcfBatch {
  std::vector<otg_vcf_record> rec; std::vector<char> regions; std::vector<uint64_t> off; std::vector<uint32_t> len; std::vector<uint8_t> seqs;
  uint32_t nr = 0, na = 0; uint64_t ru = 0, au = 0, bytes = 0; int rc = OTG_OK; double ms = 0; std::string err;
};

template <class OnDevice, class Rows>
int vcf_allele_job(const char* who, const char* vcf_path, const char* bed_path, int device, uint64_t per, int threads, otg_write_fn write, void* user,
                   otg_job_stats* stats, OnDevice on_device, Rows rows)
{
  const auto t_all = Clock::now();
  otg_job_stats st{};
  {
    Bed bed;
    const int rb = load_bed(bed_path, bed);
    if (rb != OTG_OK) return rb;
  }
  VcfPtr vcf;
  int rc = open_vcf(vcf_path, vcf);
  if (rc != OTG_OK) return rc;
  const PooledCtx ctx = acquire_ctx(device);
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "%s: %s", who, last_err().c_str());
  per = std::max<uint64_t>(1, std::min<uint64_t>(per, 1ull << 24));
  if (threads < 1) threads = 1;
  auto read_into = [&](VcfBatch& B) {
    const auto t0 = Clock::now();
    B.bytes = 0;
    for (;;) {
      B.rc = otg_vcf_read_alleles(vcf.get(), B.rec.data(), (uint32_t)B.rec.size(), &B.nr, B.regions.data(), B.regions.size(), &B.ru, B.off.data(), B.len.data(),
                                  (uint32_t)B.off.size(), &B.na, B.seqs.data(), B.seqs.size(), &B.au, &B.bytes);
      if (B.rc != OTG_ERR_CAPACITY) break;
      // one record larger than the buffers: grow them to hold it
      if (B.na > B.off.size()) { B.off.resize(B.na); B.len.resize(B.na); }
      if (B.ru > B.regions.size()) B.regions.resize(B.ru);
      if (B.au > B.seqs.size()) B.seqs.resize(B.au);
    }
    if (B.rc != OTG_OK) { B.err = last_err(); B.nr = 0; }
    B.ms = ms_since(t0);
  };
  std::vector<std::string> parts((size_t)threads);
  TwoInFlight<VcfBatch> flight;
  for (VcfBatch& B : flight) { B.rec.resize(per); B.off.resize(per); B.len.resize(per); B.regions.resize(1 << 20); B.seqs.resize(64ull << 20); }
  read_into(flight.current());
  for (;; flight.advance()) {
    VcfBatch& B = flight.current();
    st.ms_ingest += B.ms; st.input_bytes += B.bytes;
    if (B.rc != OTG_OK) return otg_fail(nullptr, B.rc, "%s: %s", who, B.err.c_str());
    if (B.nr == 0) break;
    flight.prefetch(read_into);
    st.n_regions += B.nr; st.n_alleles += B.na;
    auto t0 = Clock::now();
    rc = on_device(ctx.get(), B);
    if (rc != OTG_OK) return otg_fail(nullptr, rc, "%s: %s", who, ctx_err(ctx.get()).c_str());
    st.ms_hot_path += ms_since(t0);
    t0 = Clock::now();
    std::vector<uint32_t> cut((size_t)threads + 1, B.nr);
    cut[0] = 0;
    for (uint32_t r = 0, t = 1; r < B.nr && t < (uint32_t)threads; ++r)
      if ((uint64_t)B.rec[r].first_allele * threads >= (uint64_t)B.na * t) cut[t++] = r;
    for (int t = 1; t <= threads; ++t) cut[t] = std::max(cut[t], cut[t - 1]);
    {
      std::vector<std::thread> pool;
      for (int t = 0; t < threads; ++t) {
        parts[t].clear();
        if (cut[t + 1] > cut[t]) pool.emplace_back([&, t] { rows(parts[t], B, cut[t], cut[t + 1] - cut[t]); });
      }
      for (auto& th : pool) th.join();
    }
    st.ms_emit += ms_since(t0);
    for (int t = 0; t < threads; ++t) {
      if (!parts[t].empty() && write(user, parts[t].data(), parts[t].size()) != 0) return otg_fail(nullptr, OTG_ERR_ARG, "%s: the writer failed", who);
      st.output_bytes += parts[t].size();
    }
  }
  st.ms_total = ms_since(t_all); st.n_devices = 1; st.n_regions_ok = st.n_regions;
  if (stats) *stats = st;
  return OTG_OK;
}

// the motif arguments of a job, refused in the command line's words; and the unit stride a motif call over rows of these lengths takes
int motif_cli_args(uint32_t max_period, uint32_t slack)
{
  if (max_period < 1 || max_period > OTG_MOTIF_MAX_PERIOD)
    return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--max-period' (%u). Needs to be 1 <= x <= %d.", max_period, OTG_MOTIF_MAX_PERIOD);
  if (slack > 999) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--slack' (%u). Needs to be 0 <= x <= 999.", slack);
  return OTG_OK;
}
uint32_t motif_unit_stride(const uint32_t* len, uint32_t n, uint32_t max_period)
{
  uint32_t max_len = 0;
  for (uint32_t i = 0; i < n; ++i) max_len = std::max(max_len, len[i]);
  return std::max<uint32_t>(1, std::min<uint32_t>(max_period, max_len / 2));
}

// The tandem-repeat catalogue of a BED: the units of every record (record r: units first[r] .. first[r + 1], unit k = arena[off[k] .. + len[k]))
// and the records by region string as the VCF names them (the first record of a region wins).
struct UnitCatalogue {
  std::vector<uint64_t> first, off;
  std::vector<uint32_t> len;
  std::vector<uint8_t> arena;
  std::map<std::string, uint32_t> by_region;
  int load(const char* who, const char* bed_path)
  {
    Bed bed;
    if (int rc = load_bed(bed_path, bed)) return rc;
    uint64_t nr = 0, nu = 0, ab = 0;
    int rc = otg_parse_bed_units(bed_path, nullptr, 0, &nr, nullptr, nullptr, 0, &nu, nullptr, 0, &ab);
    if (rc != OTG_OK && rc != OTG_ERR_CAPACITY) return rc;
    first.resize(nr + 1); off.resize(nu + 1); len.resize(nu + 1); arena.resize(ab + 1);
    rc = otg_parse_bed_units(bed_path, first.data(), first.size(), &nr, off.data(), len.data(), nu, &nu, arena.data(), ab, &ab);
    if (rc != OTG_OK) return rc;
    if (nr != bed.beds.size()) return otg_fail(nullptr, OTG_ERR_FATAL, "%s: the two BED readers disagree on %s", who, bed_path);
    std::string name;
    for (uint32_t r = 0; r < bed.beds.size(); ++r) {
      name.clear();
      otg_region_name(name, bed.chr_arena.data() + bed.beds[r].chr_off, bed.beds[r].chr_len, bed.beds[r].start, bed.beds[r].end);
      by_region.emplace(name, r);
    }
    return OTG_OK;
  }
  // the units [u0, u1) of the record of this region; none: u0 = u1 = 0
  void units_of(const std::string& region, uint64_t* u0, uint64_t* u1) const
  {
    const auto it = by_region.find(region);
    *u0 = it == by_region.end() ? 0 : first[it->second];
    *u1 = it == by_region.end() ? 0 : first[it->second + 1];
  }
};

} // namespace

extern "C" {

static int tract_cli_args(const otg_tract_params& q);
// otg_assemble_files, and with `spread` otg_spread_files: the same batch loop, the spread call behind the hot path, spread rows for records
static int assemble_files_impl(const char* who, const otg_assemble_job* job, const SpreadSets* spread, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->bam_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL job, writer, BAM or BED path", who);
  if (job->n_devices < 0 || (job->n_devices > 0 && !job->devices)) return otg_fail(nullptr, OTG_ERR_ARG, "%s: bad device list", who);
  const auto t_all = Clock::now();
  g_trace_t0 = t_all;
  AssembleShared A;
  A.j = job;
  A.spread = spread;
  Job& J = A.J;
  int rc = load_bed(job->bed_path, A.bed);
  if (rc != OTG_OK) return rc;
  const uint32_t R = (uint32_t)A.bed.beds.size();
  J.st.n_regions = R;
  if (spread && spread->set_of.size() != R) return otg_fail(nullptr, OTG_ERR_FATAL, "%s: the two BED readers disagree on %s", who, job->bed_path);
  rc = open_bam(job->bam_path, A.bam);
  if (rc != OTG_OK) return rc;
  if (job->fasta_path && job->fasta_path[0]) {
    rc = open_fasta(job->fasta_path, A.fasta);
    if (rc != OTG_OK) return rc;
  }
  // SAM header; FASTA output and spread rows have none
  if (!job->is_fasta && !spread) {
    std::string hdr;
    rc = sam_header_text(A.bam.get(), job->read_group ? job->read_group : "", job->ingest.offset_l, job->ingest.offset_r, hdr);
    if (rc != OTG_OK) return rc;
    if (write(user, hdr.data(), hdr.size()) != 0) return otg_fail(nullptr, OTG_ERR_ARG, "%s: the writer failed", who);
    J.st.output_bytes += hdr.size();
  }
  J.st.n_devices = run_shards<std::string>(
      J, job->devices, job->n_devices, R, job->batch_regions, job->ingest.threads,
      [&](int device, uint32_t a, uint32_t b, int threads, OrderedOutput<std::string>& out) { shard_worker(A, device, a, b, threads, out); },
      [&](uint32_t k, const std::string& text) {
        const auto tw = Clock::now();
        if (!text.empty() && write(user, text.data(), text.size()) != 0) { J.fail(OTG_ERR_ARG, "the writer failed"); return false; }
        trace("write", k, (uint32_t)(text.size() >> 10), tw);
        J.st.output_bytes += text.size();
        return true;
      });
  trace("job", 0, R, t_all);
  J.st.ms_total = ms_since(t_all);
  if (stats) *stats = J.st;
  if (J.rc.load() != OTG_OK) return otg_fail(nullptr, J.rc.load(), "%s: %s", who, J.err.c_str());
  return OTG_OK;
}

int otg_assemble_files(const otg_assemble_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  return assemble_files_impl("otg_assemble_files", job, nullptr, write, user, stats);
}

int otg_spread_files(const otg_spread_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  const char* who = "otg_spread_files";
  if (!job || !write || !job->assemble.bam_path || !job->assemble.bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL job, writer, BAM or BED path", who);
  if (job->assemble.reads_only || job->assemble.is_fasta) return otg_fail(nullptr, OTG_ERR_ARG, "%s: --reads-only and --fasta do not apply to spread rows", who);
  SpreadSets S;
  S.q = otg_tract_params{job->match, job->mismatch, job->indel, job->min_score};
  if (int rc = tract_cli_args(S.q)) return rc;
  UnitCatalogue cat;
  if (int rc = cat.load(who, job->assemble.bed_path)) return rc;
  // a set per record with units: the records' stretches of the unit list are contiguous, so the non-empty ones tile it
  const size_t R = cat.first.size() - 1;
  S.set_of.assign(R, OTG_SPREAD_NONE);
  for (size_t r = 0; r < R; ++r)
    if (cat.first[r + 1] > cat.first[r]) { S.set_of[r] = (uint32_t)S.set_first.size(); S.set_first.push_back(cat.first[r]); }
  S.set_first.push_back(cat.first[R]);
  S.unit_off = cat.off; S.unit_len = cat.len; S.arena = cat.arena;
  S.unit_off.resize((size_t)cat.first[R] + 1); S.unit_len.resize((size_t)cat.first[R] + 1);
  S.unit_bytes = S.arena.size() - 1;
  return assemble_files_impl(who, &job->assemble, &S, write, user, stats);
}

// `otter compare` from files to text — compare() (src/compare.cpp:68-150).  Two batches in flight: while the pairs of one are aligned on the
// device and emitted, the next one is ingested (both BAMs) on a host thread.
int otg_compare_files(const otg_compare_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->truth_bam_path || !job->query_bam_path || !job->bed_path)
    return otg_fail(nullptr, OTG_ERR_ARG, "otg_compare_files: NULL job, writer, BAM or BED path");
  const auto t_all = Clock::now();
  otg_job_stats st{};
  Bed bed;
  int rc = load_bed(job->bed_path, bed);
  if (rc != OTG_OK) return rc;
  const std::vector<otg_bed>& beds = bed.beds; const std::vector<char>& chr_arena = bed.chr_arena;
  st.n_regions = (uint32_t)beds.size();
  BamPtr bt, bq;
  rc = open_bam(job->truth_bam_path, bt);
  if (rc != OTG_OK) return rc;
  rc = open_bam(job->query_bam_path, bq);
  if (rc != OTG_OK) return rc;
  // sample2index (src/compare.cpp:77-88): the first read group of each BAM (SampleIndex::init)
  std::string s0, s1;
  for (int side = 0; side < 2; ++side) {
    otg_bam* b = side ? bq.get() : bt.get();
    rc = otg_bam_sample_index(b, nullptr, nullptr, nullptr);
    if (rc != OTG_OK) return rc;
    (side ? s1 : s0) = otg_bam_sample(b, 0);
  }
  const PooledCtx ctx = acquire_ctx(job->device);
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_compare_files: %s", last_err().c_str());
  const uint32_t per = job->batch_regions ? job->batch_regions : 1024u;
  const int threads = job->threads > 0 ? job->threads : 1;
  struct Side {
    std::vector<uint8_t> arena; std::vector<otg_allele> alleles; std::vector<uint32_t> first;
    std::vector<int32_t> sp; std::vector<uint32_t> sp_first; std::string warn;
    uint32_t na = 0, ns = 0; uint64_t used = 0;
  };
  struct CmpBatch { Side side[2]; uint32_t f = 0, n = 0; int rc = OTG_OK; double ms = 0; std::string err; };
  auto ingest_into = [&](CmpBatch& B, uint32_t f) {
    B.f = f; B.n = std::min<uint32_t>(per, (uint32_t)beds.size() - f);
    const auto t0 = Clock::now();
    B.rc = OTG_OK;
    for (int side = 0; side < 2 && B.rc == OTG_OK; ++side) {
      Side& S = B.side[side];
      S.first.assign((size_t)B.n + 1, 0); S.sp_first.assign((size_t)B.n + 1, 0);
      size_t cap_al = std::max<size_t>(S.alleles.size(), (size_t)B.n * 16 + 64), cap_ar = std::max<size_t>(S.arena.size(), (size_t)B.n * 16 * 1024 + 4096);
      size_t cap_sp = std::max<size_t>(S.sp.size(), (size_t)B.n * 16 + 64), cap_w = std::max<size_t>(S.warn.size(), (size_t)B.n * 96 + 64);
      for (int attempt = 0; attempt < 4; ++attempt) {
        S.alleles.resize(cap_al); S.arena.resize(cap_ar); S.sp.resize(cap_sp); S.warn.resize(cap_w);
        S.na = 0; S.used = 0; S.ns = 0; uint64_t wl = 0;
        B.rc = otg_ingest_compare_alleles(side ? bq.get() : bt.get(), s0.c_str(), s1.c_str(), side ? 0 : 1, beds.data() + f, chr_arena.data(), B.n, threads,
                                          S.arena.data(), S.arena.size(), &S.used, S.alleles.data(), (uint32_t)S.alleles.size(), &S.na, S.first.data(),
                                          S.sp.data(), (uint32_t)S.sp.size(), &S.ns, S.sp_first.data(), &S.warn[0], S.warn.size(), &wl);
        if (B.rc != OTG_ERR_CAPACITY) { S.warn.resize(B.rc == OTG_OK ? wl : 0); break; }
        cap_al = (size_t)S.na + 64; cap_ar = (size_t)S.used + 4096; cap_sp = (size_t)S.ns + 64; cap_w = (size_t)wl + 64;
      }
      if (B.rc != OTG_OK) B.err = last_err();
    }
    B.ms = ms_since(t0);
  };
  std::vector<otg_align_task> tasks; std::vector<uint8_t> seqs; std::vector<uint64_t> pair_first;
  std::vector<double> pedit, pops; std::vector<int64_t> pair_task;
  std::vector<int32_t> scores; std::vector<uint32_t> clen;
  std::string text, wtext;
  const uint32_t n_beds = (uint32_t)beds.size();
  auto emit_warn = [&](const std::string& w) { return w.empty() || !job->warn || job->warn(job->warn_user, w.data(), w.size()) == 0; };
  TwoInFlight<CmpBatch> flight;
  if (n_beds) ingest_into(flight.current(), 0);
  for (uint32_t f = 0; f < n_beds; f += per, flight.advance()) {
    const CmpBatch& B = flight.current();
    if (B.rc != OTG_OK) return otg_fail(nullptr, B.rc, "otg_compare_files: %s", B.err.c_str());
    if (f + per < n_beds) flight.prefetch([&, f](CmpBatch& N) { ingest_into(N, f + per); });
    const Side& T = B.side[0]; const Side& Q = B.side[1];
    const uint32_t n = B.n;
    st.ms_ingest += B.ms; st.n_alleles += T.na + Q.na; st.input_bytes += T.used + Q.used;
    auto t0 = Clock::now();
    // the pairs of every compared region (get_distances, src/compare.cpp:52-63): pattern = the longer allele, ties -> the query
    tasks.clear(); seqs.clear(); pair_first.assign((size_t)n + 1, 0); pair_task.clear();
    auto add_seq = [&](const uint8_t* p, uint32_t l) { const uint64_t o = seqs.size(); seqs.insert(seqs.end(), p, p + l); return o; };
    for (uint32_t r = 0; r < n; ++r) {
      pair_first[r] = pair_task.size();
      const uint32_t nt = T.first[r + 1] - T.first[r], nq0 = Q.first[r + 1] - Q.first[r];
      if (!otg_compare_n_pairs(nt, nq0)) continue;
      const uint32_t nq = nq0 == 1 ? 2 : nq0;
      for (uint32_t i = 0; i < nt; ++i) {
        const otg_allele& ta = T.alleles[T.first[r] + i];
        for (uint32_t j = 0; j < nq; ++j) {
          const otg_allele& qa = Q.alleles[Q.first[r] + (nq0 == 1 ? 0 : j)];
          double e, o;
          if (otg_compare_special(T.arena.data() + ta.seq_off, ta.seq_len, Q.arena.data() + qa.seq_off, qa.seq_len, &e, &o)) { pair_task.push_back(-1); continue; }
          otg_align_task t; memset(&t, 0, sizeof(t));
          const bool tp = ta.seq_len > qa.seq_len;
          const otg_allele& pa = tp ? ta : qa; const otg_allele& xa = tp ? qa : ta;
          t.pattern_off = add_seq((tp ? T : Q).arena.data() + pa.seq_off, pa.seq_len); t.pattern_len = pa.seq_len;
          t.text_off = add_seq((tp ? Q : T).arena.data() + xa.seq_off, xa.seq_len); t.text_len = xa.seq_len;
          pair_task.push_back((int64_t)tasks.size());
          tasks.push_back(t);
        }
      }
    }
    pair_first[n] = pair_task.size();
    seqs.resize(seqs.size() + 64, 0);
    scores.assign(tasks.size(), 0); clen.assign(tasks.size(), 0);
    if (!tasks.empty()) {
      uint64_t used = 0;
      if (job->heuristic == OTG_HEURISTIC_NONE)
        rc = otg_edit_align_batch(ctx.get(), seqs.data(), seqs.size(), tasks.data(), (uint32_t)tasks.size(), scores.data(), nullptr, clen.data(), nullptr, 0, &used);
      else
        rc = otg_edit_align_heur_batch(ctx.get(), seqs.data(), seqs.size(), tasks.data(), (uint32_t)tasks.size(), job->heuristic, job->heur_min_wavefront_length,
                                       job->heur_max_distance_threshold, job->heur_steps_between_cutoffs, scores.data(), nullptr, clen.data(), nullptr, 0, &used, nullptr);
      if (rc != OTG_OK) return otg_fail(nullptr, rc, "otg_compare_files: %s", ctx_err(ctx.get()).c_str());
    }
    pedit.assign(pair_task.size(), 0.0); pops.assign(pair_task.size(), 0.0);
    for (size_t p = 0; p < pair_task.size(); ++p)
      if (pair_task[p] >= 0) { pedit[p] = (double)scores[(size_t)pair_task[p]]; pops[p] = (double)clen[(size_t)pair_task[p]]; }
    st.n_reads += tasks.size();
    st.ms_hot_path += ms_since(t0);
    t0 = Clock::now();
    uint64_t wneed = 0;
    otg_compare_counts cc{};
    rc = sized_text(text, [&](char* buf, uint64_t cap, uint64_t* need) {
      wtext.resize(wneed);                  // the warnings go by the same protocol: empty on the sizing call, then the size that call reported
      return otg_compare_emit(beds.data() + f, chr_arena.data(), n, T.first.data(), T.alleles.data(), T.arena.data(), T.sp_first.data(), T.sp.data(),
                              Q.first.data(), Q.alleles.data(), Q.arena.data(), pair_first.data(), pedit.data(), pops.data(), buf, cap, need,
                              wneed ? &wtext[0] : nullptr, wneed, &wneed, &cc);
    });
    if (rc != OTG_OK) return rc;
    st.ms_emit += ms_since(t0);
    st.n_regions_ok += cc.n_compared;
    st.n_regions_skipped += cc.skip_many_truth + cc.skip_one_truth + cc.skip_no_truth + cc.skip_no_query;
    if (!emit_warn(T.warn) || !emit_warn(Q.warn) || !emit_warn(wtext)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_compare_files: the warning writer failed");
    if (!text.empty() && write(user, text.data(), text.size()) != 0) return otg_fail(nullptr, OTG_ERR_ARG, "otg_compare_files: the writer failed");
    st.output_bytes += text.size();
  }
  st.ms_total = ms_since(t_all); st.n_devices = 1;
  if (stats) *stats = st;
  return OTG_OK;
}

// `otter vcf2mat` from a file to text — vcf2mat() (src/vcf2mat.cpp:48-77), on vcf_allele_job.  Batches are bounded by alleles and by the
// bytes of their rows (a row is 4^k+1 doubles: 134 MB at k = 12).
int otg_vcf2mat_files(const otg_vcf2mat_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_vcf2mat_files: NULL job, writer, VCF or BED path");
  const int k = job->k;
  if (k < 1 || k > OTG_KMER_MAX) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--kmer-size' (%d). Needs to be 1 <= x <= %d.", k, OTG_KMER_MAX);
  const uint64_t bins = (1ull << (2 * k)) + 1;
  // alleles per batch: at most 1 GiB of rows on the host and what the device workspace of otg_kmer_usage_batch holds (k >= 8: + u32 histograms)
  const uint64_t dev_row = bins * 8 + (k >= 8 ? bins * 4 : 0);
  uint64_t per = job->batch_alleles ? job->batch_alleles : std::min<uint64_t>(65536, std::max<uint64_t>(1, (1ull << 30) / (bins * 8)));
  per = std::min<uint64_t>(per, (4ull << 30) / dev_row);
  std::vector<double> usage, gc, hsd;
  return vcf_allele_job("otg_vcf2mat_files", job->vcf_path, job->bed_path, job->device, per, job->threads, write, user, stats,
    [&](otg_ctx* ctx, const VcfBatch& B) {
      usage.resize((size_t)B.na * bins); gc.resize(B.na); hsd.resize(B.na);
      return otg_kmer_usage_batch(ctx, B.seqs.data(), B.au, B.off.data(), B.len.data(), B.na, k, usage.data(), gc.data(), hsd.data());
    },
    [&](std::string& o, const VcfBatch& B, uint32_t r0, uint32_t nr) {
      otg_vcf2mat_rows(o, B.rec.data() + r0, nr, B.regions.data(), B.len.data(), k, usage.data(), gc.data(), hsd.data());
    });
}

// The motif rows of a VCF's alleles (otg_motif_batch), on vcf_allele_job: the reader, the batching and the threaded emit of otg_vcf2mat_files.
int otg_motifs_files(const otg_motifs_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_motifs_files: NULL job, writer, VCF or BED path");
  const uint32_t max_period = job->max_period, slack = job->slack;
  if (int rc = motif_cli_args(max_period, slack)) return rc;
  std::vector<otg_motif> motifs;
  std::vector<uint8_t> units;
  uint32_t stride = 1;
  return vcf_allele_job("otg_motifs_files", job->vcf_path, job->bed_path, job->device, job->batch_alleles ? job->batch_alleles : 65536, job->threads, write, user, stats,
    [&](otg_ctx* ctx, const VcfBatch& B) {
      stride = motif_unit_stride(B.len.data(), B.na, max_period);
      motifs.resize(B.na); units.resize((size_t)B.na * stride);
      return otg_motif_batch(ctx, B.seqs.data(), B.au, B.off.data(), B.len.data(), B.na, max_period, slack, motifs.data(), units.data(), stride);
    },
    [&](std::string& o, const VcfBatch& B, uint32_t r0, uint32_t nr) {
      otg_motif_rows(o, B.rec.data() + r0, nr, B.regions.data(), B.len.data(), motifs.data(), units.data(), stride);
    });
}

// The repeat-structure rows of a VCF's alleles (otg_repeat_batch, otg_repeat_collect), on vcf_allele_job as otg_motifs_files.
int otg_repeats_files(const otg_repeats_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_repeats_files: NULL job, writer, VCF or BED path");
  const uint32_t max_period = job->max_period, min_copies = job->min_copies, min_span = job->min_span;
  if (max_period < 1 || max_period > OTG_REPEAT_MAX_PERIOD)
    return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--max-period' (%u). Needs to be 1 <= x <= %d.", max_period, OTG_REPEAT_MAX_PERIOD);
  if (min_copies < 2 || min_copies > 1024) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--min-copies' (%u). Needs to be 2 <= x <= 1024.", min_copies);
  if (min_span < 2 || min_span > 65535) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--min-span' (%u). Needs to be 2 <= x <= 65535.", min_span);
  std::vector<otg_repeat_sum> sums;
  std::vector<uint64_t> seg_off;
  std::vector<otg_repeat_seg> segs;
  return vcf_allele_job("otg_repeats_files", job->vcf_path, job->bed_path, job->device, job->batch_alleles ? job->batch_alleles : 65536, job->threads, write, user, stats,
    [&](otg_ctx* ctx, const VcfBatch& B) {
      sums.resize(B.na); seg_off.resize((size_t)B.na + 1);
      uint64_t total = 0;
      if (int rc = otg_repeat_batch(ctx, B.seqs.data(), B.au, B.off.data(), B.len.data(), B.na, max_period, min_copies, min_span, sums.data(), seg_off.data(), &total)) return rc;
      segs.resize(total);
      return B.na ? otg_repeat_collect(ctx, segs.data(), total) : OTG_OK;
    },
    [&](std::string& o, const VcfBatch& B, uint32_t r0, uint32_t nr) {
      otg_repeat_rows(o, B.rec.data() + r0, nr, B.regions.data(), B.seqs.data(), B.off.data(), B.len.data(), sums.data(), seg_off.data(), segs.data());
    });
}

// The rows of a VCF's alleles against the units of a tandem-repeat catalogue, on vcf_allele_job as otg_motifs_files: what otg_copies_files and
// otg_tracts_files share.  A batch makes up to two device passes: the alleles of catalogue regions against their units (batch_fn, only the
// units the batch uses are uploaded), the others through otg_motif_batch and motifs_fn, whose units never leave the device in between.
// Rec = the operator's record (zero: the record of a task that was not run); rows_fn = its row text.
extern "C++" {
template <typename Rec, typename BatchFn, typename MotifsFn, typename RowsFn>
int catalogue_units_job(const char* who, const char* vcf_path, const char* bed_path, uint32_t max_period, uint32_t slack, int32_t device, uint32_t batch_alleles,
                        int32_t threads, otg_write_fn write, void* user, otg_job_stats* stats, BatchFn batch_fn, MotifsFn motifs_fn, RowsFn rows_fn)
{
  if (int rc = motif_cli_args(max_period, slack)) return rc;
  UnitCatalogue cat;
  if (int rc = cat.load(who, bed_path)) return rc;
  // per batch: the tasks in file order (allele a: task_first[a] .. task_first[a + 1]) and where each one's unit and record lie
  std::vector<uint64_t> task_first, unit_off, m_off, b_uoff;
  std::vector<uint32_t> unit_len, m_len, b_ulen, b_tseq, b_tunit, b_task, m_task;
  std::vector<uint8_t> source, units, b_units, m_units;
  std::vector<Rec> aligned, part;
  std::vector<otg_motif> motifs;
  return vcf_allele_job(who, vcf_path, bed_path, device, batch_alleles ? batch_alleles : 65536, threads, write, user, stats,
    [&](otg_ctx* ctx, const VcfBatch& B) {
      task_first.assign((size_t)B.na + 1, 0);
      unit_off.clear(); unit_len.clear(); source.clear(); units.clear();
      b_uoff.clear(); b_ulen.clear(); b_units.clear(); b_tseq.clear(); b_tunit.clear(); b_task.clear();
      m_off.clear(); m_len.clear(); m_task.clear();
      std::string name;
      for (uint32_t r = 0; r < B.nr; ++r) {
        const otg_vcf_record& R = B.rec[r];
        name.assign(B.regions.data() + R.region_off, R.region_len);
        uint64_t u0, u1;
        cat.units_of(name, &u0, &u1);
        const uint32_t bu0 = (uint32_t)b_ulen.size();
        for (uint64_t k = u0; k < u1; ++k) {                       // the record's units, once per record
          b_uoff.push_back(b_units.size()); b_ulen.push_back(cat.len[k]);
          b_units.insert(b_units.end(), cat.arena.begin() + cat.off[k], cat.arena.begin() + cat.off[k] + cat.len[k]);
        }
        for (uint32_t i = 0; i < R.n_alleles; ++i) {
          const uint32_t a = R.first_allele + i;
          task_first[a] = source.size();
          if (u1 > u0) {
            for (uint64_t k = u0; k < u1; ++k) {
              b_task.push_back((uint32_t)source.size()); b_tseq.push_back(a); b_tunit.push_back(bu0 + (uint32_t)(k - u0));
              source.push_back(OTG_UNITALIGN_SOURCE_BED);
              unit_off.push_back(units.size()); unit_len.push_back(cat.len[k]);
              units.insert(units.end(), cat.arena.begin() + cat.off[k], cat.arena.begin() + cat.off[k] + cat.len[k]);
            }
          } else {
            m_task.push_back((uint32_t)source.size()); m_off.push_back(B.off[a]); m_len.push_back(B.len[a]);
            source.push_back(OTG_UNITALIGN_SOURCE_MOTIF);
            unit_off.push_back(0); unit_len.push_back(0);         // filled in behind the motif pass
          }
        }
      }
      task_first[B.na] = source.size();
      aligned.assign(source.size(), Rec{});
      if (!b_task.empty()) {
        part.resize(b_task.size());
        if (int rc = batch_fn(ctx, B.seqs.data(), B.au, B.off.data(), B.len.data(), B.na, b_units.data(), b_units.size(), b_uoff.data(), b_ulen.data(),
                              (uint32_t)b_ulen.size(), b_tseq.data(), b_tunit.data(), (uint32_t)b_task.size(), part.data())) return rc;
        for (size_t k = 0; k < b_task.size(); ++k) aligned[b_task[k]] = part[k];
      }
      if (!m_task.empty()) {
        const uint32_t nm = (uint32_t)m_task.size();
        const uint32_t stride = motif_unit_stride(m_len.data(), nm, max_period);
        motifs.resize(nm); m_units.resize((size_t)nm * stride); part.resize(nm);
        if (int rc = otg_motif_batch(ctx, B.seqs.data(), B.au, m_off.data(), m_len.data(), nm, max_period, slack, motifs.data(), m_units.data(), stride)) return rc;
        if (int rc = motifs_fn(ctx, part.data())) return rc;
        for (uint32_t k = 0; k < nm; ++k) {
          const uint32_t t = m_task[k], p = motifs[k].period;
          aligned[t] = part[k];
          unit_off[t] = units.size(); unit_len[t] = p;
          units.insert(units.end(), m_units.begin() + (size_t)k * stride, m_units.begin() + (size_t)k * stride + p);
        }
      }
      units.push_back(0);                                          // (never empty: the emit takes its address)
      return (int)OTG_OK;
    },
    [&](std::string& o, const VcfBatch& B, uint32_t r0, uint32_t nr) {
      rows_fn(o, B.rec.data() + r0, nr, B.regions.data(), B.len.data(), task_first.data(), source.data(), units.data(), unit_off.data(), unit_len.data(), aligned.data());
    });
}
} // extern "C++"

// Copy numbers of a VCF's alleles against a tandem-repeat catalogue: otg_unitalign_batch and otg_unitalign_motifs on catalogue_units_job.
int otg_copies_files(const otg_copies_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_copies_files: NULL job, writer, VCF or BED path");
  return catalogue_units_job<otg_unitalign>("otg_copies_files", job->vcf_path, job->bed_path, job->max_period, job->slack, job->device, job->batch_alleles, job->threads,
                                            write, user, stats, otg_unitalign_batch, otg_unitalign_motifs, otg_unitalign_rows);
}

// the refusals of --scores and --min-score that otter_tracts and otter_loci share, with the message the tools print
static int tract_cli_args(const otg_tract_params& q)
{
  if (q.match < 1 || q.match > 16 || q.mismatch < 1 || q.mismatch > 64 || q.indel < 1 || q.indel > 64)
    return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--scores' (%u,%u,%u). Needs to be 1 <= match <= 16, 1 <= mismatch <= 64, 1 <= indel <= 64.", q.match, q.mismatch,
                    q.indel);
  if (q.min_score > (1u << 24)) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--min-score' (%u). Needs to be 0 <= x <= %u.", q.min_score, 1u << 24);
  return OTG_OK;
}

// The tracts of a VCF's alleles against a tandem-repeat catalogue: otg_tract_batch and otg_tract_motifs on catalogue_units_job, with the scores.
int otg_tracts_files(const otg_tracts_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_tracts_files: NULL job, writer, VCF or BED path");
  const otg_tract_params q{job->match, job->mismatch, job->indel, job->min_score};
  if (int rc = tract_cli_args(q)) return rc;
  return catalogue_units_job<otg_tract>(
      "otg_tracts_files", job->vcf_path, job->bed_path, job->max_period, job->slack, job->device, job->batch_alleles, job->threads, write, user, stats,
      [&](otg_ctx* ctx, const uint8_t* seqs, uint64_t au, const uint64_t* off, const uint32_t* len, uint32_t na, const uint8_t* ua, uint64_t ub, const uint64_t* uoff,
          const uint32_t* ulen, uint32_t nu, const uint32_t* ts, const uint32_t* tu, uint32_t nt, otg_tract* out) {
        return otg_tract_batch(ctx, seqs, au, off, len, na, ua, ub, uoff, ulen, nu, ts, tu, nt, &q, out);
      },
      [&](otg_ctx* ctx, otg_tract* out) { return otg_tract_motifs(ctx, &q, out); }, otg_tract_rows);
}

// The rows of a VCF's alleles against the unit sets of a tandem-repeat catalogue, on vcf_allele_job as otg_copies_files: what
// otg_unitparse_files and otg_loci_files share.  One task per allele of a catalogue region with units (batch_fn, only the sets the batch
// uses are uploaded; collect_fn brings its segments); the others get the row without units.  Rec = the operator's record (zero: an allele
// that was not a task); rows_fn = its row text.
extern "C++" {
// The unit sets and tasks of one batch, as unit_sets_job and otg_units_loci_files build them: one set per record with units, one task per allele
// of such a record, in allele order.  add() is the only place where a region's units are refused (more than eight, the lane budget, an empty
// unit): these are the set refusals of otg_unitparse_check, which the resident entries called with these arrays do not repeat; the ranges of
// the unit bytes hold by construction (every unit is copied into `units` here).
struct BatchSets {
  std::vector<uint64_t> set_first, uoff;
  std::vector<uint32_t> ulen, allele_set, tseq, tset;
  std::vector<uint8_t> units;
  void begin(uint32_t na)
  {
    set_first.assign(1, 0); uoff.clear(); ulen.clear(); units.clear(); tseq.clear(); tset.clear();
    allele_set.assign(na, OTG_UNITPARSE_NO_SET);
  }
  // units [u0, u1) of (arena, off, len) become the set of record R (region `name`); u0 == u1: the record has none
  int add(otg_ctx* ctx, const std::string& name, const otg_vcf_record& R, const uint8_t* arena, const uint64_t* off, const uint32_t* len, uint64_t u0, uint64_t u1)
  {
    if (u1 == u0) return OTG_OK;
    if (u1 - u0 > OTG_UNITPARSE_MAX_UNITS)
      return otg_fail(ctx, OTG_ERR_ARG, "%s has %llu units in the catalogue, at most %d", name.c_str(), (unsigned long long)(u1 - u0),
                      OTG_UNITPARSE_MAX_UNITS);
    if (otg_unitparse_core::up_class(len + u0, (uint32_t)(u1 - u0)) == otg_unitparse_core::UP_NO_CLASS)
      return otg_fail(ctx, OTG_ERR_ARG, "the units of %s do not fit one wave (%u lanes at four positions each, at most %d)", name.c_str(),
                      otg_unitparse_core::up_lanes(len + u0, (uint32_t)(u1 - u0), 4u), OTG_UNITPARSE_MAX_LANES);
    const uint32_t q = (uint32_t)set_first.size() - 1u;
    for (uint64_t k = u0; k < u1; ++k) {
      if (len[k] == 0u || len[k] > OTG_UNITALIGN_MAX_UNIT)
        return otg_fail(ctx, OTG_ERR_ARG, "%s has a unit of %u bytes, 1 to %d are allowed", name.c_str(), len[k], OTG_UNITALIGN_MAX_UNIT);
      uoff.push_back(units.size()); ulen.push_back(len[k]);
      units.insert(units.end(), arena + off[k], arena + off[k] + len[k]);
    }
    set_first.push_back(ulen.size());
    for (uint32_t i = 0; i < R.n_alleles; ++i) { allele_set[R.first_allele + i] = q; tseq.push_back(R.first_allele + i); tset.push_back(q); }
    return OTG_OK;
  }
  void finish() { units.push_back(0); uoff.push_back(0); ulen.push_back(0); }      // (never empty: the emit takes their addresses)
  uint32_t n_units() const { return (uint32_t)ulen.size() - 1u; }
  uint32_t n_sets() const { return (uint32_t)set_first.size() - 1u; }
  // the tasks are the alleles with units, in allele order: their records and segment offsets spread over all na alleles
  template <typename Rec>
  void spread(uint32_t na, const std::vector<Rec>& t_sums, const std::vector<uint64_t>& t_seg_off, uint64_t total, std::vector<Rec>& sums, std::vector<uint64_t>& seg_off) const
  {
    sums.assign(na, Rec{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}); seg_off.assign((size_t)na + 1, 0);
    const uint32_t nt = (uint32_t)tseq.size();
    uint32_t cur = 0;
    for (uint32_t a = 0; a < na; ++a) {
      seg_off[a] = t_seg_off[cur];
      if (cur < nt && tseq[cur] == a) sums[a] = t_sums[cur++];
    }
    seg_off[na] = total;
  }
};

template <typename Rec, typename BatchFn, typename CollectFn, typename RowsFn>
int unit_sets_job(const char* who, const char* vcf_path, const char* bed_path, int32_t device, uint32_t batch_alleles, int32_t threads, otg_write_fn write, void* user,
                  otg_job_stats* stats, BatchFn batch_fn, CollectFn collect_fn, RowsFn rows_fn)
{
  UnitCatalogue cat;
  if (int rc = cat.load(who, bed_path)) return rc;
  // per batch: the sets and tasks (BatchSets); the results per allele, in file order
  BatchSets S;
  std::vector<uint64_t> seg_off, t_seg_off;
  std::vector<Rec> sums, t_sums;
  std::vector<otg_unitparse_seg> segs;
  return vcf_allele_job(who, vcf_path, bed_path, device, batch_alleles ? batch_alleles : 65536, threads, write, user, stats,
    [&](otg_ctx* ctx, const VcfBatch& B) {
      S.begin(B.na);
      std::string name;
      for (uint32_t r = 0; r < B.nr; ++r) {
        const otg_vcf_record& R = B.rec[r];
        name.assign(B.regions.data() + R.region_off, R.region_len);
        uint64_t u0, u1;
        cat.units_of(name, &u0, &u1);
        if (int rc = S.add(ctx, name, R, cat.arena.data(), cat.off.data(), cat.len.data(), u0, u1)) return rc;
      }
      S.finish();
      const uint32_t nt = (uint32_t)S.tseq.size();
      t_sums.resize(nt); t_seg_off.assign((size_t)nt + 1, 0);
      uint64_t total = 0;
      if (nt) {
        if (int rc = batch_fn(ctx, B.seqs.data(), B.au, B.off.data(), B.len.data(), B.na, S.units.data(), S.units.size() - 1, S.uoff.data(), S.ulen.data(), S.n_units(),
                              S.set_first.data(), S.n_sets(), S.tseq.data(), S.tset.data(), nt, t_sums.data(), t_seg_off.data(), &total)) return rc;
      }
      segs.resize(total + 1);
      if (total)
        if (int rc = collect_fn(ctx, segs.data(), total)) return rc;
      S.spread(B.na, t_sums, t_seg_off, total, sums, seg_off);
      return (int)OTG_OK;
    },
    [&](std::string& o, const VcfBatch& B, uint32_t r0, uint32_t nr) {
      rows_fn(o, B.rec.data() + r0, nr, B.regions.data(), B.len.data(), S.allele_set.data(), S.set_first.data(), S.units.data(), S.uoff.data(), S.ulen.data(), sums.data(),
              seg_off.data(), segs.data());
    });
}
}

// The joint parse of a VCF's alleles against the unit sets of a tandem-repeat catalogue: otg_unitparse_batch on unit_sets_job.
int otg_unitparse_files(const otg_unitparse_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitparse_files: NULL job, writer, VCF or BED path");
  return unit_sets_job<otg_unitparse_sum>("otg_unitparse_files", job->vcf_path, job->bed_path, job->device, job->batch_alleles, job->threads, write, user, stats,
                                          otg_unitparse_batch, otg_unitparse_collect, otg_unitparse_rows);
}

// The locus mode over a VCF's alleles: otg_locus_batch on unit_sets_job, with the scores.
int otg_loci_files(const otg_loci_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_loci_files: NULL job, writer, VCF or BED path");
  const otg_tract_params q{job->match, job->mismatch, job->indel, job->min_score};
  if (int rc = tract_cli_args(q)) return rc;
  return unit_sets_job<otg_locus>(
      "otg_loci_files", job->vcf_path, job->bed_path, job->device, job->batch_alleles, job->threads, write, user, stats,
      [&](otg_ctx* ctx, const uint8_t* seqs, uint64_t au, const uint64_t* off, const uint32_t* len, uint32_t na, const uint8_t* ua, uint64_t ub, const uint64_t* uoff,
          const uint32_t* ulen, uint32_t nu, const uint64_t* sf, uint32_t ns, const uint32_t* ts, const uint32_t* tq, uint32_t nt, otg_locus* out, uint64_t* seg_off,
          uint64_t* total) { return otg_locus_batch(ctx, seqs, au, off, len, na, ua, ub, uoff, ulen, nu, sf, ns, ts, tq, nt, &q, out, seg_off, total); },
      otg_locus_collect, otg_locus_rows);
}

// the parameters of a discovery job, refused in the command line's words
static int units_cli_args(const otg_units_job& J)
{
  if (J.max_period < 1 || J.max_period > OTG_REPEAT_MAX_PERIOD)
    return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--max-period' (%u). Needs to be 1 <= x <= %d.", J.max_period, OTG_REPEAT_MAX_PERIOD);
  if (J.min_copies < 2 || J.min_copies > 1024) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--min-copies' (%u). Needs to be 2 <= x <= 1024.", J.min_copies);
  if (J.min_span < 2 || J.min_span > 65535) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--min-span' (%u). Needs to be 2 <= x <= 65535.", J.min_span);
  if (J.min_bases < 1 || J.min_bases > (1u << 24))
    return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--min-bases' (%u). Needs to be 1 <= x <= %u.", J.min_bases, 1u << 24);
  if (J.min_share > 1000) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--min-share' (%u). Needs to be 0 <= x <= 1000.", J.min_share);
  if (J.redundant > 1000) return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--redundant' (%u). Needs to be 0 <= x <= 1000.", J.redundant);
  return OTG_OK;
}

// The unit sets of a VCF's regions as a catalogue BED: otg_repeat_batch and otg_unitset_repeats on vcf_allele_job, one group per VCF record.
// A batch ends at a record boundary (otg_vcf_read_alleles delivers whole records; a record larger than the batch runs alone), so the alleles
// of a region are always in one discovery call.
int otg_units_files(const otg_units_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->vcf_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_units_files: NULL job, writer, VCF or BED path");
  if (int rc = units_cli_args(*job)) return rc;
  const uint32_t max_period = job->max_period, min_copies = job->min_copies, min_span = job->min_span;
  const otg_unitset_params q{job->min_bases, job->min_share, job->redundant, 0u};
  Bed bed;
  if (int rc = load_bed(job->bed_path, bed)) return rc;
  std::map<std::string, uint32_t> by_region;                       // the first record of a region wins
  {
    std::string name;
    for (uint32_t r = 0; r < bed.beds.size(); ++r) {
      name.clear();
      otg_region_name(name, bed.chr_arena.data() + bed.beds[r].chr_off, bed.beds[r].chr_len, bed.beds[r].start, bed.beds[r].end);
      by_region.emplace(name, r);
    }
  }
  std::vector<uint32_t> group_first, rec_bed, unit_len;
  std::vector<otg_unitset> sets;
  std::vector<uint64_t> set_first, unit_off;
  std::vector<otg_unitset_unit> units;
  std::vector<uint8_t> unit_arena;
  return vcf_allele_job("otg_units_files", job->vcf_path, job->bed_path, job->device, job->batch_alleles ? job->batch_alleles : 65536, job->threads, write, user, stats,
    [&](otg_ctx* ctx, const VcfBatch& B) {
      rec_bed.resize(B.nr); group_first.resize((size_t)B.nr + 1); sets.resize(B.nr); set_first.assign((size_t)B.nr + 1, 0);
      std::string name;
      for (uint32_t r = 0; r < B.nr; ++r) {
        name.assign(B.regions.data() + B.rec[r].region_off, B.rec[r].region_len);
        const auto it = by_region.find(name);
        if (it == by_region.end()) return otg_fail(ctx, OTG_ERR_ARG, "no BED record for the region %s", name.c_str());
        rec_bed[r] = it->second;
        group_first[r] = B.rec[r].first_allele;
      }
      group_first[B.nr] = B.na;
      if (B.na == 0) return (int)OTG_OK;                            // (records always have a REF allele)
      if (int rc = otg_repeat_batch(ctx, B.seqs.data(), B.au, B.off.data(), B.len.data(), B.na, max_period, min_copies, min_span, nullptr, nullptr, nullptr)) return rc;
      uint64_t nu = 0, nb = 0;
      if (int rc = otg_unitset_repeats(ctx, group_first.data(), B.nr, &q, sets.data(), set_first.data(), &nu, &nb)) return rc;
      units.resize(nu + 1); unit_off.resize(nu + 1); unit_len.resize(nu + 1); unit_arena.resize(nb + 1);
      return otg_unitset_collect(ctx, units.data(), unit_off.data(), unit_len.data(), nu, unit_arena.data(), nb);
    },
    [&](std::string& o, const VcfBatch& B, uint32_t r0, uint32_t nr) {
      otg_unitset_lines(o, B.rec.data() + r0, nr, rec_bed.data() + r0, bed.beds.data(), bed.chr_arena.data(), set_first.data() + r0, units.data(), unit_arena.data(),
                        unit_off.data(), unit_len.data());
    });
}

// The locus mode over a VCF's alleles with the unit sets discovered where the catalogue has none, in one pass per batch: the repeat
// structure, the discovery (one group per VCF record), then the locus mode on the batch's alleles where the repeat call left them in HBM.
// A region whose catalogue record has units keeps them; any other region gets the set discovered from its alleles; rows as otg_loci_files.
int otg_units_loci_files(const otg_loci_job* job, const otg_units_job* discover, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !discover || !write || !job->vcf_path || !job->bed_path)
    return otg_fail(nullptr, OTG_ERR_ARG, "otg_units_loci_files: NULL job, discovery parameters, writer, VCF or BED path");
  const otg_tract_params q{job->match, job->mismatch, job->indel, job->min_score};
  if (int rc = tract_cli_args(q)) return rc;
  if (int rc = units_cli_args(*discover)) return rc;
  const otg_unitset_params dq{discover->min_bases, discover->min_share, discover->redundant, 0u};
  const uint32_t max_period = discover->max_period, min_copies = discover->min_copies, min_span = discover->min_span;
  const char* who = "otg_units_loci_files";
  UnitCatalogue cat;
  if (int rc = cat.load(who, job->bed_path)) return rc;
  BatchSets S;
  std::vector<uint64_t> seg_off, t_seg_off, d_set_first, d_uoff;
  std::vector<uint32_t> group_first, d_ulen;
  std::vector<uint8_t> d_arena;
  std::vector<otg_unitset_unit> d_units;
  std::vector<otg_locus> sums, t_sums;
  std::vector<otg_unitparse_seg> segs;
  return vcf_allele_job(who, job->vcf_path, job->bed_path, job->device, job->batch_alleles ? job->batch_alleles : 65536, job->threads, write, user, stats,
    [&](otg_ctx* ctx, const VcfBatch& B) {
      S.begin(B.na);
      t_sums.clear(); t_seg_off.assign(1, 0); segs.resize(1);
      if (B.na == 0) {
        S.finish();
        S.spread(0, t_sums, t_seg_off, 0, sums, seg_off);
        return (int)OTG_OK;
      }
      group_first.resize((size_t)B.nr + 1);
      for (uint32_t r = 0; r < B.nr; ++r) group_first[r] = B.rec[r].first_allele;
      group_first[B.nr] = B.na;
      d_set_first.assign((size_t)B.nr + 1, 0);
      if (int rc = otg_repeat_batch(ctx, B.seqs.data(), B.au, B.off.data(), B.len.data(), B.na, max_period, min_copies, min_span, nullptr, nullptr, nullptr)) return rc;
      uint64_t nu = 0, nb = 0;
      if (int rc = otg_unitset_repeats(ctx, group_first.data(), B.nr, &dq, nullptr, d_set_first.data(), &nu, &nb)) return rc;
      d_units.resize(nu + 1); d_uoff.resize(nu + 1); d_ulen.resize(nu + 1); d_arena.resize(nb + 1);
      if (int rc = otg_unitset_collect(ctx, d_units.data(), d_uoff.data(), d_ulen.data(), nu, d_arena.data(), nb)) return rc;
      std::string name;
      for (uint32_t r = 0; r < B.nr; ++r) {
        const otg_vcf_record& R = B.rec[r];
        name.assign(B.regions.data() + R.region_off, R.region_len);
        uint64_t u0, u1;
        cat.units_of(name, &u0, &u1);
        const int rc = u1 > u0 ? S.add(ctx, name, R, cat.arena.data(), cat.off.data(), cat.len.data(), u0, u1)
                               : S.add(ctx, name, R, d_arena.data(), d_uoff.data(), d_ulen.data(), d_set_first[r], d_set_first[r + 1]);      // the discovered set
        if (rc) return rc;
      }
      S.finish();
      const uint32_t nt = (uint32_t)S.tseq.size();
      t_sums.resize(nt); t_seg_off.assign((size_t)nt + 1, 0);
      uint64_t total = 0;
      if (nt) {
        // the alleles lie where the repeat call read them: no second upload.  The sets have passed BatchSets::add, which stands in for
        // otg_unitparse_check here
        if (int rc = otg_locus_resident(ctx, who, ctx->last_repeat_rows, B.len.data(), B.na, S.units.data(), S.units.size() - 1, S.uoff.data(), S.ulen.data(), S.n_units(),
                                        S.set_first.data(), S.n_sets(), S.tseq.data(), S.tset.data(), nt, q, t_sums.data(), t_seg_off.data(), &total)) return rc;
      }
      segs.resize(total + 1);
      if (total)
        if (int rc = otg_locus_collect(ctx, segs.data(), total)) return rc;
      S.spread(B.na, t_sums, t_seg_off, total, sums, seg_off);
      return (int)OTG_OK;
    },
    [&](std::string& o, const VcfBatch& B, uint32_t r0, uint32_t nr) {
      otg_locus_rows(o, B.rec.data() + r0, nr, B.regions.data(), B.len.data(), S.allele_set.data(), S.set_first.data(), S.units.data(), S.uoff.data(), S.ulen.data(),
                     sums.data(), seg_off.data(), segs.data());
    });
}

// ---- `otter genotype` from files to text in one call: genotype() / genotype_process() (src/genotype.cpp:69-192).  Regions in bounded
// batches: allele ingest (host threads) -> anallele_cluster on the device -> VCF lines (or, without a reference, the two-length table),
// text in BED order.  The reference's worker loop does the same region by region on a thread pool and prints under a mutex.
int otg_genotype_files(const otg_genotype_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->bam_path || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_genotype_files: NULL job, writer, BAM or BED path");
  const bool with_ref = job->fasta_path && job->fasta_path[0];
  if (with_ref && job->metric != OTG_GT_METRIC_LENGTH && job->metric != OTG_GT_METRIC_EDIT)      // (the length table involves no clustering: no metric to refuse)
    return otg_fail(nullptr, OTG_ERR_ARG, "otg_genotype_files: unknown genotype metric %u (OTG_GT_METRIC_LENGTH = 0, OTG_GT_METRIC_EDIT = 1)", job->metric);
  const auto t_all = Clock::now();
  otg_job_stats st{};
  Bed bed;
  int rc = load_bed(job->bed_path, bed);
  if (rc != OTG_OK) return rc;
  const std::vector<otg_bed>& beds = bed.beds; const std::vector<char>& chr_arena = bed.chr_arena;
  st.n_regions = (uint32_t)beds.size();
  BamPtr bam; FastaPtr fasta;
  PooledCtx ctx(nullptr, PoolReturn{job->device});
  rc = open_bam(job->bam_path, bam);
  if (rc != OTG_OK) return rc;
  uint32_t n_samples = 0; int32_t ol = 0, orr = 0;
  rc = otg_bam_sample_index(bam.get(), &n_samples, &ol, &orr);                // SampleIndex::init (src/anbamdb.cpp:42-63)
  if (rc != OTG_OK) return rc;
  if (with_ref) {
    rc = open_fasta(job->fasta_path, fasta);
    if (rc != OTG_OK) return rc;
    if (!(ctx = acquire_ctx(job->device))) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_genotype_files: %s", last_err().c_str());
    std::string hdr;
    rc = sized_text(hdr, [&](char* buf, uint64_t cap, uint64_t* need) { return otg_emit_vcf_header(bam.get(), buf, cap, need); });   // output_vcf_header (src/genotype.cpp:16-40)
    if (rc != OTG_OK) return rc;
    if (write(user, hdr.data(), hdr.size()) != 0) return otg_fail(nullptr, OTG_ERR_ARG, "otg_genotype_files: the writer failed");
    st.output_bytes += hdr.size();
  }
  const uint32_t per = job->batch_regions ? job->batch_regions : 1024u;
  const int threads = job->threads > 0 ? job->threads : 1;
  // Two batches in flight: while one is clustered on the GPU and formatted, the next is ingested (the reference does all three one region at a
  // time, src/genotype.cpp:80-157; SURVEY finding 9: this command is BAM-I/O-bound, so ingest is what must never wait).  The VCF text of a batch is
  // formatted by `threads` host threads, each a contiguous slice of its regions, concatenated in order.
  struct GtBatch {
    std::vector<uint8_t> arena; std::vector<otg_allele> alleles; std::vector<uint32_t> first;
    uint32_t f = 0, n = 0, na = 0; uint64_t used = 0; int rc = OTG_OK; double ms = 0; std::string err;
  };
  auto ingest_into = [&](GtBatch& B, uint32_t f) {
    B.f = f; B.n = std::min<uint32_t>(per, (uint32_t)beds.size() - f);
    B.first.assign((size_t)B.n + 1, 0);
    size_t cap_al = std::max<size_t>(B.alleles.size(), (size_t)B.n * 128 + 64), cap_ar = std::max<size_t>(B.arena.size(), (size_t)B.n * 128 * 4096 + 4096);
    const auto t0 = Clock::now();
    for (int attempt = 0; attempt < 4; ++attempt) {
      B.alleles.resize(cap_al); B.arena.resize(cap_ar);
      B.na = 0; B.used = 0;
      B.rc = otg_ingest_alleles(bam.get(), beds.data() + f, chr_arena.data(), B.n, threads, fasta.get(), B.arena.data(), B.arena.size(), &B.used, B.alleles.data(), (uint32_t)B.alleles.size(), &B.na, B.first.data());
      if (B.rc != OTG_ERR_CAPACITY) break;
      cap_al = (size_t)B.na + 64; cap_ar = (size_t)B.used + 4096;
    }
    if (B.rc != OTG_OK) B.err = last_err();
    B.ms = ms_since(t0);
  };
  std::vector<uint64_t> seq_off; std::vector<uint32_t> seq_len, n_al;
  std::vector<int32_t> gt, gtl, gtk, ngt, reps; std::vector<double> hsd;
  std::string text;
  std::vector<std::string> parts;
  const uint32_t n_beds = (uint32_t)beds.size();
  TwoInFlight<GtBatch> flight;
  if (n_beds) ingest_into(flight.current(), 0);
  for (uint32_t f = 0; f < n_beds; f += per, flight.advance()) {
    GtBatch& B = flight.current();
    if (B.rc != OTG_OK) return otg_fail(nullptr, B.rc, "otg_genotype_files: %s", B.err.c_str());
    const bool more = f + per < n_beds;
    if (more && with_ref) flight.prefetch([&, f](GtBatch& N) { ingest_into(N, f + per); });
    const uint32_t n = B.n, na = B.na; const uint64_t used = B.used;
    std::vector<uint32_t>& first = B.first; std::vector<otg_allele>& alleles = B.alleles; std::vector<uint8_t>& arena = B.arena;
    st.ms_ingest += B.ms; st.n_reads += na; st.input_bytes += used;
    auto t0 = Clock::now();
    if (with_ref) {
      seq_off.resize(na); seq_len.resize(na); n_al.resize(n);
      for (uint32_t i = 0; i < na; ++i) { seq_off[i] = alleles[i].seq_off; seq_len[i] = alleles[i].seq_len; }
      for (uint32_t r = 0; r < n; ++r) n_al[r] = first[r + 1] - first[r];
      gt.resize((size_t)na + 1); gtl.resize((size_t)na + 1); gtk.resize((size_t)na + 1); reps.resize((size_t)na + 1); hsd.resize((size_t)na + 1); ngt.resize((size_t)n + 1);
      if (arena.size() < used + 64) arena.resize(used + 64);
      if (na) {
        rc = otg_genotype_cluster_metric_batch(ctx.get(), &job->params, arena.data(), used + 64, seq_off.data(), seq_len.data(), first.data(), n_al.data(), n,
                                               gt.data(), gtl.data(), gtk.data(), hsd.data(), ngt.data(), reps.data(),      // anallele_cluster (src/genotype.cpp:138)
                                               (int32_t)job->metric, nullptr, nullptr);
        if (rc != OTG_OK) return otg_fail(nullptr, rc, "otg_genotype_files: %s", ctx_err(ctx.get()).c_str());
      } else std::fill(ngt.begin(), ngt.end(), 0);
      st.ms_hot_path += ms_since(t0);
      t0 = Clock::now();
      std::string err;
      rc = emit_vcf_sliced(bed, f, n, first.data(), alleles.data(), arena.data(), n_samples, gt.data(), hsd.data(), ngt.data(), reps.data(), ol, orr, threads, parts, text, &err);
      if (rc != OTG_OK) return otg_fail(nullptr, rc, "otg_genotype_files: %s", err.c_str());
    } else {
      rc = sized_text(text, [&](char* buf, uint64_t cap, uint64_t* need) {                                                     // src/genotype.cpp:112-121
        return otg_emit_genotype_lengths(bam.get(), beds.data() + f, chr_arena.data(), n, first.data(), alleles.data(), n_samples, buf, cap, need);
      });
      if (rc != OTG_OK) return rc;
    }
    st.ms_emit += ms_since(t0);
    for (uint32_t r = 0; r < n; ++r) { if (first[r + 1] > first[r]) ++st.n_regions_ok; }
    st.n_alleles += na;
    if (!text.empty() && write(user, text.data(), text.size()) != 0) return otg_fail(nullptr, OTG_ERR_ARG, "otg_genotype_files: the writer failed");
    st.output_bytes += text.size();
    // (the two-length table without -r reads the BAM handle's sample list while it formats: there the next batch is ingested in sequence)
    if (more && !with_ref) ingest_into(flight.other(), f + per);
  }
  st.ms_total = ms_since(t_all); st.n_devices = 1;
  if (stats) *stats = st;
  return OTG_OK;
}

// ---- sample BAMs to one joint VCF: `otter assemble` per sample and `otter genotype` on their alleles, which stay on the device in between
// (cohort.hip).  Shards, batch plan and the BED-order writer as otg_assemble_files.
int otg_cohort_files(const otg_cohort_job* job, otg_write_fn write, void* user, otg_job_stats* stats)
{
  if (!job || !write || !job->bed_path) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: NULL job, writer or BED path");
  if (job->n_samples == 0 || !job->bam_paths || !job->sample_names) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: zero samples (n_samples = %u)", job->n_samples);
  if (!job->fasta_path || !job->fasta_path[0]) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: no reference FASTA (fasta_path): the joint VCF needs the reference alleles");
  if (job->n_devices < 0 || (job->n_devices > 0 && !job->devices)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: bad device list");
  if (job->gt_metric != OTG_GT_METRIC_LENGTH && job->gt_metric != OTG_GT_METRIC_EDIT)
    return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: unknown genotype metric %d (OTG_GT_METRIC_LENGTH = 0, OTG_GT_METRIC_EDIT = 1)", job->gt_metric);
  if (job->matrix_write && (job->matrix_k < 1 || job->matrix_k > OTG_KMER_MAX))
    return otg_fail(nullptr, OTG_ERR_ARG, "[ERROR] invalid '--kmer-size' (%d). Needs to be 1 <= x <= %d.", job->matrix_k, OTG_KMER_MAX);
  const uint32_t S = job->n_samples;
  {
    std::map<std::string, uint32_t> seen;
    for (uint32_t s = 0; s < S; ++s) {
      if (!job->bam_paths[s] || !job->bam_paths[s][0]) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: sample %u has no BAM path", s);
      if (!job->sample_names[s] || !job->sample_names[s][0]) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: sample %u (%s) has an empty name", s, job->bam_paths[s]);
      auto ins = seen.emplace(job->sample_names[s], s);
      if (!ins.second) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: sample name '%s' is given twice (samples %u and %u)", job->sample_names[s], ins.first->second, s);
    }
  }
  const auto t_all = Clock::now();
  g_trace_t0 = t_all;
  CohortShared C;
  C.j = job; C.n_samples = S;
  C.P = job->params; C.P.realign = 1;
  Job& M = C.M;
  int rc = load_bed(job->bed_path, C.bed);
  if (rc != OTG_OK) return rc;
  const uint32_t R = (uint32_t)C.bed.beds.size();
  M.st.n_regions = R;
  {
    // regions are identified by index here, by their chr:start-end string in the file round trip: the same string twice would differ
    std::map<std::string, uint32_t> seen;
    for (uint32_t r = 0; r < R; ++r) {
      const otg_bed& b = C.bed.beds[r];
      std::string key(C.bed.chr_arena.data() + b.chr_off, b.chr_len);
      key += ":" + std::to_string((uint32_t)b.start) + "-" + std::to_string((uint32_t)b.end);
      auto ins = seen.emplace(key, r);
      if (!ins.second) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: BED records %u and %u of %s are the same region %s", ins.first->second + 1, r + 1, job->bed_path, key.c_str());
    }
  }
  rc = open_fasta(job->fasta_path, C.fasta);
  if (rc != OTG_OK) return rc;
  C.bams.resize(S);
  for (uint32_t s = 0; s < S; ++s) {
    rc = open_bam(job->bam_paths[s], C.bams[s]);
    if (rc != OTG_OK) return rc;
    if (s > 0) {
      otg_bam* b0 = C.bams[0].get(); otg_bam* bs = C.bams[s].get();
      bool same = otg_bam_n_targets(bs) == otg_bam_n_targets(b0);
      for (uint32_t i = 0; same && i < otg_bam_n_targets(b0); ++i) {
        uint64_t l0 = 0, l1 = 0;
        const char* n0 = otg_bam_target(b0, i, &l0); const char* n1 = otg_bam_target(bs, i, &l1);
        same = l0 == l1 && strcmp(n0, n1) == 0;
      }
      if (!same) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: the targets of %s differ from those of the first BAM %s", job->bam_paths[s], job->bam_paths[0]);
    }
  }
  // headers: the VCF header with the first BAM's contigs and the samples' names; per sample the SAM header of its allele records
  {
    otg_bam* b0 = C.bams[0].get();
    otg_bam_set_samples(b0, job->sample_names, S, job->ingest.offset_l, job->ingest.offset_r);
    std::string hdr;
    rc = sized_text(hdr, [&](char* buf, uint64_t cap, uint64_t* need) { return otg_emit_vcf_header(b0, buf, cap, need); });
    if (rc != OTG_OK) return rc;
    if (write(user, hdr.data(), hdr.size()) != 0) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: the writer failed");
    M.st.output_bytes += hdr.size();
    for (uint32_t s = 0; job->allele_write && s < S; ++s) {
      rc = sam_header_text(b0, job->sample_names[s], job->ingest.offset_l, job->ingest.offset_r, hdr);
      if (rc != OTG_OK) return rc;
      if (job->allele_write(job->allele_user, s, hdr.data(), hdr.size()) != 0) return otg_fail(nullptr, OTG_ERR_ARG, "otg_cohort_files: the allele writer failed");
    }
  }
  M.st.n_devices = run_shards<CohortText>(
      M, job->devices, job->n_devices, R, job->batch_regions, job->ingest.threads,
      [&](int device, uint32_t a, uint32_t b, int threads, OrderedOutput<CohortText>& out) { cohort_shard_worker(C, device, a, b, threads, out); },
      [&](uint32_t, const CohortText& text) {
        if (!text.vcf.empty() && write(user, text.vcf.data(), text.vcf.size()) != 0) { M.fail(OTG_ERR_ARG, "the writer failed"); return false; }
        M.st.output_bytes += text.vcf.size();
        if (!text.mat.empty() && job->matrix_write(job->matrix_user, text.mat.data(), text.mat.size()) != 0) { M.fail(OTG_ERR_ARG, "the matrix writer failed"); return false; }
        for (uint32_t s = 0; s < (uint32_t)text.sam.size(); ++s)
          if (!text.sam[s].empty() && job->allele_write(job->allele_user, s, text.sam[s].data(), text.sam[s].size()) != 0) { M.fail(OTG_ERR_ARG, "the allele writer failed"); return false; }
        return true;
      });
  trace("job", 0, R, t_all);
  M.st.ms_total = ms_since(t_all);
  if (stats) *stats = M.st;
  if (M.rc.load() != OTG_OK) return otg_fail(nullptr, M.rc.load(), "otg_cohort_files: %s", M.err.c_str());
  return OTG_OK;
}

int otg_assemble_batch_plan(uint32_t n_regions, uint32_t batch_regions, uint32_t* sizes, uint32_t capacity, uint32_t* n_batches)
{
  if (!n_batches || (capacity && !sizes)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_assemble_batch_plan: NULL argument");
  const std::vector<std::pair<uint32_t, uint32_t>> plan = batch_plan(0, n_regions, batch_regions);
  *n_batches = (uint32_t)plan.size();
  if (plan.size() > capacity) return OTG_ERR_CAPACITY;
  for (size_t i = 0; i < plan.size(); ++i) sizes[i] = plan[i].second;
  return OTG_OK;
}

void otg_assemble_files_release(void)
{
  std::lock_guard<std::mutex> lk(g_pool_m);
  for (auto& p : g_pool) otg_destroy(p.second);
  g_pool.clear();
  g_batches.clear();
}

} // extern "C"

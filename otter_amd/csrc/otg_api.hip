// otg_api.hip — context, device scratch and the L1/L2 C-ABI entry points (host side).
#include "otg_common.hpp"
#include <cmath>
#include <cstdarg>
#include <algorithm>

thread_local std::string g_otg_err;

int otg_fail(otg_ctx* ctx, int code, const char* fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_otg_err = buf;
  if (ctx) ctx->err = buf;
  return code;
}

// bam_sink.cpp is built without the rest of the library in stand-alone programs; inside the library its refusals reach otg_last_error(NULL) here
extern "C" void otg_set_global_error(const char* msg) { g_otg_err = msg ? msg : ""; }

std::mutex& otg_device_mutex(int device)
{
  static std::mutex m[64];
  return m[(unsigned)device % 64u];
}

void* otg_slot(otg_ctx* ctx, int slot, size_t bytes)
{
  if (bytes == 0) bytes = 16;
  DevBuf& b = ctx->pool[slot];
  if (b.cap >= bytes) return b.p;
  if (b.p) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
  // 25 % headroom (at most 1 GB): a slightly larger batch must not cost a hipFree + hipMalloc; the multi-gigabyte kernel workspaces are
  // sized independently of the batch by their callers and need none
  size_t want = bytes + std::min<size_t>(bytes >> 2, (size_t)1 << 30) + 256;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess && want > bytes) { (void)hipGetLastError(); want = bytes; e = hipMalloc(&b.p, want); }
  if (e != hipSuccess) {
    otg_fail(ctx, OTG_ERR_HIP, "hipMalloc(%zu bytes, slot %d) failed: %s", want, slot, hipGetErrorString(e));
    b.p = nullptr;
    return nullptr;
  }
  b.cap = want;
  return b.p;
}

int otg_rows_check(otg_ctx* ctx, const char* who, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* off, const uint32_t* len, uint32_t n,
                   uint32_t* max_len)
{
  if (n && (!off || !len || (arena_bytes && !arena))) return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL argument", who);
  uint32_t longest = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (off[i] > arena_bytes || len[i] > arena_bytes - off[i])
      return otg_fail(ctx, OTG_ERR_ARG, "%s: allele %u (offset %llu, length %u) lies outside the %llu-byte arena", who, i, (unsigned long long)off[i], len[i],
                      (unsigned long long)arena_bytes);
    longest = std::max(longest, len[i]);
  }
  if (max_len) *max_len = longest;
  return OTG_OK;
}

int otg_rows_upload(otg_ctx* ctx, int slot_seq, int slot_meta, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* off, const uint32_t* len,
                    uint32_t n, OtgRows* out)
{
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint8_t* d_arena = (uint8_t*)otg_slot(ctx, slot_seq, arena_bytes + 64);
  uint8_t* d_meta = (uint8_t*)otg_slot(ctx, slot_meta, (size_t)n * 12);
  if (!d_arena || !d_meta) return OTG_ERR_HIP;
  uint64_t* d_off = (uint64_t*)d_meta;
  uint32_t* d_len = (uint32_t*)(d_meta + (size_t)n * 8);
  HIP_TRY(ctx, hipMemsetAsync(d_arena + arena_bytes, 0, 64, ctx->stream));
  if (arena_bytes) HIP_TRY(ctx, hipMemcpyAsync(d_arena, arena, arena_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_off, off, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_len, len, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  *out = OtgRows{d_arena, d_off, d_len};
  return OTG_OK;
}

int otg_seg_collect(otg_ctx* ctx, const char* who, const char* noun, OtgSegLast otg_ctx::*which, int slot_segs, size_t seg_bytes, void* segs, uint64_t capacity)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL context", who);
  if (!(ctx->*which).valid) return otg_fail(ctx, OTG_ERR_ARG, "%s: no %s results on this context", who, noun);
  const uint64_t total = (ctx->*which).total;
  if (capacity < total)
    return otg_fail(ctx, OTG_ERR_CAPACITY, "%s: capacity %llu, the latest call has %llu segments", who, (unsigned long long)capacity, (unsigned long long)total);
  if (total == 0) return OTG_OK;
  if (!segs) return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL segs", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(segs, ctx->pool[slot_segs].p, (size_t)total * seg_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OTG_OK;
}

int otg_seg_device_results(otg_ctx* ctx, const char* who, const char* noun, OtgSegLast otg_ctx::*which, int slot_res, int slot_segs, size_t sum_bytes, uint32_t* n,
                           const void** sums, const uint64_t** seg_off, const void** segs, uint64_t* total)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL context", who);
  const OtgSegLast& last = ctx->*which;
  if (!last.valid) return otg_fail(ctx, OTG_ERR_ARG, "%s: no %s results on this context", who, noun);
  const uint8_t* res = (const uint8_t*)ctx->pool[slot_res].p;
  if (n) *n = last.n;
  if (sums) *sums = res;
  if (seg_off) *seg_off = (const uint64_t*)(res + (size_t)last.n * sum_bytes);
  if (segs) *segs = ctx->pool[slot_segs].p;
  if (total) *total = last.total;
  return OTG_OK;
}

int otg_text_out(const char* who, const std::string& text, char* out, uint64_t capacity, uint64_t* out_len)
{
  *out_len = text.size();
  if (text.size() > capacity || (!out && !text.empty())) return otg_fail(nullptr, OTG_ERR_CAPACITY, "%s: output buffer too small", who);
  if (!text.empty()) memcpy(out, text.data(), text.size());
  return OTG_OK;
}

// ---- glibc exp() restated on the host, used ONLY to detect which build of exp() the host libm runs
// (the device KDE mirrors that build bit for bit; see cluster.hip / DESIGN.md §5). -------------------
#include "exp_table.inc"
static double host_exp_variant(double x, bool use_fma);
static int exp_probe(uint64_t* n_args, uint64_t* n_differ, uint64_t* mism_fma, uint64_t* mism_nofma);

extern "C" {

void otg_params_default(otg_params* p)
{
  memset(p, 0, sizeof(*p));
  p->max_alleles = 2; p->ignore_haps = 1; p->max_cov = 200; p->flank = 100; p->bandwidth_length = 500;
  p->min_cov_fraction2_l = 500; p->mismatch = 4; p->gap_open = 6; p->gap_ext = 2; p->realign = 0;
  p->bandwidth_short = 0.01; p->bandwidth_long = 0.015; p->max_error = 0.01; p->min_cov_fraction = 0.2;
  p->min_cov_fraction2_f = 0.1; p->min_sim = 0.9; p->gt_max_error = 0.025; p->gt_max_cosdis = 0.025;
  p->heuristic = OTG_HEURISTIC_NONE; p->heur_min_wavefront_length = 10; p->heur_max_distance_threshold = 50; p->heur_steps_between_cutoffs = 1;
}

int otg_set_heuristic(otg_ctx* ctx, int strategy, int min_wavefront_length, int max_distance_threshold, int steps_between_cutoffs)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_set_heuristic: no context");
  if (strategy != OTG_HEURISTIC_NONE && strategy != OTG_HEURISTIC_WFADAPTIVE) return otg_fail(ctx, OTG_ERR_ARG, "otg_set_heuristic: unknown strategy %d", strategy);
  if (strategy == OTG_HEURISTIC_WFADAPTIVE && (min_wavefront_length < 0 || max_distance_threshold < 0))
    return otg_fail(ctx, OTG_ERR_ARG, "otg_set_heuristic: negative wavefront length or distance threshold");
  ctx->heur_strategy = strategy;
  if (strategy == OTG_HEURISTIC_WFADAPTIVE) {
    ctx->heur_min_wf_len = min_wavefront_length; ctx->heur_max_dist = max_distance_threshold;
    ctx->heur_steps = steps_between_cutoffs < 1 ? 1 : steps_between_cutoffs;
  }
  return OTG_OK;
}

int otg_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* otg_last_error(otg_ctx* ctx) { return ctx ? ctx->err.c_str() : g_otg_err.c_str(); }

int otg_create(int device, otg_ctx** out)
{
  if (!out) return otg_fail(nullptr, OTG_ERR_ARG, "otg_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "no HIP device available (%s); libotter_gpu has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device < 0 || device >= n) return otg_fail(nullptr, OTG_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
  otg_ctx* ctx = new otg_ctx();
  ctx->device = device;
  ctx->pool.resize(SLOT_COUNT);
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&ctx->prop, device) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
    delete ctx;
    return otg_fail(nullptr, OTG_ERR_HIP, "HIP device %d could not be initialised", device);
  }
  ctx->n_cu = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
  // probe the host libm: does exp() round like glibc's FMA build or its non-FMA build?  (exp_probe below)
  {
    uint64_t n_args = 0, n_differ = 0, mism[2] = {0, 0};
    ctx->exp_variant = exp_probe(&n_args, &n_differ, &mism[1], &mism[0]);
    ctx->exp_probe_mismatches = (long long)mism[ctx->exp_variant];
  }
  *out = ctx;
  return OTG_OK;
}

void otg_destroy(otg_ctx* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  otg_pipeline_free(ctx);
  otg_cohort_free(ctx);
  for (auto& b : ctx->pool) if (b.p) (void)hipFree(b.p);
  for (int i = 0; i < 5; ++i) { if (ctx->tier_stream[i]) (void)hipStreamDestroy(ctx->tier_stream[i]); if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]); }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->edit_hist) (void)hipHostFree(ctx->edit_hist);
  for (int i = 0; i < 2; ++i) if (ctx->edit_hist_ev[i]) (void)hipEventDestroy(ctx->edit_hist_ev[i]);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int otg_trim(otg_ctx* ctx)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_trim: no context");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // the aligners' per-launch workspaces (provenance slabs, row tables, op lists): nothing in them outlives a call
  for (int slot : {SLOT_WF_WS, SLOT_REVOPS, SLOT_BT_POOL}) {
    DevBuf& b = ctx->pool[slot];
    if (b.p) { HIP_TRY(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
  }
  ctx->last_chain = -1;      // the score bounds went with SLOT_BT_POOL: otg_affine_last_routing has nothing to read until the next launch
  return OTG_OK;
}

int otg_exp_variant(otg_ctx* ctx) { return ctx ? ctx->exp_variant : -1; }
long long otg_exp_probe_mismatches(otg_ctx* ctx) { return ctx ? ctx->exp_probe_mismatches : -1; }

int otg_exp_probe(uint64_t* n_args, uint64_t* n_differ, uint64_t* mismatches_fma, uint64_t* mismatches_nofma)
{
  return exp_probe(n_args, n_differ, mismatches_fma, mismatches_nofma);
}

int otg_exp_host(const double* x, uint64_t n, int variant, double* out)
{
  if ((n && (!x || !out)) || (variant != 0 && variant != 1)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_exp_host: NULL argument or variant not 0 / 1");
  for (uint64_t i = 0; i < n; ++i) out[i] = host_exp_variant(x[i], variant != 0);
  return OTG_OK;
}

int otg_exp_device(otg_ctx* ctx, const double* x, uint64_t n, int variant, double* out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_exp_device: no context (no HIP device?)");
  if ((n && (!x || !out)) || (variant != 0 && variant != 1)) return otg_fail(ctx, OTG_ERR_ARG, "otg_exp_device: NULL argument or variant not 0 / 1");
  if (n == 0) return OTG_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  double* d = (double*)otg_slot(ctx, SLOT_AUX0, n * sizeof(double));
  if (!d) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemcpyAsync(d, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = otg_launch_exp(ctx, d, n, variant)) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(out, d, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OTG_OK;
}

static uint32_t max_len_of(const otg_align_task* tasks, uint32_t n)
{
  uint32_t m = 1;
  for (uint32_t i = 0; i < n; ++i) {
    if (tasks[i].pattern_len > m) m = tasks[i].pattern_len;
    if (tasks[i].text_len > m) m = tasks[i].text_len;
  }
  return m;
}

static int check_tasks(otg_ctx* ctx, const otg_align_task* tasks, uint32_t n, uint64_t arena_bytes)
{
  for (uint32_t i = 0; i < n; ++i) {
    const otg_align_task& t = tasks[i];
    if (t.pattern_off + t.pattern_len > arena_bytes || t.text_off + t.text_len > arena_bytes)
      return otg_fail(ctx, OTG_ERR_ARG, "task %u: sequence range outside the arena", i);
    if (t.endsfree && (t.pattern_begin_free < 0 || t.pattern_end_free < 0 || t.text_begin_free < 0 || t.text_end_free < 0))
      return otg_fail(ctx, OTG_ERR_ARG, "task %u: negative free-end length", i);
  }
  return OTG_OK;
}

int otg_edit_distance_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes,
                            const otg_align_task* tasks, uint32_t n_tasks, int32_t* scores_out, uint64_t* cells_out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_edit_distance_batch: no context (no HIP device?)");
  if (n_tasks == 0) return OTG_OK;
  if (!seq_arena || !tasks || !scores_out) return otg_fail(ctx, OTG_ERR_ARG, "otg_edit_distance_batch: NULL argument");
  int rc = check_tasks(ctx, tasks, n_tasks, arena_bytes);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint8_t* d_arena = (uint8_t*)otg_slot(ctx, SLOT_ARENA, arena_bytes + 64);
  otg_align_task* d_tasks = (otg_align_task*)otg_slot(ctx, SLOT_TASKS, (size_t)n_tasks * sizeof(otg_align_task));
  int32_t* d_scores = (int32_t*)otg_slot(ctx, SLOT_SCORES, (size_t)n_tasks * sizeof(int32_t));
  uint64_t* d_cells = (uint64_t*)otg_slot(ctx, SLOT_CELLS, (size_t)n_tasks * sizeof(uint64_t));
  if (!d_arena || !d_tasks || !d_scores || !d_cells) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemsetAsync(d_arena + arena_bytes, 0, 64, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_arena, seq_arena, arena_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_tasks, tasks, (size_t)n_tasks * sizeof(otg_align_task), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_scores, 0xff, (size_t)n_tasks * sizeof(int32_t), ctx->stream));
  ctx->max_seq_len = max_len_of(tasks, n_tasks);
  rc = otg_launch_edit(ctx, d_arena, d_tasks, n_tasks, d_scores, d_cells, nullptr, nullptr);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(scores_out, d_scores, (size_t)n_tasks * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (cells_out) HIP_TRY(ctx, hipMemcpyAsync(cells_out, d_cells, (size_t)n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t i = 0; i < n_tasks; ++i)
    if (scores_out[i] < 0) return otg_fail(ctx, OTG_ERR_FATAL, "edit task %u did not terminate", i);
  return OTG_OK;
}

// Staging shared by the three edit alignment entry points (the caller has validated its arguments and set ctx's heuristic): arena and tasks to
// the device, device op-string slots, the launch (exact: otg_launch_edit_align, adaptive: otg_launch_edit_align_adaptive), the times and tier
// counts of the call, the cell counts, then the length-only / capacity protocol and the packed op strings.
static int edit_align_staged(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const otg_align_task* tasks, uint32_t n_tasks, bool adaptive,
                             int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                             uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used, uint64_t* cells_out)
{
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // device op-string slots: task i has at most pattern_len + text_len columns
  std::vector<uint64_t> slot(n_tasks + 1);
  slot[0] = 0;
  for (uint32_t i = 0; i < n_tasks; ++i) slot[i + 1] = slot[i] + (cigar_arena ? (((uint64_t)tasks[i].pattern_len + tasks[i].text_len + 15) & ~15ull) : 0);
  uint8_t* d_arena = (uint8_t*)otg_slot(ctx, SLOT_ARENA, arena_bytes + 64);
  otg_align_task* d_tasks = (otg_align_task*)otg_slot(ctx, SLOT_TASKS, (size_t)n_tasks * sizeof(otg_align_task));
  uint8_t* d_cig = cigar_arena ? (uint8_t*)otg_slot(ctx, SLOT_CIG_ARENA, slot[n_tasks] + 64) : nullptr;
  if (!d_arena || !d_tasks || (cigar_arena && !d_cig)) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemsetAsync(d_arena + arena_bytes, 0, 64, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_arena, seq_arena, arena_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_tasks, tasks, (size_t)n_tasks * sizeof(otg_align_task), hipMemcpyHostToDevice, ctx->stream));
  ctx->max_seq_len = max_len_of(tasks, n_tasks);
  double sms = 0, pms = 0;
  uint32_t fin[2] = {0u, 0u};
  int rc;
  if (adaptive) {
    std::vector<uint64_t> cells(n_tasks);
    rc = otg_launch_edit_align_adaptive(ctx, d_arena, d_tasks, tasks, n_tasks, scores_out, cells.data(), cigar_len_out, d_cig, slot.data(), &sms, &pms, fin);
    if (rc) return rc;
    if (cells_out) memcpy(cells_out, cells.data(), (size_t)n_tasks * sizeof(uint64_t));
  } else {
    rc = otg_launch_edit_align(ctx, d_arena, d_tasks, tasks, n_tasks, scores_out, cigar_len_out, d_cig, slot.data(), &sms, &pms, fin);
    if (rc) return rc;
    if (cells_out) {        // the exact score chain left its cell counts in SLOT_CELLS
      if (hipMemcpy(cells_out, ctx->pool[SLOT_CELLS].p, (size_t)n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return otg_fail(ctx, OTG_ERR_HIP, "copying the cell counts failed");
    }
  }
  ctx->last_score_ms = sms; ctx->last_prov_ms = pms;
  ctx->last_align_tiers[0] = fin[0]; ctx->last_align_tiers[1] = fin[1];
  uint64_t pos = 0;
  for (uint32_t i = 0; i < n_tasks; ++i) pos += cigar_len_out[i];
  if (cigar_bytes_used) *cigar_bytes_used = pos;
  if (!cigar_arena) return OTG_OK;
  if (pos > cigar_capacity) return otg_fail(ctx, OTG_ERR_CAPACITY, "cigar_capacity %llu too small, %llu needed", (unsigned long long)cigar_capacity, (unsigned long long)pos);
  std::vector<uint8_t> h_cig(slot[n_tasks] + 1);
  HIP_TRY(ctx, hipMemcpyAsync(h_cig.data(), d_cig, slot[n_tasks], hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  pos = 0;
  for (uint32_t i = 0; i < n_tasks; ++i) {
    cigar_off_out[i] = pos;
    memcpy(cigar_arena + pos, h_cig.data() + slot[i], cigar_len_out[i]);
    pos += cigar_len_out[i];
  }
  return OTG_OK;
}

int otg_edit_align_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const otg_align_task* tasks, uint32_t n_tasks,
                         int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                         uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_edit_align_batch: no context (no HIP device?)");
  if (cigar_bytes_used) *cigar_bytes_used = 0;
  if (n_tasks == 0) return OTG_OK;
  if (!seq_arena || !tasks || !scores_out || !cigar_len_out || (cigar_arena && !cigar_off_out))
    return otg_fail(ctx, OTG_ERR_ARG, "otg_edit_align_batch: NULL argument");
  if (ctx->heur_strategy != OTG_HEURISTIC_NONE)
    return otg_fail(ctx, OTG_ERR_ARG, "otg_edit_align_batch: exact alignment only; the context's heuristic is WFadaptive (its traceback is not implemented)");
  for (uint32_t i = 0; i < n_tasks; ++i)
    if (tasks[i].endsfree) return otg_fail(ctx, OTG_ERR_ARG, "otg_edit_align_batch: task %u is ends-free; only end-to-end alignment is supported", i);
  int rc = check_tasks(ctx, tasks, n_tasks, arena_bytes);
  if (rc) return rc;
  return edit_align_staged(ctx, seq_arena, arena_bytes, tasks, n_tasks, false, scores_out, cigar_off_out, cigar_len_out, cigar_arena, cigar_capacity,
                           cigar_bytes_used, nullptr);
}

int otg_edit_align_last_ms(otg_ctx* ctx, double* score_ms, double* prov_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_edit_align_last_ms: NULL context");
  if (score_ms) *score_ms = ctx->last_score_ms;
  if (prov_ms) *prov_ms = ctx->last_prov_ms;
  return OTG_OK;
}

// otg_edit_align_heur_batch and otg_edit_align_span_batch: the heuristic named per call; the second takes tasks with free ends too
static int edit_align_named(otg_ctx* ctx, const char* who, bool span, const uint8_t* seq_arena, uint64_t arena_bytes, const otg_align_task* tasks, uint32_t n_tasks,
                            int strategy, int min_wavefront_length, int max_distance_threshold, int steps_between_cutoffs,
                            int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                            uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used, uint64_t* cells_out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "%s: no context (no HIP device?)", who);
  if (cigar_bytes_used) *cigar_bytes_used = 0;
  if (strategy != OTG_HEURISTIC_NONE && strategy != OTG_HEURISTIC_WFADAPTIVE)
    return otg_fail(ctx, OTG_ERR_ARG, "%s: unknown strategy %d", who, strategy);
  if (strategy == OTG_HEURISTIC_WFADAPTIVE && (min_wavefront_length < 0 || max_distance_threshold < 0))
    return otg_fail(ctx, OTG_ERR_ARG, "%s: negative wavefront length or distance threshold", who);
  if (n_tasks == 0) return OTG_OK;
  if (!seq_arena || !tasks || !scores_out || !cigar_len_out || (cigar_arena && !cigar_off_out))
    return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL argument", who);
  if (!span)
    for (uint32_t i = 0; i < n_tasks; ++i)
      if (tasks[i].endsfree) return otg_fail(ctx, OTG_ERR_ARG, "%s: task %u is ends-free; only end-to-end alignment is supported", who, i);
  int rc = check_tasks(ctx, tasks, n_tasks, arena_bytes);
  if (rc) return rc;
  // the context's own heuristic is neither consulted nor left changed: the score chain reads it, so it is set for the call and put back on every path
  const int saved[4] = {ctx->heur_strategy, ctx->heur_min_wf_len, ctx->heur_max_dist, ctx->heur_steps};
  ctx->heur_strategy = strategy;
  if (strategy == OTG_HEURISTIC_WFADAPTIVE) {
    ctx->heur_min_wf_len = min_wavefront_length; ctx->heur_max_dist = max_distance_threshold;
    ctx->heur_steps = steps_between_cutoffs < 1 ? 1 : steps_between_cutoffs;
  }
  rc = edit_align_staged(ctx, seq_arena, arena_bytes, tasks, n_tasks, strategy == OTG_HEURISTIC_WFADAPTIVE, scores_out, cigar_off_out, cigar_len_out,
                         cigar_arena, cigar_capacity, cigar_bytes_used, cells_out);
  ctx->heur_strategy = saved[0]; ctx->heur_min_wf_len = saved[1]; ctx->heur_max_dist = saved[2]; ctx->heur_steps = saved[3];
  return rc;
}

int otg_edit_align_heur_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const otg_align_task* tasks, uint32_t n_tasks,
                              int strategy, int min_wavefront_length, int max_distance_threshold, int steps_between_cutoffs,
                              int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                              uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used, uint64_t* cells_out)
{
  return edit_align_named(ctx, "otg_edit_align_heur_batch", false, seq_arena, arena_bytes, tasks, n_tasks, strategy, min_wavefront_length,
                          max_distance_threshold, steps_between_cutoffs, scores_out, cigar_off_out, cigar_len_out, cigar_arena, cigar_capacity,
                          cigar_bytes_used, cells_out);
}

int otg_edit_align_span_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes, const otg_align_task* tasks, uint32_t n_tasks,
                              int strategy, int min_wavefront_length, int max_distance_threshold, int steps_between_cutoffs,
                              int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                              uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used, uint64_t* cells_out)
{
  return edit_align_named(ctx, "otg_edit_align_span_batch", true, seq_arena, arena_bytes, tasks, n_tasks, strategy, min_wavefront_length,
                          max_distance_threshold, steps_between_cutoffs, scores_out, cigar_off_out, cigar_len_out, cigar_arena, cigar_capacity,
                          cigar_bytes_used, cells_out);
}

int otg_edit_align_last_tiers(otg_ctx* ctx, uint32_t finished[2])
{
  if (!ctx || !finished) return otg_fail(ctx, OTG_ERR_ARG, "otg_edit_align_last_tiers: NULL argument");
  finished[0] = ctx->last_align_tiers[0]; finished[1] = ctx->last_align_tiers[1];
  return OTG_OK;
}

int otg_affine_align_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes,
                           const otg_align_task* tasks, uint32_t n_tasks,
                           int32_t mismatch, int32_t gap_open, int32_t gap_ext,
                           int32_t* scores_out, uint64_t* cigar_off_out, uint32_t* cigar_len_out,
                           uint8_t* cigar_arena, uint64_t cigar_capacity, uint64_t* cigar_bytes_used,
                           uint64_t* cells_out)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_affine_align_batch: no context (no HIP device?)");
  if (cigar_bytes_used) *cigar_bytes_used = 0;
  if (n_tasks == 0) return OTG_OK;
  if (!seq_arena || !tasks || !scores_out || !cigar_off_out || !cigar_len_out || !cigar_arena)
    return otg_fail(ctx, OTG_ERR_ARG, "otg_affine_align_batch: NULL argument");
  int rc = check_tasks(ctx, tasks, n_tasks, arena_bytes);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // device CIGAR slots: task i may emit at most pattern_len + text_len ops
  std::vector<uint64_t> slot(n_tasks + 1);
  slot[0] = 0;
  for (uint32_t i = 0; i < n_tasks; ++i) slot[i + 1] = slot[i] + (((uint64_t)tasks[i].pattern_len + tasks[i].text_len + 15) & ~15ull);
  uint8_t* d_arena = (uint8_t*)otg_slot(ctx, SLOT_ARENA, arena_bytes + 64);
  otg_align_task* d_tasks = (otg_align_task*)otg_slot(ctx, SLOT_TASKS, (size_t)n_tasks * sizeof(otg_align_task));
  int32_t* d_scores = (int32_t*)otg_slot(ctx, SLOT_SCORES, (size_t)n_tasks * sizeof(int32_t));
  uint64_t* d_cells = (uint64_t*)otg_slot(ctx, SLOT_CELLS, (size_t)n_tasks * sizeof(uint64_t));
  uint64_t* d_off = (uint64_t*)otg_slot(ctx, SLOT_CIG_OFF, (size_t)(n_tasks + 1) * sizeof(uint64_t));
  uint32_t* d_len = (uint32_t*)otg_slot(ctx, SLOT_CIG_LEN, (size_t)n_tasks * sizeof(uint32_t));
  uint8_t* d_cig = (uint8_t*)otg_slot(ctx, SLOT_CIG_ARENA, slot[n_tasks] + 64);
  if (!d_arena || !d_tasks || !d_scores || !d_cells || !d_off || !d_len || !d_cig) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemsetAsync(d_arena + arena_bytes, 0, 64, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_arena, seq_arena, arena_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_tasks, tasks, (size_t)n_tasks * sizeof(otg_align_task), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_off, slot.data(), (size_t)(n_tasks + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_scores, 0xff, (size_t)n_tasks * sizeof(int32_t), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_len, 0, (size_t)n_tasks * sizeof(uint32_t), ctx->stream));
  ctx->max_seq_len = max_len_of(tasks, n_tasks);
  rc = otg_launch_affine(ctx, d_arena, d_tasks, n_tasks, mismatch, gap_open, gap_ext, d_scores, d_off, d_len, d_cig, d_cells);
  if (rc) return rc;
  std::vector<uint8_t> h_cig(slot[n_tasks] + 1);
  HIP_TRY(ctx, hipMemcpyAsync(scores_out, d_scores, (size_t)n_tasks * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(cigar_len_out, d_len, (size_t)n_tasks * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (cells_out) HIP_TRY(ctx, hipMemcpyAsync(cells_out, d_cells, (size_t)n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h_cig.data(), d_cig, slot[n_tasks], hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t pos = 0;
  rc = OTG_OK;
  for (uint32_t i = 0; i < n_tasks; ++i) {
    if (scores_out[i] < 0)
      return otg_fail(ctx, scores_out[i] == -1 ? OTG_ERR_CAPACITY : OTG_ERR_FATAL,
                      "affine task %u failed on the device (code %d: -1 = backtrace storage exhausted)", i, scores_out[i]);
    cigar_off_out[i] = pos;
    if (pos + cigar_len_out[i] <= cigar_capacity) memcpy(cigar_arena + pos, h_cig.data() + slot[i], cigar_len_out[i]);
    else rc = OTG_ERR_CAPACITY;
    pos += cigar_len_out[i];
  }
  if (cigar_bytes_used) *cigar_bytes_used = pos;
  if (rc) return otg_fail(ctx, rc, "cigar_capacity %llu too small, %llu needed", (unsigned long long)cigar_capacity, (unsigned long long)pos);
  return OTG_OK;
}

} // extern "C"

// otg_cluster_batch, and otg_cluster_trace_batch when `trace` names the host arrays of the trace: those are mirrored on the device for the
// call (plain allocations: a test path, not a pooled one), filled by the TRACE instantiations of the kernel and copied back
static int cluster_batch_impl(otg_ctx* ctx, const char* who, const otg_params* params,
                              const double* dist, const uint64_t* dist_off,
                              const uint32_t* read_len, const uint64_t* len_off,
                              const uint32_t* n_valid, uint32_t n_regions,
                              int32_t* labels_out, int32_t* ic_out, int32_t* fc_out, double* bounds_out,
                              int exp_variant, const otg_cluster_trace* trace)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "%s: no context (no HIP device?)", who);
  if (n_regions == 0) return OTG_OK;
  if (!params || !dist_off || !read_len || !len_off || !n_valid || !labels_out || !ic_out || !fc_out)
    return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL argument", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint64_t n_dist = 0, n_len = 0;
  uint32_t n_max = 0;
  std::vector<uint32_t> wide;          // regions above the LDS scratch of the clustering kernel
  for (uint32_t r = 0; r < n_regions; ++r) {
    uint64_t n = n_valid[r];
    n_max = std::max<uint32_t>(n_max, n_valid[r]);
    if (n_valid[r] > OTG_CLUSTER_NMAX) wide.push_back(r);
    n_dist = std::max<uint64_t>(n_dist, dist_off[r] + n * (n ? n - 1 : 0) / 2);
    n_len = std::max<uint64_t>(n_len, len_off[r] + n);
  }
  if (n_dist && !dist) return otg_fail(ctx, OTG_ERR_ARG, "%s: dist is NULL", who);
  double* d_dist = (double*)otg_slot(ctx, SLOT_AUX0, (n_dist + 1) * sizeof(double));
  uint64_t* d_doff = (uint64_t*)otg_slot(ctx, SLOT_AUX1, (size_t)n_regions * sizeof(uint64_t));
  uint32_t* d_len = (uint32_t*)otg_slot(ctx, SLOT_AUX2, (n_len + 1) * sizeof(uint32_t));
  uint64_t* d_loff = (uint64_t*)otg_slot(ctx, SLOT_AUX3, (size_t)n_regions * sizeof(uint64_t));
  uint32_t* d_nv = (uint32_t*)otg_slot(ctx, SLOT_AUX4, (size_t)n_regions * sizeof(uint32_t));
  int32_t* d_lab = (int32_t*)otg_slot(ctx, SLOT_AUX5, (n_len + 1) * sizeof(int32_t));
  int32_t* d_ic = (int32_t*)otg_slot(ctx, SLOT_AUX6, (size_t)n_regions * 3 * sizeof(int32_t));
  double* d_bounds = (double*)otg_slot(ctx, SLOT_AUX7, (size_t)n_regions * 3 * sizeof(double));
  double* d_work = (double*)otg_slot(ctx, SLOT_AUX9, (n_dist + 1) * sizeof(double));
  if (!d_dist || !d_doff || !d_len || !d_loff || !d_nv || !d_lab || !d_ic || !d_bounds || !d_work) return OTG_ERR_HIP;
  int32_t* d_fc = d_ic + n_regions;
  int32_t* d_err = d_fc + n_regions;
  if (n_dist) HIP_TRY(ctx, hipMemcpyAsync(d_dist, dist, n_dist * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_doff, dist_off, (size_t)n_regions * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_len, read_len, n_len * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_loff, len_off, (size_t)n_regions * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_nv, n_valid, (size_t)n_regions * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_lab, 0xff, (n_len + 1) * sizeof(int32_t), ctx->stream));
  // the trace arrays on the device: one allocation, every byte 0xff (ints -1, doubles a NaN) where the kernel writes nothing
  struct TraceBuf {
    char* p = nullptr;
    ~TraceBuf() { if (p) (void)hipFree(p); }
  } tb;
  otg_cluster_trace d_tr{};
  struct Part { void** dev; void* host; size_t bytes, off; };
  std::vector<Part> parts;
  if (trace) {
    const size_t R = n_regions, G = OTG_TRACE_GRID, X = OTG_TRACE_EXT;
    parts = {{(void**)&d_tr.dens_raw, trace->dens_raw, R * G * 8, 0}, {(void**)&d_tr.dens, trace->dens, R * G * 8, 0}, {(void**)&d_tr.sums, trace->sums, R * G * 8, 0},
             {(void**)&d_tr.max_i, trace->max_i, R * X * 4, 0}, {(void**)&d_tr.max_v, trace->max_v, R * X * 8, 0},
             {(void**)&d_tr.min_i, trace->min_i, R * X * 4, 0}, {(void**)&d_tr.min_v, trace->min_v, R * X * 8, 0},
             {(void**)&d_tr.state, trace->state, R * 8 * 4, 0}, {(void**)&d_tr.scalars, trace->scalars, R * 2 * 8, 0},
             {(void**)&d_tr.merge, trace->merge, 2 * (size_t)n_len * 4, 0}, {(void**)&d_tr.height, trace->height, (size_t)n_len * 8, 0},
             {(void**)&d_tr.labels_first, trace->labels_first, (size_t)n_len * 4, 0}};
    size_t total = 0;
    for (Part& q : parts) {
      if (!q.host) return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL array in the trace", who);
      q.off = total;
      total += (q.bytes + 255) & ~(size_t)255;
    }
    HIP_TRY(ctx, hipMalloc((void**)&tb.p, total));
    HIP_TRY(ctx, hipMemsetAsync(tb.p, 0xff, total, ctx->stream));
    for (Part& q : parts) *q.dev = tb.p + q.off;
  }
  int rc = otg_launch_cluster(ctx, params, d_dist, d_doff, d_len, d_loff, d_nv, n_regions, n_max, wide.data(), (uint32_t)wide.size(), d_lab, d_ic, d_fc, d_bounds, d_err,
                              trace ? &d_tr : nullptr, exp_variant);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  for (const Part& q : parts)
    if (q.bytes) HIP_TRY(ctx, hipMemcpyAsync(q.host, tb.p + q.off, q.bytes, hipMemcpyDeviceToHost, ctx->stream));
  std::vector<int32_t> h_err(n_regions);
  HIP_TRY(ctx, hipMemcpyAsync(labels_out, d_lab, n_len * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ic_out, d_ic, (size_t)n_regions * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(fc_out, d_fc, (size_t)n_regions * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h_err.data(), d_err, (size_t)n_regions * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (bounds_out) HIP_TRY(ctx, hipMemcpyAsync(bounds_out, d_bounds, (size_t)n_regions * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t r = 0; r < n_regions; ++r)
    if (h_err[r] && !(trace && h_err[r] >= 1 && h_err[r] <= 5))      // a traced region that ends in 1-5 is delivered with its code (trace->state)
      return otg_fail(ctx, h_err[r] == 10 ? OTG_ERR_CAPACITY : OTG_ERR_FATAL,
                      "region %u: clustering failed with code %d (1-4: the reference exit(1)s here, src/otterclust.cpp:39-109; "
                      "5: std::sort emulation depth; 10: more valid reads than the clustering workspace was sized for)", r, h_err[r]);
  return OTG_OK;
}

extern "C" {

int otg_cluster_batch(otg_ctx* ctx, const otg_params* params,
                      const double* dist, const uint64_t* dist_off,
                      const uint32_t* read_len, const uint64_t* len_off,
                      const uint32_t* n_valid, uint32_t n_regions,
                      int32_t* labels_out, int32_t* ic_out, int32_t* fc_out, double* bounds_out)
{
  return cluster_batch_impl(ctx, "otg_cluster_batch", params, dist, dist_off, read_len, len_off, n_valid, n_regions, labels_out, ic_out, fc_out, bounds_out, -1, nullptr);
}

int otg_cluster_trace_batch(otg_ctx* ctx, const otg_params* params,
                            const double* dist, const uint64_t* dist_off,
                            const uint32_t* read_len, const uint64_t* len_off,
                            const uint32_t* n_valid, uint32_t n_regions,
                            int32_t* labels_out, int32_t* ic_out, int32_t* fc_out, double* bounds_out,
                            int exp_variant, const otg_cluster_trace* trace)
{
  if (!trace || exp_variant < -1 || exp_variant > 1) return otg_fail(ctx, OTG_ERR_ARG, "otg_cluster_trace_batch: no trace, or exp_variant not -1 / 0 / 1");
  return cluster_batch_impl(ctx, "otg_cluster_trace_batch", params, dist, dist_off, read_len, len_off, n_valid, n_regions, labels_out, ic_out, fc_out, bounds_out,
                            exp_variant, trace);
}

int otg_poa_consensus_batch(otg_ctx* ctx, const uint8_t* seq_arena, uint64_t arena_bytes,
                            const uint8_t* cigar_arena, uint64_t cigar_bytes,
                            const otg_poa_member* members, uint32_t n_members,
                            const otg_poa_graph* graphs, uint32_t n_graphs,
                            uint64_t* out_off, uint32_t* out_len,
                            uint8_t* out_arena, uint64_t out_capacity, uint64_t* out_bytes_used)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "otg_poa_consensus_batch: no context (no HIP device?)");
  if (out_bytes_used) *out_bytes_used = 0;
  if (n_graphs == 0) return OTG_OK;
  if (!seq_arena || !graphs || !out_off || !out_len || !out_arena || (n_members && (!members || !cigar_arena)))
    return otg_fail(ctx, OTG_ERR_ARG, "otg_poa_consensus_batch: NULL argument");
  for (uint32_t g = 0; g < n_graphs; ++g) {
    if (graphs[g].backbone_off + graphs[g].backbone_len > arena_bytes || (uint64_t)graphs[g].first_member + graphs[g].n_members > n_members)
      return otg_fail(ctx, OTG_ERR_ARG, "graph %u: backbone or member range out of bounds", g);
  }
  for (uint32_t m = 0; m < n_members; ++m)
    if (members[m].seq_off + members[m].seq_len > arena_bytes || members[m].cigar_off + members[m].cigar_len > cigar_bytes)
      return otg_fail(ctx, OTG_ERR_ARG, "member %u: sequence or op string out of bounds", m);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint8_t* d_arena = (uint8_t*)otg_slot(ctx, SLOT_ARENA, arena_bytes + 64);
  uint8_t* d_cig = (uint8_t*)otg_slot(ctx, SLOT_CIG_ARENA, cigar_bytes + 64);
  otg_poa_member* d_mem = (otg_poa_member*)otg_slot(ctx, SLOT_AUX0, (size_t)(n_members + 1) * sizeof(otg_poa_member));
  otg_poa_graph* d_gr = (otg_poa_graph*)otg_slot(ctx, SLOT_AUX1, (size_t)n_graphs * sizeof(otg_poa_graph));
  uint32_t* d_len = (uint32_t*)otg_slot(ctx, SLOT_AUX2, (size_t)n_graphs * sizeof(uint32_t));
  if (!d_arena || !d_cig || !d_mem || !d_gr || !d_len) return OTG_ERR_HIP;
  HIP_TRY(ctx, hipMemcpyAsync(d_arena, seq_arena, arena_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (cigar_bytes) HIP_TRY(ctx, hipMemcpyAsync(d_cig, cigar_arena, cigar_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_members) HIP_TRY(ctx, hipMemcpyAsync(d_mem, members, (size_t)n_members * sizeof(otg_poa_member), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_gr, graphs, (size_t)n_graphs * sizeof(otg_poa_graph), hipMemcpyHostToDevice, ctx->stream));
  std::vector<uint64_t> node_off;
  int rc = otg_launch_poa(ctx, d_arena, d_cig, d_mem, n_members, d_gr, graphs, n_graphs, d_len, node_off);
  if (rc) return rc;
  std::vector<uint32_t> h_start(n_graphs);
  std::vector<int32_t> h_status(n_graphs);
  std::vector<uint8_t> h_out(node_off[n_graphs] + 1);
  HIP_TRY(ctx, hipMemcpyAsync(out_len, d_len, (size_t)n_graphs * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h_start.data(), ctx->pool[SLOT_P29].p, (size_t)n_graphs * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h_status.data(), ctx->pool[SLOT_P28].p, (size_t)n_graphs * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h_out.data(), ctx->pool[SLOT_P17].p, node_off[n_graphs], hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t pos = 0;
  rc = OTG_OK;
  for (uint32_t g = 0; g < n_graphs; ++g) {
    if (h_status[g]) return otg_fail(ctx, OTG_ERR_FATAL, "POA graph %u failed on the device (status %d)", g, h_status[g]);
    out_off[g] = pos;
    if (pos + out_len[g] <= out_capacity) memcpy(out_arena + pos, h_out.data() + node_off[g] + h_start[g], out_len[g]);
    else rc = OTG_ERR_CAPACITY;
    pos += out_len[g];
  }
  if (out_bytes_used) *out_bytes_used = pos;
  if (rc) return otg_fail(ctx, rc, "out_capacity %llu too small, %llu needed", (unsigned long long)out_capacity, (unsigned long long)pos);
  return OTG_OK;
}

} // extern "C"

// The launch part of anallele_cluster on device-resident inputs: what otg_genotype_cluster_batch runs behind its uploads and the cohort path
// (cohort.hip) runs on its regrouped buffers.  d_height (2 x (na + 1) doubles, or NULL): the traced kernels, see genotype_kernel.
// metric / max_len: under OTG_GT_METRIC_EDIT the first matrix is built from alignments before the kernels (max_len = the longest allele); the
// caller has passed otg_genotype_metric_fits and calls otg_genotype_metric_finish after waiting for the stream.
// h_n_alleles is the host copy of d_n (wide routing).  d_gt holds 4 x (na + 1) int32 (gt, gt_l,
// gt_k, reps), d_ngt 2 x n_regions (n_gt, then the per-region error flags).  ctx->ev0 / ev1 are recorded around the kernels; no synchronisation.
int otg_genotype_resident(otg_ctx* ctx, const otg_params* params, const uint8_t* d_arena, const uint64_t* d_off, const uint32_t* d_len,
                          const uint32_t* d_first, const uint32_t* d_n, const uint32_t* h_n_alleles, uint32_t n_regions, const uint64_t* d_poff,
                          uint64_t n_pairs, uint64_t na, int32_t* d_gt, double* d_hsd, int32_t* d_ngt, double* d_height, int metric, uint32_t max_len)
{
  uint32_t a_max = 0;
  std::vector<uint32_t> wide;          // regions above the LDS scratch of the genotype kernel
  for (uint32_t r = 0; r < n_regions; ++r) {
    a_max = std::max<uint32_t>(a_max, h_n_alleles[r]);
    if (h_n_alleles[r] > OTG_CLUSTER_NMAX) wide.push_back(r);
  }
  int32_t *d_gtl = d_gt + (na + 1), *d_gtk = d_gtl + (na + 1), *d_reps = d_gtk + (na + 1), *d_err = d_ngt + n_regions;
  HIP_TRY(ctx, hipMemsetAsync(d_gt, 0xff, (na + 1) * 4 * 4, ctx->stream));
  const bool edit = metric == OTG_GT_METRIC_EDIT;
  if (edit && !ctx->ev2) HIP_TRY(ctx, hipEventCreate(&ctx->ev2));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = OTG_OK;
  if (edit) {      // the first matrix from alignments (genotype_edit.hip), into the slot the kernel reads it from; ev2 between the two parts
    if ((rc = otg_launch_genotype_edit_matrix(ctx, d_arena, d_off, d_len, d_first, d_n, n_regions, d_poff, n_pairs, na, max_len))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  }
  rc = otg_launch_genotype(ctx, params, d_arena, d_off, d_len, d_first, d_n, n_regions, d_poff, n_pairs, na, a_max, wide.data(), (uint32_t)wide.size(),
                           d_gt, d_gtl, d_gtk, d_hsd, d_ngt, d_reps, d_err, d_height, d_height ? d_height + (na + 1) : nullptr, edit);
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  return OTG_OK;
}

// otg_genotype_cluster_batch, and otg_genotype_cluster_trace_batch when `trace` is given: the traced kernels, then the matrices copied back
// from their slots (region r's pairs at the running sum of A (A - 1) / 2, its alleles at first_allele[r])
static int genotype_batch_impl(otg_ctx* ctx, const char* who, const otg_params* params, const uint8_t* seq_arena, uint64_t arena_bytes,
                               const uint64_t* seq_off, const uint32_t* seq_len,
                               const uint32_t* first_allele, const uint32_t* n_alleles, uint32_t n_regions,
                               int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out,
                               int32_t* n_gt_out, int32_t* reps_out, const otg_genotype_trace* trace,
                               int metric = OTG_GT_METRIC_LENGTH, double* dist_out = nullptr, uint64_t* n_aligned_out = nullptr)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_NO_DEVICE, "%s: no context (no HIP device?)", who);
  if (n_aligned_out) *n_aligned_out = 0;
  if (int rc = otg_genotype_metric_fits(ctx, who, metric, 0)) return rc;
  if (n_regions == 0) return OTG_OK;
  if (!params || !seq_arena || !seq_off || !seq_len || !first_allele || !n_alleles || !gt_out || !gt_l_out || !gt_k_out || !hsd_out || !n_gt_out || !reps_out)
    return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL argument", who);
  if (trace && (!trace->dl || !trace->dk || !trace->kvec || !trace->vnorm || !trace->height_l || !trace->height_k))
    return otg_fail(ctx, OTG_ERR_ARG, "%s: NULL array in the trace", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint64_t na = 0;
  std::vector<uint64_t> pair_off(n_regions + 1, 0);
  for (uint32_t r = 0; r < n_regions; ++r) {
    na = std::max<uint64_t>(na, (uint64_t)first_allele[r] + n_alleles[r]);
    uint64_t A = n_alleles[r];
    pair_off[r + 1] = pair_off[r] + A * (A ? A - 1 : 0) / 2;
  }
  uint32_t max_len = 0;
  for (uint64_t i = 0; i < na; ++i) {
    if (seq_off[i] + seq_len[i] > arena_bytes) return otg_fail(ctx, OTG_ERR_ARG, "allele %llu: sequence outside the arena", (unsigned long long)i);
    max_len = std::max(max_len, seq_len[i]);
  }
  if (int rc = otg_genotype_metric_fits(ctx, who, metric, pair_off[n_regions])) return rc;
  uint8_t* d_arena = (uint8_t*)otg_slot(ctx, SLOT_ARENA, arena_bytes + 64);
  uint64_t* d_off = (uint64_t*)otg_slot(ctx, SLOT_AUX0, (na + 1) * 8);
  uint32_t* d_len = (uint32_t*)otg_slot(ctx, SLOT_AUX1, (na + 1) * 4);
  uint32_t* d_first = (uint32_t*)otg_slot(ctx, SLOT_AUX2, (size_t)n_regions * 4);
  uint32_t* d_n = (uint32_t*)otg_slot(ctx, SLOT_AUX3, (size_t)n_regions * 4);
  uint64_t* d_poff = (uint64_t*)otg_slot(ctx, SLOT_AUX4, (size_t)(n_regions + 1) * 8);
  int32_t* d_gt = (int32_t*)otg_slot(ctx, SLOT_AUX5, (na + 1) * 4 * 4);
  double* d_hsd = (double*)otg_slot(ctx, SLOT_AUX6, (na + 1) * 8);
  int32_t* d_ngt = (int32_t*)otg_slot(ctx, SLOT_AUX7, (size_t)n_regions * 2 * 4);
  if (!d_arena || !d_off || !d_len || !d_first || !d_n || !d_poff || !d_gt || !d_hsd || !d_ngt) return OTG_ERR_HIP;
  int32_t *d_gtl = d_gt + (na + 1), *d_gtk = d_gtl + (na + 1), *d_reps = d_gtk + (na + 1), *d_err = d_ngt + n_regions;
  HIP_TRY(ctx, hipMemcpyAsync(d_arena, seq_arena, arena_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_off, seq_off, na * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_len, seq_len, na * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_first, first_allele, (size_t)n_regions * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_n, n_alleles, (size_t)n_regions * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_poff, pair_off.data(), (size_t)(n_regions + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  struct TraceBuf {
    double* p = nullptr;
    ~TraceBuf() { if (p) (void)hipFree(p); }
  } tb;
  if (trace) {
    HIP_TRY(ctx, hipMalloc((void**)&tb.p, 2 * (na + 1) * 8));
    HIP_TRY(ctx, hipMemsetAsync(tb.p, 0xff, 2 * (na + 1) * 8, ctx->stream));
  }
  int rc = otg_genotype_resident(ctx, params, d_arena, d_off, d_len, d_first, d_n, n_alleles, n_regions, d_poff, pair_off[n_regions], na, d_gt, d_hsd, d_ngt, tb.p,
                                 metric, max_len);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  bool finished = false;
  if (metric == OTG_GT_METRIC_EDIT) {      // a pair the chain gave up fails the call before anything is copied out: no partial results
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc2 = otg_genotype_metric_finish(ctx, metric, n_aligned_out)) return rc2;
    finished = true;
  }
  if (dist_out && pair_off[n_regions]) HIP_TRY(ctx, hipMemcpyAsync(dist_out, ctx->pool[SLOT_P20].p, pair_off[n_regions] * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (trace) {
    const uint64_t np = pair_off[n_regions];
    if (np) HIP_TRY(ctx, hipMemcpyAsync(trace->dl, ctx->pool[SLOT_P20].p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (np) HIP_TRY(ctx, hipMemcpyAsync(trace->dk, ctx->pool[SLOT_P21].p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(trace->kvec, ctx->pool[SLOT_P23].p, na * 65 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(trace->vnorm, ctx->pool[SLOT_P24].p, na * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(trace->height_l, tb.p, na * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(trace->height_k, tb.p + (na + 1), na * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  std::vector<int32_t> h_err(n_regions);
  HIP_TRY(ctx, hipMemcpyAsync(gt_out, d_gt, na * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(gt_l_out, d_gtl, na * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(gt_k_out, d_gtk, na * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(reps_out, d_reps, na * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(hsd_out, d_hsd, na * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(n_gt_out, d_ngt, (size_t)n_regions * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h_err.data(), d_err, (size_t)n_regions * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!finished) { if (int rc2 = otg_genotype_metric_finish(ctx, metric, n_aligned_out)) return rc2; }
  for (uint32_t r = 0; r < n_regions; ++r)
    if (h_err[r]) return otg_fail(ctx, OTG_ERR_CAPACITY, "region %u: %u alleles, more than the clustering workspace was sized for", r, n_alleles[r]);
  return OTG_OK;
}

extern "C" {

int otg_genotype_cluster_batch(otg_ctx* ctx, const otg_params* params, const uint8_t* seq_arena, uint64_t arena_bytes,
                               const uint64_t* seq_off, const uint32_t* seq_len,
                               const uint32_t* first_allele, const uint32_t* n_alleles, uint32_t n_regions,
                               int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out,
                               int32_t* n_gt_out, int32_t* reps_out)
{
  return genotype_batch_impl(ctx, "otg_genotype_cluster_batch", params, seq_arena, arena_bytes, seq_off, seq_len, first_allele, n_alleles, n_regions,
                             gt_out, gt_l_out, gt_k_out, hsd_out, n_gt_out, reps_out, nullptr);
}

int otg_genotype_cluster_trace_batch(otg_ctx* ctx, const otg_params* params, const uint8_t* seq_arena, uint64_t arena_bytes,
                                     const uint64_t* seq_off, const uint32_t* seq_len,
                                     const uint32_t* first_allele, const uint32_t* n_alleles, uint32_t n_regions,
                                     int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out,
                                     int32_t* n_gt_out, int32_t* reps_out, const otg_genotype_trace* trace)
{
  if (!trace) return otg_fail(ctx, OTG_ERR_ARG, "otg_genotype_cluster_trace_batch: no trace");
  return genotype_batch_impl(ctx, "otg_genotype_cluster_trace_batch", params, seq_arena, arena_bytes, seq_off, seq_len, first_allele, n_alleles, n_regions,
                             gt_out, gt_l_out, gt_k_out, hsd_out, n_gt_out, reps_out, trace);
}

int otg_genotype_cluster_metric_batch(otg_ctx* ctx, const otg_params* params, const uint8_t* seq_arena, uint64_t arena_bytes,
                                      const uint64_t* seq_off, const uint32_t* seq_len,
                                      const uint32_t* first_allele, const uint32_t* n_alleles, uint32_t n_regions,
                                      int32_t* gt_out, int32_t* gt_l_out, int32_t* gt_k_out, double* hsd_out,
                                      int32_t* n_gt_out, int32_t* reps_out, int32_t metric, double* dist_out, uint64_t* n_aligned_out)
{
  return genotype_batch_impl(ctx, "otg_genotype_cluster_metric_batch", params, seq_arena, arena_bytes, seq_off, seq_len, first_allele, n_alleles, n_regions,
                             gt_out, gt_l_out, gt_k_out, hsd_out, n_gt_out, reps_out, nullptr, metric, dist_out, n_aligned_out);
}

int otg_genotype_metric_last_ms(otg_ctx* ctx, double* align_ms, double* cluster_ms)
{
  if (!ctx) return otg_fail(nullptr, OTG_ERR_ARG, "otg_genotype_metric_last_ms: NULL context");
  if (align_ms) *align_ms = ctx->last_gt_align_ms;
  if (cluster_ms) *cluster_ms = ctx->last_gt_cluster_ms;
  return OTG_OK;
}

int otg_last_kernel_ms(otg_ctx* ctx, double* ms)
{
  if (!ctx || !ms) return otg_fail(ctx, OTG_ERR_ARG, "otg_last_kernel_ms: NULL argument");
  *ms = ctx->last_kernel_ms;
  return OTG_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------
static inline uint64_t asu64(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static inline double asf64(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

static double host_exp_variant(double x, bool use_fma)
{
  // glibc 2.28+ exp (sysdeps/ieee754/dbl-64/e_exp.c), N = 128; use_fma mirrors the x86-64 ifunc'd FMA build
  const double InvLn2N = 0x1.71547652b82fep0 * 128, NegLn2hiN = -0x1.62e42fefa0000p-8, NegLn2loN = -0x1.cf79abc9e3b3ap-47;
  const double Shift = 0x1.8p52;
  const double C2 = 0x1.ffffffffffdbdp-2, C3 = 0x1.555555555543cp-3, C4 = 0x1.55555cf172b91p-5, C5 = 0x1.1111167a4d017p-7;
  auto F = [use_fma](double a, double b, double c) { return use_fma ? std::fma(a, b, c) : a * b + c; };
  uint32_t abstop = (uint32_t)(asu64(x) >> 52) & 0x7ff;
  if (abstop - 0x3c9 >= 0x408 - 0x3c9) {
    if (abstop - 0x3c9 >= 0x80000000u) return 1.0 + x;
    if (abstop >= 0x409) {
      if (asu64(x) == asu64(-INFINITY)) return 0.0;
      if (abstop >= 0x7ff) return 1.0 + x;
      return (asu64(x) >> 63) ? 0.0 : INFINITY;
    }
    abstop = 0;
  }
  double kd = F(InvLn2N, x, Shift);      // the FMA build fuses z + Shift (gcc contracts it); the non-FMA build rounds z first
  uint64_t ki = asu64(kd);
  kd -= Shift;
  double r = F(kd, NegLn2loN, F(kd, NegLn2hiN, x));
  uint64_t idx = 2 * (ki % 128), top = ki << 45;
  double tail = asf64(OTG_EXP_TAB[idx]);
  uint64_t sbits = OTG_EXP_TAB[idx + 1] + top;
  double r2 = r * r;
  double tmp = use_fma ? F(r2 * r2, F(r, C5, C4), F(r2, F(r, C3, C2), tail + r))
                       : tail + r + r2 * (C2 + r * C3) + r2 * r2 * (C4 + r * C5);
  if (abstop == 0) {
    double scale, y;
    if ((ki & 0x80000000) == 0) { sbits -= 1009ull << 52; scale = asf64(sbits); y = 0x1p1009 * F(scale, tmp, scale); return y; }
    sbits += 1022ull << 52; scale = asf64(sbits);
    double st = scale * tmp;
    y = scale + st;
    if (y < 1.0) { double hi, lo; lo = scale - y + st; hi = 1.0 + y; lo = 1.0 - hi + y + lo; y = (hi + lo) - 1.0; if (y == 0.0) y = 0.0; }
    return 0x1p-1022 * y;
  }
  double scale = asf64(sbits);
  return F(scale, tmp, scale);
}

// The probe of otg_create: which restatement equals the host libm's exp() on every argument of a set that tells the two builds apart.  The
// builds differ on about 5 in 10^4 arguments, and the FMA build's fused `InvLn2N*x + Shift` shows only next to the half-way points
// -(j + 1/2) ln2/128 of the table index, so the set holds those points with both neighbours (j < 16384: down to -88.7) and 2^17 arguments of
// the KDE's own form -(z*z/2), z in [0, 39) — x <= 0 throughout, as in the KDE.  Returns the variant with no mismatch (1 = FMA, 0 = non-FMA);
// when both or neither is clean, the one with fewer mismatches, FMA on a tie.  The counts go to the caller: a host libm that matches neither
// build shows as a non-zero count of the chosen variant (otg_exp_probe_mismatches), not as a silent vote.
static int exp_probe(uint64_t* n_args, uint64_t* n_differ, uint64_t* mism_fma, uint64_t* mism_nofma)
{
  uint64_t na = 0, nd = 0, mf = 0, mn = 0;
  auto one = [&](double x) {
    volatile double xv = x;                  // the call must reach libm: no constant folding
    const uint64_t ref = asu64(std::exp(xv)), a = asu64(host_exp_variant(x, true)), b = asu64(host_exp_variant(x, false));
    ++na; nd += (a != b); mf += (a != ref); mn += (b != ref);
  };
  const double step = 0x1.62e42fefa39efp-1 / 128;      // ln2 / 128
  for (int j = 0; j < 16384; ++j) {
    const double h = -((double)j + 0.5) * step;
    one(std::nextafter(h, 0.0)); one(h); one(std::nextafter(h, -INFINITY));
  }
  uint64_t s = 88172645463325252ULL;
  for (int i = 0; i < (1 << 17); ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const double u = (double)(s >> 11) * (1.0 / 9007199254740992.0);
    const double z = u * 39.0;
    one(-(z * z / 2));
  }
  if (n_args) *n_args = na;
  if (n_differ) *n_differ = nd;
  if (mism_fma) *mism_fma = mf;
  if (mism_nofma) *mism_nofma = mn;
  return mn < mf ? 0 : 1;
}

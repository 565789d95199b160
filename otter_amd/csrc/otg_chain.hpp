// otg_chain.hpp — host plumbing shared by the aligner tier chains (wfa_edit.hip, wfa_affine.hip, wfa_adaptive.hip, edit_align.hip): the layout
// of SLOT_COUNTERS, the kernel_ms / launches timer, the todo cursor a chain hands from tier to tier, and the environment switches.
#pragma once
#include "otg_common.hpp"
#include <cstddef>
#include <cstdlib>

// ---- SLOT_COUNTERS: one size from its first use on, so nothing in it ever moves.  A chain zeroes its own group when it starts (otg_counters).
struct OtgCounters {
  struct Tier { uint32_t ticket, overflow; };     // the persistent blocks' ticket counter; length of the list of what the tier gives up
  struct ExactEdit {
    uint32_t wf_ticket, tier_ticket[OTG_MYERS_TIERS];      // the capped wavefront pass; the bit-parallel tiers
    Tier wide, last;
    // the router kernels take this group as ONE array: len[t] = length of lists[t] (the last: the wide wavefront tier's), then the sampling
    // router's own list.  The chain copies it to ctx->edit_hist for the next pass of its kind.
    struct Routes { uint32_t len[OTG_MYERS_TIERS + 1], wf_len; } routes;
  } exact_edit;
  struct ExactAffine {
    uint32_t seg[OTG_REG_TIERS + 2];              // the counting sort's bounds: register tier t owns sorted[seg[t] .. seg[t + 1])
    uint32_t reg_overflow, reg_ticket[OTG_REG_TIERS], bound_ticket;
    Tier a, b, c;
    // NOT zeroed per launch: cells visited, accumulated over a run (otg_assemble_run zeroes it); behind it the clock sums of a -DOTG_REG_TIMING build
    unsigned long long visited, unused_, reg_timing[7];
  } exact_affine;
  struct AdaptiveEdit { Tier packed1024, packed4096, packed16384, bytes2048, bytes16384, last; } adaptive_edit;
  struct AdaptiveAffine { Tier win256, win1024, win4096, bytes1024, last; } adaptive_affine;
};
static_assert(offsetof(OtgCounters, exact_affine.visited) % 8 == 0 && offsetof(OtgCounters, exact_affine.reg_timing) % 8 == 0, "64-bit atomics need 8-byte alignment");
static_assert(offsetof(OtgCounters, exact_affine.reg_timing) - offsetof(OtgCounters, exact_affine.visited) == 16, "wfa_affine_reg.hip adds its clock sums at visited + 2 .. visited + 8");
static_assert(sizeof(OtgCounters::ExactEdit::Routes) <= 16 * sizeof(uint32_t), "ctx->edit_hist holds 16 words per kind of pass");

// A chain's group of the slot, its first `bytes` bytes zeroed on the stream (a slot just created: all of it).  nullptr on failure (error recorded).
template <class G>
G* otg_counters(otg_ctx* ctx, G OtgCounters::*group, size_t bytes = sizeof(G))
{
  const bool fresh = !ctx->pool[SLOT_COUNTERS].p;
  OtgCounters* c = (OtgCounters*)otg_slot(ctx, SLOT_COUNTERS, sizeof(OtgCounters));
  if (!c) return nullptr;
  ctx->last_chain = (int)((const char*)&(c->*group) - (const char*)c);      // the chain that runs now owns what the accessors of the last launch read
  const hipError_t e = fresh ? hipMemsetAsync(c, 0, sizeof(OtgCounters), ctx->stream) : hipMemsetAsync(&(c->*group), 0, bytes, ctx->stream);
  if (e != hipSuccess) { otg_fail(ctx, OTG_ERR_HIP, "zeroing the chain counters failed"); return nullptr; }
  return &(c->*group);
}
// device counter: (score, diagonal) cells the exact gap-affine tiers visited; null while the slot does not exist
inline unsigned long long* otg_affine_visited(otg_ctx* ctx) { OtgCounters* c = (OtgCounters*)ctx->pool[SLOT_COUNTERS].p; return c ? &c->exact_affine.visited : nullptr; }

// ---- kernel_ms / launches: a chain records ctx->ev0 in front of its first tier and ctx->ev1 behind its last when a time is asked for
// (kernel_ms non-null); only then does the host wait for ev1, here
inline int otg_timer_add(otg_ctx* ctx, float* kernel_ms, uint64_t* launches)
{
  if (!kernel_ms) return OTG_OK;
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
  float ms = 0;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *kernel_ms += ms;
  if (launches) *launches += 1;
  return OTG_OK;
}

// ---- where a tier reads its work: a list of task slots (null: the slots 0 .. n - 1), its length on the device (n) or, n null, immediate
struct OtgTodo {
  const uint32_t *list, *n; uint32_t imm;
  void next(const uint32_t* gave_up, const uint32_t* len) { list = gave_up; n = len; imm = 0; }      // the next tier reads what this one gave up
};

// ---- environment switches (kept in a function-local static where the switch is read once per process)
inline int otg_env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
inline bool otg_env_set(const char* name) { return getenv(name) != nullptr; }

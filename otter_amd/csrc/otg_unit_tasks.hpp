// otg_unit_tasks.hpp — what the kernels that align tasks (allele, unit) share (unitalign.hip, tract.hip): the view of a call's alleles, units and
// task lists on the device, the bins (tier, class, length bucket) and the scatter of the classified tasks into the order their launches walk.
// Device code only; each translation unit gets its own copy of the kernel.
#pragma once
#include "otg_common.hpp"
#include "otg_unitalign_core.hpp"
#include <cstdlib>
#include <cstring>

namespace {

using namespace otg_unitalign_core;

constexpr uint32_t UA_T = 256;                                   // threads of every workgroup here
constexpr uint32_t UA_NBINS = 2u * UA_CLASSES * UA_BUCKETS;      // (tier, class, bucket)
constexpr uint32_t UA_NO_BIN = 0xffffffffu;

struct UaIn {
  OtgRows rows;
  OtgUnitSource u;
  const uint32_t* task_seq; const uint32_t* task_unit;
  __device__ __forceinline__ uint32_t seq(uint32_t t) const { return task_seq ? task_seq[t] : t; }
  __device__ __forceinline__ uint32_t unit(uint32_t t) const { return task_unit ? task_unit[t] : t; }
  __device__ __forceinline__ uint32_t unit_len(uint32_t k) const { return u.d_unit_off ? u.d_unit_len[k] : u.d_motifs[k].period; }
  __device__ __forceinline__ const uint8_t* unit_at(uint32_t k) const { return u.d_units + (u.d_unit_off ? u.d_unit_off[k] : (uint64_t)k * u.unit_stride); }
};

// ---- binning: the scatter of the classified tasks into their bins' stretches of the order
__global__ __launch_bounds__(UA_T) void ua_scatter(uint32_t n, const uint32_t* __restrict__ task_bin, const uint32_t* __restrict__ start,
                                                  uint32_t* __restrict__ cursor, uint32_t* __restrict__ order)
{
  const uint32_t t = blockIdx.x * UA_T + threadIdx.x;
  if (t >= n) return;
  const uint32_t bin = task_bin[t];
  if (bin == UA_NO_BIN) return;
  order[start[bin] + atomicAdd(&cursor[bin], 1u)] = t;            // start[bin] + count(bin) = start[bin + 1] <= n
}

// a switch of the environment: set, not empty and not "0"
inline bool ua_env(const char* name)
{
  const char* e = getenv(name);
  return e && *e && strcmp(e, "0") != 0;
}

} // namespace

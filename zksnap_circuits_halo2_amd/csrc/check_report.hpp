// The report record of the witness checks (include/zkhip.h zkhip_check_report) and the one reduction the three check kernels share:
// rowvm.hip k_row_vm<R, true> (gates), rowvm.hip k_check_copies (copy constraints), lookup.hip k_lookup_member (lookup membership).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace zkhip {

// report[0] = failures (a count), report[1] = first (a minimum): both exact whatever the launch geometry and the order of arrival
constexpr unsigned long long CHECK_NONE = ~0ull;

// Every lane of the wavefront that is still running calls this with its verdict and its item's index.  One ballot; a wavefront with no failing
// lane issues no atomic (a satisfied witness writes nothing); otherwise the lowest failing lane adds the popcount and offers its index.  The
// callers number their items upwards with the lane, so the lowest failing lane holds the wavefront's lowest failing index.  Both are ordinary
// vector atomics on global memory (global_atomic_add_x2 / global_atomic_umin_x2, no return value).
__device__ __forceinline__ void check_report_wave(bool failing, unsigned long long index, unsigned long long* __restrict__ report) {
  const unsigned long long mask = __ballot(failing);
  if (!mask) return;
  const uint32_t lowest = (uint32_t)__ffsll(mask) - 1u;
  if ((threadIdx.x & 63u) == lowest) {
    atomicAdd(report, (unsigned long long)__popcll(mask));
    atomicMin(report + 1, index);
  }
}

}  // namespace zkhip

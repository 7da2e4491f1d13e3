// Whether the first two single-lane steps of the reduction plan (reduce_plan.hpp) are carried by one launch (msm.hip: msm_reduce_buckets,
// k_pyramid_pair), host arithmetic only so that it can be checked on its own (tests/cpp/reduce_fuse_host_check.cpp).  The plan keeps
// describing single steps; the fused launch replaces l[0] and l[1]: it reads the buckets (stride l[0].in_stride) and writes the state of
// l[1] (stride l[1].out_stride), one lane per four buckets and five additions per lane.
//
// Measured (profiles/r30_pyramid_fused_steps.txt) and not fused: later pairs -- their launches have Z lanes of three additions beside the X
// lanes of five and lost 6 us at 2^17 lanes (steps 3 + 4 of 32 sets of 2^15), and with X lanes alone they are too small (2^16 lanes, one
// wavefront per SIMD at half the issue rate: +8 us for steps 3 + 4 of 2^19 buckets) --, and the form with two lanes per output.
#pragma once
#include "reduce_plan.hpp"

namespace zkhip {

// Lanes of the fused launch over all bucket sets between which it beats the two single steps: one round of two wavefronts on each of the
// chip's 1024 SIMDs (the kernel's occupancy).  2^17 lanes: 77.9 us against 53.4 + 37.3 (one set of 2^19 buckets), 77.5 against 52.5 + 34.6
// (16 sets of 2^15); 2^18 lanes, two rounds: 164.2 against 96.9 + 67.1 (32 sets of 2^15) (profiles/r30_pyramid_fused_steps.txt).
constexpr size_t REDUCE_FUSE_MIN_LANES = (size_t)1 << 17;
constexpr size_t REDUCE_FUSE_END_LANES = (size_t)1 << 18;

inline bool reduce_fuse_first_pair(const reduce_plan& p, int WB) {
  if (p.n < 2 || p.l[0].kind != REDUCE_STEP || p.l[1].kind != REDUCE_STEP || p.l[0].s != 1 || p.l[0].N < 8) return false;
  const size_t lanes = (size_t)(p.l[0].N / 4) * (size_t)WB;
  return lanes >= REDUCE_FUSE_MIN_LANES && lanes < REDUCE_FUSE_END_LANES;
}

}  // namespace zkhip

// Launch plan of the bucket reduction (msm.hip: msm_reduce_buckets), host arithmetic only so that it can be checked on its own
// (tests/cpp/reduce_plan_host_check.cpp).  Pyramid step s (1-based) turns the state [X (N) | Z^0 .. Z^(s-2) (N/2 each)], N = B >> (s-1),
// into [X' (N/2) | Z'^0 .. Z'^(s-1) (N/4 each)] with reduce_step_adds(N, s) additions; steps 1 .. c-2 leave X with 2 elements.
// The plan is a function of (B, WB) alone:
//   STEP       one lane per addition   (a step of more than REDUCE_QUAD_MAX additions over all bucket sets: throughput-bound)
//   STEP_QUAD  a quad per addition     (latency-bound, one level per launch)
//   PAIR_QUAD  steps s and s+1 in one launch, two quads per output (latency-bound and fewer than REDUCE_PAIR_MAX_LANES lanes)
//   FINISH     every remaining step, the weighted sum and the store in one workgroup per bucket set (WB <= REDUCE_FINISH_MAX_SETS)
// With more bucket sets than REDUCE_FINISH_MAX_SETS the plan is single steps only and the caller launches the weighted sum itself.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zkhip {

constexpr size_t REDUCE_QUAD_MAX = 65536;             // additions of a step up to which four lanes share one (profiles/r04_pyramid_quad_threshold_ab.txt)
constexpr size_t REDUCE_PAIR_MAX_LANES = (size_t)1 << 16;   // a pair launch (8 lanes per output) stays below this many lanes: a quarter of the chip's
constexpr int REDUCE_FINISH_MAX_SETS = 64;            // bucket sets up to which the finish kernel replaces the last launches
constexpr uint32_t REDUCE_FINISH_ADDS = 128;          // additions of the finish kernel's first level: one per quad of its 512 threads
constexpr uint32_t REDUCE_FINISH_ADDS2 = 80;          // bound of its second level (below); the two bound the LDS ping-pong buffers
constexpr int REDUCE_MAX_LAUNCHES = 32;               // c <= 21: at most c - 2 = 19 steps + the finish

enum reduce_kind : int { REDUCE_STEP = 0, REDUCE_STEP_QUAD = 1, REDUCE_PAIR_QUAD = 2, REDUCE_FINISH = 3 };

struct reduce_launch {
  int kind;
  int s;                   // first step the launch executes
  int steps;               // steps it consumes (FINISH: every step that is left, possibly none)
  uint32_t N;              // X elements of its input state
  uint32_t in_stride;      // elements per bucket set of its input = N + (s - 1) N / 2
  uint32_t out_stride;     // elements per bucket set of its output (FINISH: 0, it writes results)
};

struct reduce_plan {
  int n;                   // launches
  int nz;                  // Z rows of the final state = number of pyramid steps
  bool finish;             // the last launch is FINISH; otherwise the state after the last launch has stride `last_stride`
  uint32_t last_stride;
  reduce_launch l[REDUCE_MAX_LAUNCHES];
};

inline uint32_t reduce_step_adds(uint32_t N, int s) { return N / 2 + (uint32_t)s * (N / 4); }       // = elements of the state after step s
inline uint32_t reduce_state_elems(uint32_t N, int s) { return N + (uint32_t)(s - 1) * (N / 2); }   // state before step s

// B: buckets per set (a power of two >= 2), WB: bucket sets.  Returns false when the plan does not fit (never for B <= 2^20).
inline bool reduce_make_plan(uint32_t B, int WB, reduce_plan* p) {
  p->n = 0;
  p->finish = WB <= REDUCE_FINISH_MAX_SETS;
  uint32_t N = B, stride = B;
  int s = 1;
  while (N > 2) {
    const uint32_t adds = reduce_step_adds(N, s);
    if (p->finish && adds <= REDUCE_FINISH_ADDS) break;          // the finish kernel takes it from here
    if (p->n >= REDUCE_MAX_LAUNCHES - 1) return false;
    reduce_launch& L = p->l[p->n++];
    L.s = s; L.N = N; L.in_stride = stride;
    const uint32_t adds2 = N >= 8 ? reduce_step_adds(N / 2, s + 1) : 0;
    const bool pair = p->finish && N >= 8 && adds2 > REDUCE_FINISH_ADDS      // (both steps lie before the finish kernel's first)
                      && (size_t)adds2 * (size_t)WB * 8 < REDUCE_PAIR_MAX_LANES;
    if ((size_t)adds * (size_t)WB > REDUCE_QUAD_MAX) { L.kind = REDUCE_STEP; L.steps = 1; L.out_stride = adds; }
    else if (pair) { L.kind = REDUCE_PAIR_QUAD; L.steps = 2; L.out_stride = adds2; }
    else { L.kind = REDUCE_STEP_QUAD; L.steps = 1; L.out_stride = adds; }
    stride = L.out_stride;
    N >>= L.steps;
    s += L.steps;
  }
  if (p->finish) {
    // LDS bounds of the finish kernel: its first level writes <= REDUCE_FINISH_ADDS elements; N / 2 + s N / 4 <= 128 with s >= 1 gives
    // N <= 128, so the second level writes adds / 2 + N / 8 <= 64 + 16 elements
    if (N > 2 && (reduce_step_adds(N, s) > REDUCE_FINISH_ADDS || (N > 4 && reduce_step_adds(N / 2, s + 1) > REDUCE_FINISH_ADDS2))) return false;
    reduce_launch& L = p->l[p->n++];
    L.kind = REDUCE_FINISH; L.s = s; L.N = N; L.in_stride = stride; L.out_stride = 0;
    L.steps = 0;
    for (uint32_t M = N; M > 2; M >>= 1) L.steps++;
    s += L.steps;
  }
  p->nz = s - 1;
  p->last_stride = stride;
  return true;
}

}  // namespace zkhip

// Steps 8 - 9 of the MSM, the bucket reduction (msm.hip: msm_reduce_buckets): every launch of it, and the index maps of its pyramid kernels,
// host arithmetic that g++ compiles too so that both can be executed on their own (tests/cpp/reduce_plan_host_check.cpp).  Pyramid step s
// (1-based) turns the state [X (N) | Z^0 .. Z^(s-2) (N/2 each)], N = B >> (s-1), into [X' (N/2) | Z'^0 .. Z'^(s-1) (N/4 each)] with
// reduce_step_adds(N, s) additions; steps 1 .. c-2 leave X with 2 elements.  The plan is a function of (B, WB, prepared) alone, one entry per
// kernel launch:
//   STEP         one lane per addition   (a step of more than REDUCE_QUAD_MAX additions over all bucket sets: throughput-bound)
//   PAIR         steps 1 and 2 in one launch, one lane per four buckets and five additions per lane: where both are STEP and the launch is one
//                round of two wavefronts per SIMD (REDUCE_FUSE_MIN_LANES <= lanes < REDUCE_FUSE_END_LANES)
//   STEP_QUAD    a quad per addition     (latency-bound, one level per launch)
//   PAIR_QUAD    steps s and s+1 in one launch, two quads per output (latency-bound and fewer than REDUCE_PAIR_MAX_LANES lanes)
//   FINISH       every remaining step, the weighted sum and the store in one workgroup per bucket set (WB <= REDUCE_FINISH_MAX_SETS)
//   HORNER_QUAD  the weighted sum behind a pyramid of single steps (more sets than FINISH takes), a workgroup of quads per set; above
//                REDUCE_HORNER_QUAD_MAX_SETS sets HORNER, one lane per term (throughput-bound)
//   STORE, FOLD  where the weighted-sum kernel did not write the results itself (`direct`): a prepared MSM's result per set, or the window fold
//
// Measured (profiles/r30_pyramid_fused_steps.txt) and not fused: later pairs -- their launches have Z lanes of three additions beside the X
// lanes of five and lost 6 us at 2^17 lanes (steps 3 + 4 of 32 sets of 2^15), and with X lanes alone they are too small (2^16 lanes, one
// wavefront per SIMD at half the issue rate: +8 us for steps 3 + 4 of 2^19 buckets) --, and the form with two lanes per output.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define REDUCE_HD __host__ __device__ __forceinline__
#else
#define REDUCE_HD inline
#endif

namespace zkhip {

constexpr size_t REDUCE_QUAD_MAX = 65536;             // additions of a step up to which four lanes share one (profiles/r04_pyramid_quad_threshold_ab.txt)
constexpr size_t REDUCE_PAIR_MAX_LANES = (size_t)1 << 16;   // a pair launch (8 lanes per output) stays below this many lanes: a quarter of the chip's
constexpr int REDUCE_FINISH_MAX_SETS = 64;            // bucket sets up to which the finish kernel replaces the last launches
constexpr uint32_t REDUCE_FINISH_ADDS = 128;          // additions of the finish kernel's first level: one per quad of its 512 threads
constexpr uint32_t REDUCE_FINISH_ADDS2 = 80;          // bound of its second level (below); the two bound the LDS ping-pong buffers
constexpr int REDUCE_HORNER_QUAD_MAX_SETS = 2048;     // bucket sets up to which the weighted sum runs on quads and writes a prepared MSM's results itself
constexpr int REDUCE_MAX_LAUNCHES = 32;               // c <= 21: at most c - 2 = 19 steps + the weighted sum + the store

// Lanes of the fused launch over all bucket sets between which it beats the two single steps: one round of two wavefronts on each of the
// chip's 1024 SIMDs (the kernel's occupancy).  2^17 lanes: 77.9 us against 53.4 + 37.3 (one set of 2^19 buckets), 77.5 against 52.5 + 34.6
// (16 sets of 2^15); 2^18 lanes, two rounds: 164.2 against 96.9 + 67.1 (32 sets of 2^15) (profiles/r30_pyramid_fused_steps.txt).
constexpr size_t REDUCE_FUSE_MIN_LANES = (size_t)1 << 17;
constexpr size_t REDUCE_FUSE_END_LANES = (size_t)1 << 18;

// workgroup sizes of the kernels whose grids the plan computes (msm.hip: their launch bounds and their launches)
constexpr int PYRAMID_THREADS = 128;         // k_pyramid_step, k_pyramid_step_quad, k_pyramid_pair_quad, k_pyramid_pair
constexpr int FINISH_THREADS = 512;          // 128 quads.  (1024 threads leave a wavefront 128 VGPRs: the quad addition then spills ~400 of them)
constexpr int HORNER_THREADS = 64;           // k_window_horner: two 32-lane groups, one per bucket set
constexpr int STORE_THREADS = 64;            // k_store_results

enum reduce_kind : int { REDUCE_STEP = 0, REDUCE_STEP_QUAD = 1, REDUCE_PAIR_QUAD = 2, REDUCE_FINISH = 3, REDUCE_PAIR = 4,
                         REDUCE_HORNER_QUAD = 5, REDUCE_HORNER = 6, REDUCE_STORE = 7, REDUCE_FOLD = 8 };

struct reduce_launch {
  int kind;
  int s;                   // first step the launch executes (behind the pyramid: nz + 1)
  int steps;               // steps it consumes (FINISH: every step that is left, possibly none; behind the pyramid: 0)
  uint32_t N;              // X elements of its input state
  uint32_t in_stride;      // elements per bucket set of its input = N + (s - 1) N / 2 (STORE, FOLD: 0, they read the window sums)
  uint32_t out_stride;     // elements per bucket set of its output (0 where it writes window sums or results)
  uint32_t grid;           // workgroups in x; the pyramid kernels take the bucket set from a second grid dimension of WB rows
};

struct reduce_plan {
  int n;                   // launches
  int nz;                  // Z rows of the final state = number of pyramid steps
  bool finish;             // the pyramid ends in FINISH; otherwise the state after its last launch has stride `last_stride`
  bool direct;             // the weighted-sum kernel (FINISH or HORNER_QUAD) writes the results itself: no STORE behind it
  uint32_t last_stride;
  reduce_launch l[REDUCE_MAX_LAUNCHES];
};

REDUCE_HD uint32_t reduce_step_adds(uint32_t N, int s) { return N / 2 + (uint32_t)s * (N / 4); }       // = elements of the state after step s
REDUCE_HD uint32_t reduce_state_elems(uint32_t N, int s) { return N + (uint32_t)(s - 1) * (N / 2); }   // state before step s
inline uint32_t reduce_blocks(size_t lanes, int threads) { return (uint32_t)((lanes + (size_t)threads - 1) / (size_t)threads); }

// Operand map of one pyramid step (the equations: msm.hip section 8): output element t < reduce_step_adds(N, s) of step s is in[ia] + in[ib]
REDUCE_HD void reduce_step_operands(uint32_t N, int s, uint32_t t, uint32_t& ia, uint32_t& ib) {
  if (t < N / 2) {
    ia = 2 * t; ib = 2 * t + 1;
  } else {
    const uint32_t r = t - N / 2;
    const uint32_t l = r / (N / 4), u = r % (N / 4);
    if ((int)l == s - 1) { ia = 4 * u + 1; ib = 4 * u + 3; }
    else { ia = N + l * (N / 2) + 2 * u; ib = ia + 1; }
  }
}

// Steps s and s + 1 at once (k_pyramid_pair_quad): output element o < reduce_step_adds(N / 2, s + 1) is the sum of two pair sums, and
// pair `half` (0, 1) of it is in[ia] + in[ib].  N >= 8.
REDUCE_HD void reduce_pair_quad_operands(uint32_t N, int s, uint32_t o, uint32_t half, uint32_t& ia, uint32_t& ib) {
  if (o < N / 4) {
    ia = 4 * o + 2 * half; ib = ia + 1;
  } else {
    const uint32_t r = o - N / 4;
    const uint32_t l = r / (N / 8), v = r % (N / 8);
    if ((int)l == s - 1) { ia = 8 * v + 4 * half + 1; ib = ia + 2; }
    else if ((int)l == s) { ia = 8 * v + 4 * half + 2; ib = ia + 1; }
    else { ia = N + l * (N / 2) + 4 * v + 2 * half; ib = ia + 1; }
  }
}

// Steps 1 and 2 at once (k_pyramid_pair): lane t < N / 4 reads X[4t + j], j = 0 .. 3, writes X''[t], and of the lane pair (2v, 2v + 1) the
// even lane writes Z''^0[v], the odd one Z''^1[v].  N >= 8.
REDUCE_HD uint32_t reduce_pair_in(uint32_t t, uint32_t j) { return 4 * t + j; }
REDUCE_HD uint32_t reduce_pair_x_out(uint32_t t) { return t; }
REDUCE_HD uint32_t reduce_pair_z_out(uint32_t N, uint32_t t) { return N / 4 + ((t & 1) ? N / 8 : 0) + t / 2; }

// B: buckets per set (a power of two >= 2), WB: bucket sets, prepared: every set's weighted sum is a result (otherwise the sets are the
// windows of one MSM).  Returns false when the plan does not fit (never for B <= 2^20).
inline bool reduce_make_plan(uint32_t B, int WB, bool prepared, reduce_plan* p) {
  p->n = 0;
  p->finish = WB <= REDUCE_FINISH_MAX_SETS;
  p->direct = prepared && WB <= REDUCE_HORNER_QUAD_MAX_SETS;
  const size_t sets = (size_t)WB;
  uint32_t N = B, stride = B;
  int s = 1;
  while (N > 2) {
    const uint32_t adds = reduce_step_adds(N, s);
    if (p->finish && adds <= REDUCE_FINISH_ADDS) break;          // the finish kernel takes it from here
    if (p->n >= REDUCE_MAX_LAUNCHES - 2) return false;
    reduce_launch& L = p->l[p->n++];
    L.s = s; L.N = N; L.in_stride = stride;
    const uint32_t adds2 = N >= 8 ? reduce_step_adds(N / 2, s + 1) : 0;
    const bool pair_quad = p->finish && N >= 8 && adds2 > REDUCE_FINISH_ADDS      // (both steps lie before the finish kernel's first)
                           && (size_t)adds2 * sets * 8 < REDUCE_PAIR_MAX_LANES;
    const size_t pair_lanes = (size_t)(N / 4) * sets;
    const bool pair = s == 1 && N >= 8 && (size_t)adds2 * sets > REDUCE_QUAD_MAX  // (step 2 is a single-lane step as well)
                      && pair_lanes >= REDUCE_FUSE_MIN_LANES && pair_lanes < REDUCE_FUSE_END_LANES;
    if ((size_t)adds * sets > REDUCE_QUAD_MAX) {
      if (pair) { L.kind = REDUCE_PAIR; L.steps = 2; L.out_stride = adds2; L.grid = reduce_blocks(N / 4, PYRAMID_THREADS); }
      else { L.kind = REDUCE_STEP; L.steps = 1; L.out_stride = adds; L.grid = reduce_blocks(adds, PYRAMID_THREADS); }
    }
    else if (pair_quad) { L.kind = REDUCE_PAIR_QUAD; L.steps = 2; L.out_stride = adds2; L.grid = reduce_blocks((size_t)8 * adds2, PYRAMID_THREADS); }
    else { L.kind = REDUCE_STEP_QUAD; L.steps = 1; L.out_stride = adds; L.grid = reduce_blocks((size_t)4 * adds, PYRAMID_THREADS); }
    stride = L.out_stride;
    N >>= L.steps;
    s += L.steps;
  }
  reduce_launch& S = p->l[p->n++];            // the weighted sum
  S.s = s; S.N = N; S.in_stride = stride; S.out_stride = 0; S.steps = 0;
  if (p->finish) {
    // LDS bounds of the finish kernel: its first level writes <= REDUCE_FINISH_ADDS elements; N / 2 + s N / 4 <= 128 with s >= 1 gives
    // N <= 128, so the second level writes adds / 2 + N / 8 <= 64 + 16 elements
    if (N > 2 && (reduce_step_adds(N, s) > REDUCE_FINISH_ADDS || (N > 4 && reduce_step_adds(N / 2, s + 1) > REDUCE_FINISH_ADDS2))) return false;
    S.kind = REDUCE_FINISH; S.grid = (uint32_t)WB;
    for (uint32_t M = N; M > 2; M >>= 1) S.steps++;
    s += S.steps;
  }
  else if (WB <= REDUCE_HORNER_QUAD_MAX_SETS) { S.kind = REDUCE_HORNER_QUAD; S.grid = (uint32_t)WB; }
  else { S.kind = REDUCE_HORNER; S.grid = reduce_blocks(sets * 32, HORNER_THREADS); }
  p->nz = s - 1;
  p->last_stride = stride;
  if (!p->direct) p->l[p->n++] = {prepared ? REDUCE_STORE : REDUCE_FOLD, s, 0, 2, 0, 0, prepared ? reduce_blocks(sets, STORE_THREADS) : 1u};
  return true;
}

}  // namespace zkhip

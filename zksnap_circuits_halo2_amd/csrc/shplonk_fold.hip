// The SHPLONK accumulation scalars on the device (include/zkhip.h, "the batch verifier"; the arithmetic and the plan's layout are shplonk_fold.hpp's):
//
//   k_shplonk_scalars    one workgroup per proof, in five phases with a barrier between them: the point differences and the y and v tables into
//                        LDS; the sets' products and the pairs' partial numerators; ONE lane's inversion; the sets' weights and the pairs' Lagrange
//                        weights; then one lane per column of the proof's A row, and the G column as strided partial sums joined through LDS
//                        (gwc_fold.hpp's lanes and join).  The plan's tables are shared by the batch and read through the caches; a proof's
//                        evaluations are read once, consecutive lanes on consecutive 32-byte elements.  A plan that one wave covers runs 64 lanes.
//
// While one lane inverts (about 11 k instructions) the others wait at the barrier: a workgroup is a proof, and a batch has a workgroup per proof
// to fill the chip with.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include "fr_vec.hpp"
#include "shplonk_fold.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

__device__ __forceinline__ void sf_store_zero(uint32_t* p) {
  const uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  store_words(p, w);
}

// plan: the words shplonk_plan_marshal builds.  One pointer for the head and the six tables, as in k_gwc_scalars.
__global__ void __launch_bounds__(SHPLONK_THREADS) k_shplonk_scalars(const uint32_t* __restrict__ evals, const uint32_t* __restrict__ points, const uint32_t* __restrict__ plan,
                                                                     uint32_t* __restrict__ rows_a, uint32_t* __restrict__ rows_c, uint32_t* __restrict__ status) {
  __shared__ fe diff[SHPLONK_MAX_POINTS], ytab[GWC_V_BITS], vpow[SHPLONK_MAX_SETS], zset[SHPLONK_MAX_SETS], wset[SHPLONK_MAX_SETS], lag[SHPLONK_MAX_PAIRS],
      xpow[SHPLONK_MAX_POINTS], part[SHPLONK_THREADS], shared[2];      // shared: Z_T, norm
  __shared__ uint32_t bad;
  const sf_layout lay = sf_layout_read(plan);
  const uint32_t* point_omega = plan + lay.point_omega;
  const uint32_t* pair_coeff = plan + lay.pair_coeff;
  const uint32_t* set_start = plan + lay.set_start;
  const uint32_t* pair_word = plan + lay.pair_word;
  const uint32_t* slot_word = plan + lay.slot_word;
  const uint32_t* query_word = plan + lay.query_word;
  const uint32_t t = threadIdx.x, T = blockDim.x;
  const uint64_t p = blockIdx.x;
  const uint32_t* point = points + p * 32;                  // x, y, v, u
  const uint32_t n_cols = 2 + lay.n_slots + 1;              // (n_slots <= 65536: no wrap)
  uint32_t* row_a = rows_a + p * n_cols * 8;
  auto pair = [&](uint32_t j) { return pair_word[j]; };

  // 1. points: the three tables in a wave each where there are four (t - 64, t - 128 wrap above every count for the lanes in front)
  const uint32_t vt = T > 64 ? t - 64 : t, yt = T > 64 ? t - 128 : t;
  if (t < lay.n_points) diff[t] = sf_diff<Fr>(gf_reduce<Fr>(gf_load5(point + 24)), gf_reduce<Fr>(gf_load5(point)), gf_load5(point_omega + t * 8));
  if (vt < lay.n_sets) vpow[vt] = ip_pow<Fr>(gf_reduce<Fr>(gf_load5(point + 16)), vt);
  if (yt < GWC_V_BITS) ytab[yt] = gf_v_entry<Fr>(gf_reduce<Fr>(gf_load5(point + 8)), yt);
  __syncthreads();

  // 2. sets: task 0 is Z_T, tasks 1 .. n_sets the sets' Z_i, the tasks behind them the pairs' partial numerators (at most 1 + 64 + 256 tasks)
  for (uint32_t task = t; task < 1 + lay.n_sets + lay.n_pairs; task += T) {
    if (task == 0) {
      shared[0] = sf_outside<Fr>(diff, lay.n_points, 0);
    } else if (task <= lay.n_sets) {
      const uint32_t i = task - 1;
      zset[i] = sf_outside<Fr>(diff, lay.n_points, sf_set_mask(set_start[i], set_start[i + 1], pair));
    } else {
      const uint32_t j = task - 1 - lay.n_sets, i = pair_word[j] >> 16;
      lag[j] = sf_numerator<Fr>(diff, set_start[i], set_start[i + 1], j, pair);
    }
  }
  __syncthreads();

  // 3. the inversion, and the proof's status
  if (t == 0) {
    const sf_inverse inv = sf_invert<Fr>(gf_reduce<Fr>(gf_load5(point)), zset[0]);
    shared[1] = inv.norm;
    sf_xinv_powers<Fr>(xpow, lay.longest, inv.xinv);
    bad = inv.bad ? 1u : 0u;
    status[p] = inv.bad ? 1u : 0u;
  }
  __syncthreads();
  if (bad) {                                                // the same in every lane: the workgroup leaves together
    for (uint32_t c = t; c < n_cols; c += T) sf_store_zero(row_a + (uint64_t)c * 8);
    if (t == 0) sf_store_zero(rows_c + p * 8);
    return;
  }

  // 4. weights: w_i per set; a pair's lane makes its set's w_i again (two products) in place of a barrier behind the sets' lanes
  for (uint32_t task = t; task < lay.n_sets + lay.n_pairs; task += T) {
    if (task < lay.n_sets) {
      wset[task] = sf_weight<Fr>(vpow[task], zset[task], shared[1]);
    } else {
      const uint32_t j = task - lay.n_sets, i = pair_word[j] >> 16;
      lag[j] = sf_lagrange<Fr>(sf_weight<Fr>(vpow[i], zset[i], shared[1]), lag[j], xpow[set_start[i + 1] - set_start[i] - 1], gf_load5(pair_coeff + j * 8));
    }
  }
  __syncthreads();

  // 5. columns: H', H, the slots; then G
  for (uint32_t c = t; c < n_cols - 1; c += T) {
    if (c == 0) gf_store_ext(row_a, gf_reduce<Fr>(gf_load5(point + 24)));
    else if (c == 1) gf_store_ext(row_a + 8, sf_h_column<Fr>(shared[0], shared[1]));
    else gf_store_ext(row_a + (uint64_t)c * 8, gf_coeff<Fr>(wset, ytab, slot_word[c - 2]));
  }
  if (t == 0) gf_store_ext(rows_c + p * 8, fe_one<Fr>());
  const uint32_t* record = evals + p * lay.n_evals * 8;
  part[t] = gf_g_lane<Fr>(lag, ytab, lay.n_evals, t, T, [&](uint32_t q) { return query_word[q]; }, [&](uint32_t q) { return gf_load5(record + (uint64_t)q * 8); });
  gf_join_block(part, t, T);
  if (t == 0) gf_store_ext(row_a + (uint64_t)(n_cols - 1) * 8, gf_neg<Fr>(part[0]));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// Validates the plan and builds the words the kernel reads; touches no device.  ZKHIP_EINVAL with the error text set, or ZKHIP_OK and `blob`.
int shplonk_plan_marshal(const zkhip_shplonk_plan* plan, uint32_t k, const uint64_t* omega, std::vector<uint32_t>* blob) {
  const char* who = "shplonk_scalars";
  if (!plan) { set_error("%s: null plan", who); return ZKHIP_EINVAL; }
  const uint32_t n_evals = plan->n_evals, n_sets = plan->n_sets, n_slots = plan->n_slots, n_points = plan->n_points;
  if (n_sets < 1 || n_sets > SHPLONK_MAX_SETS) { set_error("%s: %u rotation sets: 1 .. %u", who, n_sets, SHPLONK_MAX_SETS); return ZKHIP_EINVAL; }
  if (n_points < 1 || n_points > SHPLONK_MAX_POINTS) { set_error("%s: %u super points: 1 .. %u", who, n_points, SHPLONK_MAX_POINTS); return ZKHIP_EINVAL; }
  if (n_evals < 1 || n_evals > GWC_MAX_EVALS) { set_error("%s: %u evaluations: 1 .. %u", who, n_evals, GWC_MAX_EVALS); return ZKHIP_EINVAL; }
  if (n_slots < 1 || n_slots > GWC_MAX_SLOTS) { set_error("%s: %u polynomial slots: 1 .. %u", who, n_slots, GWC_MAX_SLOTS); return ZKHIP_EINVAL; }
  if (!plan->point_rotation || !plan->set_start || !plan->set_point || !plan->slot_set || !plan->slot_pos || !plan->query_slot || !plan->query_point) {
    set_error("%s: null plan array", who);
    return ZKHIP_EINVAL;
  }
  if (k > 28) { set_error("%s: k = %u > 28", who, k); return ZKHIP_EINVAL; }
  if (!omega || !fr_words_canonical(omega)) { set_error("%s: omega is null or not a canonical Fr", who); return ZKHIP_EINVAL; }
  for (uint32_t t = 0; t < n_points; t++) {
    if (plan->point_rotation[t] >= ((uint64_t)1 << k)) { set_error("%s: point %u: rotation %u is not reduced mod 2^%u", who, t, plan->point_rotation[t], k); return ZKHIP_EINVAL; }
    for (uint32_t s = 0; s < t; s++)
      if (plan->point_rotation[s] == plan->point_rotation[t]) { set_error("%s: points %u and %u are one rotation", who, s, t); return ZKHIP_EINVAL; }
  }
  // the CSR list of the sets: from 0, every set with a point, at most SHPLONK_MAX_PAIRS pairs (checked entry by entry: nothing behind them is read)
  if (plan->set_start[0] != 0) { set_error("%s: set_start[0] = %u", who, plan->set_start[0]); return ZKHIP_EINVAL; }
  for (uint32_t i = 0; i < n_sets; i++) {
    if (plan->set_start[i + 1] <= plan->set_start[i]) { set_error("%s: set %u has no point", who, i); return ZKHIP_EINVAL; }
    if (plan->set_start[i + 1] > SHPLONK_MAX_PAIRS) { set_error("%s: more than %u (set, point) pairs", who, SHPLONK_MAX_PAIRS); return ZKHIP_EINVAL; }
  }
  const uint32_t n_pairs = plan->set_start[n_sets];
  uint32_t longest = 0;
  for (uint32_t i = 0; i < n_sets; i++) {
    uint64_t mask = 0;
    for (uint32_t j = plan->set_start[i]; j < plan->set_start[i + 1]; j++) {
      const uint32_t pt = plan->set_point[j];
      if (pt >= n_points) { set_error("%s: set %u: point %u of %u", who, i, pt, n_points); return ZKHIP_EINVAL; }
      if ((mask >> pt) & 1u) { set_error("%s: set %u holds point %u twice", who, i, pt); return ZKHIP_EINVAL; }
      mask |= (uint64_t)1 << pt;
    }
    const uint32_t len = plan->set_start[i + 1] - plan->set_start[i];          // <= n_points <= 64: the points of a set are distinct
    if (len > longest) longest = len;
  }
  uint64_t expected = 0;                                                       // sum over the slots of their sets' lengths
  for (uint32_t s = 0; s < n_slots; s++) {
    if (plan->slot_set[s] >= n_sets || plan->slot_pos[s] >= (1u << GWC_V_BITS)) {
      set_error("%s: slot %u: set %u of %u, position %u (below 2^%u)", who, s, plan->slot_set[s], n_sets, plan->slot_pos[s], GWC_V_BITS);
      return ZKHIP_EINVAL;
    }
    expected += plan->set_start[plan->slot_set[s] + 1] - plan->set_start[plan->slot_set[s]];
  }
  const sf_layout lay = sf_layout_of(n_evals, n_sets, n_slots, n_points, n_pairs, longest);
  blob->assign(lay.words, 0);
  uint32_t* out = blob->data();
  std::vector<uint64_t> seen(n_slots, 0);                                      // per slot: the positions inside its set that a query has named
  for (uint32_t q = 0; q < n_evals; q++) {
    const uint32_t s = plan->query_slot[q], pt = plan->query_point[q];
    if (s >= n_slots || pt >= n_points) { set_error("%s: query %u: slot %u of %u, point %u of %u", who, q, s, n_slots, pt, n_points); return ZKHIP_EINVAL; }
    const uint32_t i = plan->slot_set[s], begin = plan->set_start[i], end = plan->set_start[i + 1];
    uint32_t j = begin;
    while (j < end && plan->set_point[j] != pt) j++;
    if (j == end) { set_error("%s: query %u: point %u is not in set %u of slot %u", who, q, pt, i, s); return ZKHIP_EINVAL; }
    if ((seen[s] >> (j - begin)) & 1u) { set_error("%s: query %u: slot %u is queried twice at point %u", who, q, s, pt); return ZKHIP_EINVAL; }
    seen[s] |= (uint64_t)1 << (j - begin);
    out[lay.query_word + q] = gf_query_word(j, plan->slot_pos[s]);
  }
  if (expected != n_evals) { set_error("%s: %u evaluations, the slots' sets ask for %llu", who, n_evals, (unsigned long long)expected); return ZKHIP_EINVAL; }
  out[0] = n_evals; out[1] = n_sets; out[2] = n_slots; out[3] = n_points; out[4] = n_pairs; out[5] = longest;
  uint32_t ow[8];
  std::memcpy(ow, omega, 32);
  const fe w = gf_reduce<Fr>(fe_from_ext_lazy(ow));
  std::vector<fe> omega_pow(n_points);
  for (uint32_t t = 0; t < n_points; t++) {
    omega_pow[t] = ip_pow<Fr>(w, plan->point_rotation[t]);
    uint32_t words[8];
    fe_to_ext<Fr>(omega_pow[t], words);
    std::memcpy(out + lay.point_omega + (size_t)t * 8, words, 32);
  }
  for (uint32_t i = 0; i < n_sets; i++) {
    out[lay.set_start + i] = plan->set_start[i];
    for (uint32_t j = plan->set_start[i]; j < plan->set_start[i + 1]; j++) {
      out[lay.pair_word + j] = plan->set_point[j] | (i << 16);
      uint32_t words[8];
      fe_to_ext<Fr>(sf_pair_coefficient<Fr>(plan->set_point, plan->set_start[i], plan->set_start[i + 1], j, [&](uint32_t pt) { return omega_pow[pt]; }), words);
      std::memcpy(out + lay.pair_coeff + (size_t)j * 8, words, 32);
    }
  }
  out[lay.set_start + n_sets] = n_pairs;
  for (uint32_t s = 0; s < n_slots; s++) out[lay.slot_word + s] = gf_query_word(plan->slot_set[s], plan->slot_pos[s]);
  return ZKHIP_OK;
}

int shplonk_scalars_device(const std::vector<uint32_t>& blob, const uint32_t* d_evals, const uint32_t* d_points, uint64_t n_proofs, uint32_t* d_rows_a,
                           uint32_t* d_rows_c, uint32_t* d_status, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring) {
  if (blob.size() < SF_HEAD_WORDS || ws_bytes < blob.size() * 4) { set_error("shplonk_scalars: workspace too small"); return ZKHIP_EINVAL; }
  const sf_layout lay = sf_layout_read(blob.data());
  // through the argument ring, a slot's worth at a time, as gwc_scalars_device does
  for (size_t at = 0; at < blob.size() * 4; at += arg_ring::SLOT_BYTES) {
    const size_t bytes = blob.size() * 4 - at < arg_ring::SLOT_BYTES ? blob.size() * 4 - at : arg_ring::SLOT_BYTES;
    const int rc = upload_args(ring, (char*)ws + at, (const char*)blob.data() + at, bytes, stream);
    if (rc != ZKHIP_OK) return rc;
  }
  uint32_t widest = lay.n_evals > lay.n_slots + 2 ? lay.n_evals : lay.n_slots + 2;
  if (1 + lay.n_sets + lay.n_pairs > widest) widest = 1 + lay.n_sets + lay.n_pairs;
  const uint32_t threads = widest <= SHPLONK_THREADS_SHORT ? SHPLONK_THREADS_SHORT : SHPLONK_THREADS;
  hipLaunchKernelGGL(k_shplonk_scalars, dim3((unsigned)n_proofs), dim3(threads), 0, stream, d_evals, d_points, (const uint32_t*)ws, d_rows_a, d_rows_c, d_status);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

// The batch verifier's scalar side on the device (include/zkhip.h, "the batch verifier"; the arithmetic is gwc_fold.hpp's):
//
//   k_gwc_scalars    one workgroup per proof: the u and v tables into LDS, then one lane per column of the proof's A row (and, for the witness
//                    columns, of its C row), then the G column as strided partial sums joined through LDS.  The plan's tables (omega^rot per set,
//                    a word per query, the CSR list of every polynomial's queries) are shared by the batch and read through the caches; a proof's
//                    evaluations are read once, consecutive lanes on consecutive 32-byte elements.  A plan that one wave covers runs 64 lanes.
//   k_fold_own       out[i][j] = +- r_i rows[i][j]: one lane per element, one product each.
//   k_fold_shared    per shared column and span of FOLD_SPAN rows one workgroup: lane t sums the rows t, t + 256, ... of the span (a fused
//                    multiply-add per row), the 256 sums are joined through LDS.  One span: the column's sum is written.  More: the sums go to
//                    scratch, [span][column], and
//   k_fold_finish    joins them, one workgroup per column (at most FOLD_SPAN of them: 2^24 rows).
//
// A fold reads a column with a stride of n_cols elements: every 32-byte element is a sector of its own, which is what the rows' layout (a proof's
// scalars side by side, as the MSM behind the fold wants them) costs here; the batches of a verifier are a few MB at the most.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include "fr_vec.hpp"
#include "gwc_fold.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

// (the element loads and stores and gf_join_block, the join through LDS, are gwc_fold.hpp's: shplonk_fold.hip uses the same)
// plan: the words gwc_scalars_device uploads -- omega^rot per set (8 words each) | a word per query | slot_start [n_slots + 1] | slot_query [n_evals].
// One pointer for the four tables: the kernel sits at the SGPR limit, and every argument kept for its whole length is a spilled scalar elsewhere.
__global__ void __launch_bounds__(GWC_THREADS) k_gwc_scalars(const uint32_t* __restrict__ evals, const uint32_t* __restrict__ points, const uint32_t* __restrict__ plan,
                                                             uint32_t n_evals, uint32_t n_sets, uint32_t n_slots, uint32_t* __restrict__ rows_a,
                                                             uint32_t* __restrict__ rows_c) {
  __shared__ fe vtab[GWC_V_BITS], upow[GWC_MAX_SETS], part[GWC_THREADS];
  const uint32_t* set_omega = plan;
  const uint32_t* query_word = plan + n_sets * 8;
  const uint32_t* slot_start = query_word + n_evals;
  const uint32_t* slot_query = slot_start + n_slots + 1;
  const uint32_t t = threadIdx.x, T = blockDim.x;
  const uint64_t p = blockIdx.x;
  const uint32_t* point = points + p * 24;                  // x, v, u
  if (t < GWC_V_BITS) vtab[t] = gf_v_entry<Fr>(gf_reduce<Fr>(gf_load5(point + 8)), t);
  const uint32_t ut = T > 64 ? t - 64 : t;                  // the u table in a wave of its own where there is one (t < 64 wraps above every n_sets)
  if (ut < n_sets) upow[ut] = ip_pow<Fr>(gf_reduce<Fr>(gf_load5(point + 16)), ut);
  __syncthreads();
  const uint32_t n_cols = n_sets + n_slots + 1;
  uint32_t* row_a = rows_a + p * n_cols * 8;
  for (uint32_t c = t; c < n_cols - 1; c += T) {            // (n_cols <= 64 + 65536 + 1: no wrap)
    if (c < n_sets) {
      gf_store_ext(row_a + (uint64_t)c * 8, gf_witness_column<Fr>(upow[c], gf_reduce<Fr>(gf_load5(point)), gf_load5(set_omega + c * 8)));
      gf_store_ext(rows_c + (p * n_sets + c) * 8, upow[c]);
    } else {
      const uint32_t s = c - n_sets;
      gf_store_ext(row_a + (uint64_t)c * 8, gf_slot_column<Fr>(upow, vtab, slot_start[s], slot_start[s + 1], [&](uint32_t i) { return query_word[slot_query[i]]; }));
    }
  }
  const uint32_t* record = evals + p * n_evals * 8;
  part[t] = gf_g_lane<Fr>(upow, vtab, n_evals, t, T, [&](uint32_t q) { return query_word[q]; }, [&](uint32_t q) { return gf_load5(record + (uint64_t)q * 8); });
  gf_join_block(part, t, T);
  if (t == 0) gf_store_ext(row_a + (uint64_t)(n_cols - 1) * 8, gf_neg<Fr>(part[0]));
}

__global__ void __launch_bounds__(FOLD_THREADS) k_fold_own(const uint32_t* __restrict__ rows, uint32_t n_cols, uint32_t n_own, const uint32_t* __restrict__ r,
                                                           uint64_t n_rows, uint32_t negate, uint32_t* __restrict__ out) {
  const uint64_t idx = (uint64_t)blockIdx.x * FOLD_THREADS + threadIdx.x;
  if (idx >= n_rows * n_own) return;
  const uint64_t i = idx / n_own;
  const uint32_t j = (uint32_t)(idx % n_own);
  gf_store_packed(out + idx * 8, gf_scale<Fr>(gf_load5(r + i * 8), gf_load0(rows + (i * n_cols + j) * 8), negate != 0));
}

// blockIdx.x: the shared column; blockIdx.y: the span of rows.  gridDim.y == 1: out = the column's sum; else partials[span][column]
__global__ void __launch_bounds__(FOLD_THREADS) k_fold_shared(const uint32_t* __restrict__ rows, uint32_t n_cols, uint32_t n_own, const uint32_t* __restrict__ r,
                                                              uint64_t n_rows, uint32_t negate, uint32_t* __restrict__ out, uint32_t* __restrict__ partials) {
  __shared__ fe part[FOLD_THREADS];
  const uint32_t t = threadIdx.x, j = blockIdx.x, n_shared = gridDim.x;
  const uint64_t row0 = (uint64_t)blockIdx.y * FOLD_SPAN;
  const uint64_t left = n_rows - row0;                      // (the grid has no span behind the rows)
  const uint32_t count = left < FOLD_SPAN ? (uint32_t)left : FOLD_SPAN;
  const uint32_t* column = rows + (row0 * n_cols + n_own + j) * 8;
  const uint32_t* mult = r + row0 * 8;
  part[t] = gf_fold_lane<Fr>(count, t, FOLD_THREADS, [&](uint32_t i) { return gf_load5(mult + (uint64_t)i * 8); },
                             [&](uint32_t i) { return gf_load0(column + (uint64_t)i * n_cols * 8); });
  gf_join_block(part, t, FOLD_THREADS);
  if (t != 0) return;
  if (gridDim.y == 1) gf_store_packed(out + (uint64_t)j * 8, negate ? gf_neg<Fr>(part[0]) : part[0]);
  else gf_store_packed(partials + ((uint64_t)blockIdx.y * n_shared + j) * 8, part[0]);
}

__global__ void __launch_bounds__(FOLD_THREADS) k_fold_finish(const uint32_t* __restrict__ partials, uint32_t n_spans, uint32_t negate, uint32_t* __restrict__ out) {
  __shared__ fe part[FOLD_THREADS];
  const uint32_t t = threadIdx.x, j = blockIdx.x, n_shared = gridDim.x;
  part[t] = gf_join_lane<Fr>(n_spans, t, FOLD_THREADS, [&](uint32_t b) { return gf_load0(partials + ((uint64_t)b * n_shared + j) * 8); });
  gf_join_block(part, t, FOLD_THREADS);
  if (t == 0) gf_store_packed(out + (uint64_t)j * 8, negate ? gf_neg<Fr>(part[0]) : part[0]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
int gwc_plan_validate(const zkhip_gwc_plan* plan, uint32_t k, const uint64_t* omega) {
  const char* who = "gwc_scalars";
  if (!plan) { set_error("%s: null plan", who); return ZKHIP_EINVAL; }
  if (plan->n_sets < 1 || plan->n_sets > GWC_MAX_SETS) { set_error("%s: %u point sets: 1 .. %u", who, plan->n_sets, GWC_MAX_SETS); return ZKHIP_EINVAL; }
  if (plan->n_evals < 1 || plan->n_evals > GWC_MAX_EVALS) { set_error("%s: %u evaluations: 1 .. %u", who, plan->n_evals, GWC_MAX_EVALS); return ZKHIP_EINVAL; }
  if (plan->n_slots < 1 || plan->n_slots > GWC_MAX_SLOTS) { set_error("%s: %u polynomial slots: 1 .. %u", who, plan->n_slots, GWC_MAX_SLOTS); return ZKHIP_EINVAL; }
  if (!plan->set_rotation || !plan->query_set || !plan->query_pos || !plan->query_slot) { set_error("%s: null plan array", who); return ZKHIP_EINVAL; }
  if (k > 28) { set_error("%s: k = %u > 28", who, k); return ZKHIP_EINVAL; }
  if (!omega || !fr_words_canonical(omega)) { set_error("%s: omega is null or not a canonical Fr", who); return ZKHIP_EINVAL; }
  for (uint32_t i = 0; i < plan->n_sets; i++)
    if (plan->set_rotation[i] >= ((uint64_t)1 << k)) { set_error("%s: set %u: rotation %u is not reduced mod 2^%u", who, i, plan->set_rotation[i], k); return ZKHIP_EINVAL; }
  for (uint32_t q = 0; q < plan->n_evals; q++)
    if (plan->query_set[q] >= plan->n_sets || plan->query_pos[q] >= plan->n_evals || plan->query_slot[q] >= plan->n_slots) {
      set_error("%s: query %u: set %u of %u, position %u of %u, slot %u of %u", who, q, plan->query_set[q], plan->n_sets, plan->query_pos[q], plan->n_evals,
                plan->query_slot[q], plan->n_slots);
      return ZKHIP_EINVAL;
    }
  return ZKHIP_OK;
}

// the plan as the kernel reads it, in 32-bit words: omega^rot per set (8 words each) | a word per query | slot_start [n_slots + 1] | slot_query [n_evals]
static size_t gwc_plan_words(const zkhip_gwc_plan* plan) { return (size_t)plan->n_sets * 8 + plan->n_evals + plan->n_slots + 1 + plan->n_evals; }

size_t gwc_scalars_workspace_bytes(const zkhip_gwc_plan* plan) { return gwc_plan_words(plan) * 4; }

int gwc_scalars_device(const zkhip_gwc_plan* plan, const uint32_t* d_evals, const uint32_t* d_points, uint32_t k, const uint64_t* omega, uint64_t n_proofs,
                       uint32_t* d_rows_a, uint32_t* d_rows_c, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring) {
  const uint32_t n_sets = plan->n_sets, n_evals = plan->n_evals, n_slots = plan->n_slots;
  if (ws_bytes < gwc_plan_words(plan) * 4) { set_error("gwc_scalars: workspace too small"); return ZKHIP_EINVAL; }
  std::vector<uint32_t> blob(gwc_plan_words(plan));
  uint32_t* set_omega = blob.data();
  uint32_t* query_word = set_omega + (size_t)n_sets * 8;
  uint32_t* slot_start = query_word + n_evals;
  uint32_t* slot_query = slot_start + n_slots + 1;
  uint32_t ow[8];
  std::memcpy(ow, omega, 32);
  const fe w = gf_reduce<Fr>(fe_from_ext_lazy(ow));
  for (uint32_t i = 0; i < n_sets; i++) {
    uint32_t out[8];
    fe_to_ext<Fr>(ip_pow<Fr>(w, plan->set_rotation[i]), out);
    std::memcpy(set_omega + (size_t)i * 8, out, 32);
  }
  for (uint32_t s = 0; s <= n_slots; s++) slot_start[s] = 0;
  for (uint32_t q = 0; q < n_evals; q++) {
    query_word[q] = gf_query_word(plan->query_set[q], plan->query_pos[q]);
    slot_start[plan->query_slot[q] + 1]++;
  }
  for (uint32_t s = 0; s < n_slots; s++) slot_start[s + 1] += slot_start[s];
  std::vector<uint32_t> fill(slot_start, slot_start + n_slots);
  for (uint32_t q = 0; q < n_evals; q++) slot_query[fill[plan->query_slot[q]]++] = q;      // a slot's queries in query order
  // through the argument ring, a slot's worth at a time: no wait for the stream (a plan above the ring's eight slots waits for its own first copies)
  for (size_t at = 0; at < blob.size() * 4; at += arg_ring::SLOT_BYTES) {
    const size_t bytes = blob.size() * 4 - at < arg_ring::SLOT_BYTES ? blob.size() * 4 - at : arg_ring::SLOT_BYTES;
    const int rc = upload_args(ring, (char*)ws + at, (const char*)blob.data() + at, bytes, stream);
    if (rc != ZKHIP_OK) return rc;
  }
  const uint32_t* d = (const uint32_t*)ws;
  const uint32_t widest = n_evals > n_sets + n_slots ? n_evals : n_sets + n_slots;
  const uint32_t threads = widest <= GWC_THREADS_SHORT ? GWC_THREADS_SHORT : GWC_THREADS;
  hipLaunchKernelGGL(k_gwc_scalars, dim3((unsigned)n_proofs), dim3(threads), 0, stream, d_evals, d_points, d, n_evals, n_sets, n_slots, d_rows_a, d_rows_c);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

size_t fold_rows_workspace_bytes(uint32_t n_cols, uint32_t n_own, uint64_t n_rows) {
  const uint64_t spans = (n_rows + FOLD_SPAN - 1) / FOLD_SPAN;
  return spans > 1 ? (size_t)spans * (n_cols - n_own) * 32 : 0;
}

int fold_rows_device(const uint32_t* d_rows, uint32_t n_cols, uint32_t n_own, const uint32_t* d_r, uint32_t negate, uint64_t n_rows, uint32_t* d_out_own,
                     uint32_t* d_out_shared, void* ws, size_t ws_bytes, hipStream_t stream) {
  const uint32_t n_shared = n_cols - n_own;
  if (n_rows == 0) {
    if (n_shared) HIPCHK(hipMemsetAsync(d_out_shared, 0, (size_t)n_shared * 32, stream));
    return ZKHIP_OK;
  }
  if (n_own) {
    const uint64_t elems = n_rows * n_own;
    hipLaunchKernelGGL(k_fold_own, dim3((unsigned)((elems + FOLD_THREADS - 1) / FOLD_THREADS)), dim3(FOLD_THREADS), 0, stream, d_rows, n_cols, n_own, d_r, n_rows,
                       negate, d_out_own);
    HIPCHK(hipGetLastError());
  }
  if (n_shared) {
    const uint32_t spans = (uint32_t)((n_rows + FOLD_SPAN - 1) / FOLD_SPAN);
    if (ws_bytes < fold_rows_workspace_bytes(n_cols, n_own, n_rows)) { set_error("fr_fold_rows: workspace too small"); return ZKHIP_EINVAL; }
    hipLaunchKernelGGL(k_fold_shared, dim3(n_shared, spans), dim3(FOLD_THREADS), 0, stream, d_rows, n_cols, n_own, d_r, n_rows, negate, d_out_shared, (uint32_t*)ws);
    HIPCHK(hipGetLastError());
    if (spans > 1) {
      hipLaunchKernelGGL(k_fold_finish, dim3(n_shared), dim3(FOLD_THREADS), 0, stream, (const uint32_t*)ws, spans, negate, d_out_shared);
      HIPCHK(hipGetLastError());
    }
  }
  return ZKHIP_OK;
}

}  // namespace zkhip

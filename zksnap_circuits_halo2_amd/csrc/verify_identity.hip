// The quotient identity at x for a batch of proofs (include/zkhip.h, "the quotient identity at x"): the step of [DEP] halo2-axiom
// plonk/verifier.rs `verify_proof` that recomputes the expected quotient evaluation from the gate, permutation and lookup expressions at x and
// compares it with h(x) (x^n - 1) -- the reference's aggregator runs it once per ballot proof (/root/reference/aggregator/src/wrapper.rs:140-155).
// The identity is a row program (evaluation.py identity_program); a proof is a ROW of it, so a batch is what rowvm.hip's interpreter already
// runs.  What this file adds is the layout around that launch:
//
//   k_identity_columns   [proof][evaluation] records -> [column][proof], a 16 x 16 tile of 32-byte elements through LDS: both the global reads
//                        (512 contiguous bytes of one proof per 32 lanes) and the global writes (512 contiguous bytes of one column) are
//                        whole cache lines.  LDS rows are padded to 34 slots of 16 bytes: a column read then puts the 16 lanes of every
//                        ds_read_b128 lane group on 16 different slots of the 256-byte bank row (slot = lane + 2 column mod 16).
//                        One extra grid row (blockIdx.y = the number of evaluation tiles) writes, one lane per proof, the five challenge
//                        columns and the four derived ones (identity_points.hpp) and the proof's in-domain flag.
//   k_identity_verdict   result column + flags -> status per proof and the report (check_report.hpp).
//   k_domain_points      identity_points.hpp for an array of points, one lane per point (zkhip_fr_domain_points_device).
//
// A lane of the derived row runs k squarings, ~3 (n - u) products and one inversion (~11 k instructions): blocks of that row use their first
// 16 lanes, so a batch spreads over the SIMDs as thinly as it goes.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "check_report.hpp"
#include "fr_vec.hpp"
#include "identity_points.hpp"
#include "instance_evals.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

constexpr uint32_t ID_TILE = 16;                         // proofs x evaluations per block
constexpr uint32_t ID_ROW_SLOTS = 2 * ID_TILE + 2;       // 16-byte slots per LDS row (two per element, two of padding)
constexpr uint32_t ID_THREADS = 256;
constexpr uint32_t ID_DERIVED = 9;                       // theta, beta, gamma, y, x, x^n, l_0, l_last, l_active

struct identity_domain {                                 // by value: the domain's constants in external words
  fe_arg omega, n_inv;
  uint32_t k, u;
};

__device__ __forceinline__ void id_store_ext(uint32_t* p, const fe& v) {
  uint32_t w[8];
  fe_to_ext<Fr>(v, w);
  store_words(p, w);
}

__device__ __forceinline__ identity_points id_points(const identity_domain& dom, const uint32_t (&xw)[8]) {
  uint32_t ow[8], nw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) { ow[i] = dom.omega.w[i]; nw[i] = dom.n_inv.w[i]; }
  return identity_points_at<Fr>(fe_from_ext_lazy(xw), dom.k, dom.u, fe_from_ext_lazy(ow), fe_from_ext_lazy(nw));
}

__global__ void __launch_bounds__(ID_THREADS) k_identity_columns(const uint4* __restrict__ evals, uint32_t n_evals, const uint32_t* __restrict__ challenges,
                                                                 uint64_t n_proofs, const identity_domain dom, uint4* __restrict__ cols,
                                                                 uint32_t* __restrict__ in_domain, uint32_t eval_tiles) {
  __shared__ uint4 tile[ID_TILE * ID_ROW_SLOTS];
  const uint64_t p0 = (uint64_t)blockIdx.x * ID_TILE;
  if (blockIdx.y == eval_tiles) {                        // the derived row: one lane per proof
    const uint64_t p = p0 + threadIdx.x;
    if (threadIdx.x >= ID_TILE || p >= n_proofs) return;
    uint32_t* out = (uint32_t*)cols;
    uint32_t xw[8];
#pragma unroll 1
    for (uint32_t c = 0; c < 5; c++) {
      load_words(challenges + (p * 5 + c) * 8, xw);      // (the last one read is x)
      store_words(out + ((uint64_t)(n_evals + c) * n_proofs + p) * 8, xw);
    }
    const identity_points v = id_points(dom, xw);
    id_store_ext(out + ((uint64_t)(n_evals + 5) * n_proofs + p) * 8, v.xn);
    id_store_ext(out + ((uint64_t)(n_evals + 6) * n_proofs + p) * 8, v.l0);
    id_store_ext(out + ((uint64_t)(n_evals + 7) * n_proofs + p) * 8, v.l_last);
    id_store_ext(out + ((uint64_t)(n_evals + 8) * n_proofs + p) * 8, v.l_active);
    in_domain[p] = v.in_domain ? 1u : 0u;
    return;
  }
  const uint32_t e0 = blockIdx.y * ID_TILE;
#pragma unroll
  for (uint32_t r = 0; r < 2; r++) {                     // in: lane -> (proof, 16-byte piece of the proof's 16 evaluations)
    const uint32_t idx = threadIdx.x + r * ID_THREADS, row = idx / (2 * ID_TILE), piece = idx % (2 * ID_TILE);
    const uint64_t p = p0 + row;
    const uint32_t e = e0 + piece / 2;
    if (p < n_proofs && e < n_evals) tile[row * ID_ROW_SLOTS + piece] = evals[(p * n_evals + e) * 2 + (piece & 1u)];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < 2; r++) {                     // out: lane -> (evaluation, 16-byte piece of the column's 16 proofs)
    const uint32_t idx = threadIdx.x + r * ID_THREADS, col = idx / (2 * ID_TILE), piece = idx % (2 * ID_TILE);
    const uint64_t p = p0 + piece / 2;
    const uint32_t e = e0 + col;
    if (p < n_proofs && e < n_evals) cols[((uint64_t)e * n_proofs + p) * 2 + (piece & 1u)] = tile[(piece / 2) * ID_ROW_SLOTS + col * 2 + (piece & 1u)];
  }
}

__global__ void __launch_bounds__(256) k_identity_verdict(const uint4* __restrict__ result, const uint32_t* __restrict__ in_domain, uint64_t n_proofs,
                                                          int32_t* __restrict__ status, unsigned long long* __restrict__ report) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t verdict = 0;
  if (p < n_proofs) {
    const uint4 a = result[p * 2], b = result[p * 2 + 1];
    const bool nonzero = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) != 0u;
    verdict = in_domain[p] ? 2 : (nonzero ? 1 : 0);
    status[p] = verdict;
  }
  check_report_wave(verdict != 0, p, report);
}

__global__ void __launch_bounds__(64) k_domain_points(const uint32_t* __restrict__ x, uint64_t n_points, const identity_domain dom, uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_points) return;
  uint32_t xw[8];
  load_words(x + i * 8, xw);
  const identity_points v = id_points(dom, xw);
  id_store_ext(out + (0 * n_points + i) * 8, v.xn);
  id_store_ext(out + (1 * n_points + i) * 8, v.l0);
  id_store_ext(out + (2 * n_points + i) * 8, v.l_last);
  id_store_ext(out + (3 * n_points + i) * 8, v.l_active);
}

// ---- instance columns: e[q][p] for every (query, proof) pair (instance_evals.hpp) ----------------------------------------------------------------
// A group of IE_GROUP lanes per pair, pairs in the order of the output ([query][proof]): the lanes of a group read consecutive 32-byte elements of
// one proof's public inputs per step, the first lanes of consecutive groups write consecutive elements of one output column.  A group never
// leaves its 16-lane row, and the joins exchange nine limbs per fraction half with __shfl_xor at distances 1 and 2 (4 and 8 as well in a group of
// 16).  The gfx950 build lowers them to ds_bpermute_b32 -- 36 of the kernel's ~7700 instructions, through the LDS crossbar with no LDS allocated --
// so a hand-written DPP exchange has nothing to win here.  Every lane of a group reaches the joins: a lane with no term carries 0 / 1.
// The group size is a build-time constant, 4 by measurement (profiles/r28_instance_columns.txt: at 4096 proofs of 30 / 70 values 0.093 / 0.116 ms
// a call against 0.159 / 0.281 ms with 1 lane and 0.237 / 0.241 ms with 16; at one proof 0.091 ms against 0.085 .. 0.094 ms with 16, inside the
// spread of two series of the same build, and 0.172 ms with 1).  -DZKHIP_INSTANCE_GROUP=1|4|16 builds the others for that measurement; nothing
// reads it at run time.
#ifndef ZKHIP_INSTANCE_GROUP
#define ZKHIP_INSTANCE_GROUP 4
#endif
constexpr uint32_t IE_GROUP = ZKHIP_INSTANCE_GROUP;
constexpr uint32_t IE_THREADS = 256;
static_assert(IE_GROUP == 1 || IE_GROUP == 4 || IE_GROUP == 16, "a lane group is 1, 4 or 16 lanes: it stays inside one 16-lane row");

struct instance_query_table {                            // by value: per query, where its column lies in a proof's inputs and how it is rotated
  uint32_t offset[INSTANCE_MAX_QUERIES], len[INSTANCE_MAX_QUERIES], rot[INSTANCE_MAX_QUERIES];
};

struct instance_domain {
  fe_arg omega, omega_g, n_inv;                          // omega_g = omega^IE_GROUP
  uint32_t k;
};

__device__ __forceinline__ fe ie_shfl_xor(const fe& a, int mask) {
  fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = (uint32_t)__shfl_xor((int)a.l[i], mask, 64);
  return r;
}

__device__ __forceinline__ fe ie_arg(const fe_arg& c) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = c.w[i];
  return fe_from_ext_lazy(w);
}

// x of proof p: x[p * x_stride] words (a plain array of points, or the fifth challenge of every record)
__global__ void __launch_bounds__(IE_THREADS) k_instance_evals(const uint32_t* __restrict__ x, uint32_t x_stride, const uint32_t* __restrict__ instances,
                                                               uint64_t total_len, const instance_query_table qt, uint32_t n_queries, uint64_t n_proofs,
                                                               const instance_domain dom, uint32_t* __restrict__ out) {
  const uint64_t pair = ((uint64_t)blockIdx.x * IE_THREADS + threadIdx.x) / IE_GROUP;
  const uint32_t g = threadIdx.x % IE_GROUP;
  if (pair >= (uint64_t)n_queries * n_proofs) return;    // a whole group at a time: the lanes of a join are all here
  const uint32_t q = (uint32_t)(pair / n_proofs);
  const uint64_t p = pair % n_proofs;
  uint32_t xw[8];
  load_words(x + p * x_stride, xw);
  const fe xv = fe_from_ext_lazy(xw);
  const uint32_t* column = instances + (p * total_len + qt.offset[q]) * 8;
  ie_fraction f = ie_lane<Fr>(xv, dom.k, ie_arg(dom.omega), ie_arg(dom.omega_g), qt.rot[q], qt.len[q], g, IE_GROUP, [&](uint32_t i) {
    uint32_t vw[8];
    load_words(column + (uint64_t)i * 8, vw);
    return fe_from_ext_lazy(vw);
  });
#pragma unroll
  for (uint32_t d = 1; d < IE_GROUP; d <<= 1) {
    ie_fraction other;
    other.num = ie_shfl_xor(f.num, (int)d);
    other.den = ie_shfl_xor(f.den, (int)d);
    f = ie_join<Fr>(f, other);
  }
  if (g == 0) id_store_ext(out + pair * 8, ie_finish<Fr>(f, xv, dom.k, ie_arg(dom.n_inv)));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
int identity_domain_validate(const char* who, uint32_t k, uint64_t usable_rows, const uint64_t* omega) {
  if (!omega) { set_error("%s: null omega", who); return ZKHIP_EINVAL; }
  if (k > 28) { set_error("%s: k = %u > 28", who, k); return ZKHIP_EINVAL; }
  const uint64_t n = (uint64_t)1 << k;
  if (usable_rows < 1 || usable_rows >= n || n - usable_rows > IDENTITY_MAX_TAIL) {
    set_error("%s: usable_rows = %llu: needs 1 <= usable_rows < 2^%u and 2^%u - usable_rows <= %u", who, (unsigned long long)usable_rows, k, k, IDENTITY_MAX_TAIL);
    return ZKHIP_EINVAL;
  }
  if (!fr_words_canonical(omega)) { set_error("%s: omega is not a canonical Fr", who); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}

// the constants a launch takes by value; 1 / n = (2^k)^-1 on the host: k doublings of one and the inversion of fe_inverse.hpp
static identity_domain id_make_domain(uint32_t k, uint32_t u, const uint64_t* omega) {
  identity_domain d;
  std::memcpy(d.omega.w, omega, 32);
  fe n = fe_one<Fr>();
  for (uint32_t i = 0; i < k; i++) n = fe_canon_lt2p<Fr>(fe_norm(fe_dbl(n)));
  fe_to_ext<Fr>(fe_inverse<Fr>(n), d.n_inv.w);
  d.k = k;
  d.u = u;
  return d;
}

int fr_domain_points_device(uint32_t k, uint32_t usable_rows, const uint64_t* omega, const uint32_t* d_x, uint64_t n_points, uint32_t* d_out, hipStream_t stream) {
  const identity_domain dom = id_make_domain(k, usable_rows, omega);
  hipLaunchKernelGGL(k_domain_points, dim3((unsigned)((n_points + 63) / 64)), dim3(64), 0, stream, d_x, n_points, dom, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int verify_identity_validate(const zkhip_vm_program* p, uint32_t n_evals, uint32_t n_queries) {
  if (!p) { set_error("verify_identity: null program"); return ZKHIP_EINVAL; }
  if ((uint64_t)n_evals + ID_DERIVED + n_queries > 65536) {
    set_error("verify_identity: %u evaluations + %u derived and instance columns exceed 65536", n_evals, ID_DERIVED + n_queries);
    return ZKHIP_EINVAL;
  }
  const int rc = row_vm_validate(p, n_evals + ID_DERIVED + n_queries, 0, 0);      // every column below n_evals + 9 + n_queries, every index inside its table
  if (rc != ZKHIP_OK) return rc;
  // the rotation TABLE, named by an instruction or not: the window launch sizes its halos by every entry
  for (uint32_t i = 0; i < p->n_rotations; i++)
    if (p->rotations[i] != 0) { set_error("verify_identity: rotation %d: a rotated opening is a column of its own", p->rotations[i]); return ZKHIP_EINVAL; }
  for (uint32_t pc = 0; pc < p->n_insns; pc++) {
    const zkhip_vm_insn& in = p->insns[pc];
    const int n_opnd = (in.op == ZKHIP_OP_MAD) ? 3 : ((in.op == ZKHIP_OP_ADD || in.op == ZKHIP_OP_SUB || in.op == ZKHIP_OP_MUL) ? 2 : 1);
    const zkhip_vm_operand* o[3] = {&in.a, &in.b, &in.c};
    for (int i = 0; i < n_opnd; i++)
      if (o[i]->kind == ZKHIP_SRC_PREV || o[i]->kind == ZKHIP_SRC_ROWPOW) {
        set_error("verify_identity: instruction %u reads %s: a proof is a row of its own", pc, o[i]->kind == ZKHIP_SRC_PREV ? "ZKHIP_SRC_PREV" : "ZKHIP_SRC_ROWPOW");
        return ZKHIP_EINVAL;
      }
  }
  return ZKHIP_OK;
}

size_t verify_identity_columns_bytes(uint32_t n_evals, uint32_t n_queries, uint64_t n_proofs) {
  return ((size_t)n_evals + ID_DERIVED + n_queries + 1) * n_proofs * 32 + n_proofs * 4;      // the columns, the result column, the flags
}

size_t verify_identity_vm_bytes(const zkhip_vm_program* p, uint32_t n_evals, uint32_t n_queries) {
  return row_vm_workspace_bytes(p, 1, n_evals + ID_DERIVED + n_queries, 0);
}

int instance_queries_validate(const char* who, uint32_t k, uint64_t max_len, const char* max_name, const uint32_t* column_lens, uint32_t n_columns,
                              const uint32_t* query_columns, const uint32_t* query_rotations, uint32_t n_queries, instance_layout* out) {
  if (n_columns > INSTANCE_MAX_QUERIES || n_queries > INSTANCE_MAX_QUERIES) {
    set_error("%s: %u instance columns, %u queries: at most %u of each", who, n_columns, n_queries, INSTANCE_MAX_QUERIES);
    return ZKHIP_EINVAL;
  }
  if ((n_columns && !column_lens) || (n_queries && (!query_columns || !query_rotations))) { set_error("%s: null instance column or query array", who); return ZKHIP_EINVAL; }
  if (k > 28) { set_error("%s: k = %u > 28", who, k); return ZKHIP_EINVAL; }
  uint64_t offsets[INSTANCE_MAX_QUERIES], total = 0;
  for (uint32_t c = 0; c < n_columns; c++) {
    if (column_lens[c] > max_len) { set_error("%s: instance column %u holds %u values, more than %s = %llu", who, c, column_lens[c], max_name, (unsigned long long)max_len); return ZKHIP_EINVAL; }
    offsets[c] = total;
    total += column_lens[c];
  }
  out->total_len = total;
  out->n_queries = n_queries;
  for (uint32_t q = 0; q < n_queries; q++) {
    if (query_columns[q] >= n_columns) { set_error("%s: query %u names instance column %u of %u", who, q, query_columns[q], n_columns); return ZKHIP_EINVAL; }
    if (query_rotations[q] >= ((uint64_t)1 << k)) { set_error("%s: query %u: rotation %u is not reduced mod 2^%u", who, q, query_rotations[q], k); return ZKHIP_EINVAL; }
    out->offset[q] = (uint32_t)offsets[query_columns[q]];      // (64 columns of at most 2^28 values: below 2^34 ... checked next)
    out->len[q] = column_lens[query_columns[q]];
    out->rot[q] = query_rotations[q];
  }
  if (total > 0xffffffffull) { set_error("%s: %llu public inputs per proof", who, (unsigned long long)total); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}

static instance_domain ie_make_domain(uint32_t k, const uint64_t* omega) {
  const identity_domain base = id_make_domain(k, 0, omega);
  instance_domain d;
  d.omega = base.omega;
  d.n_inv = base.n_inv;
  d.k = k;
  uint32_t w[8];
  std::memcpy(w, omega, 32);
  fe_to_ext<Fr>(ip_pow<Fr>(fe_mul<Fr>(fe_one<Fr>(), fe_from_ext_lazy(w)), IE_GROUP), d.omega_g.w);
  return d;
}

static int instance_evals_launch(const instance_domain& dom, const uint32_t* d_x, uint32_t x_stride, const uint32_t* d_instances, const instance_layout& lay,
                                 uint64_t n_proofs, uint32_t* d_out, hipStream_t stream) {
  instance_query_table qt;
  std::memset(&qt, 0, sizeof qt);
  for (uint32_t q = 0; q < lay.n_queries; q++) { qt.offset[q] = lay.offset[q]; qt.len[q] = lay.len[q]; qt.rot[q] = lay.rot[q]; }
  const uint64_t lanes = (uint64_t)lay.n_queries * n_proofs * IE_GROUP;
  hipLaunchKernelGGL(k_instance_evals, dim3((unsigned)((lanes + IE_THREADS - 1) / IE_THREADS)), dim3(IE_THREADS), 0, stream, d_x, x_stride, d_instances,
                     lay.total_len, qt, lay.n_queries, n_proofs, dom, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int fr_instance_evals_device(uint32_t k, const uint64_t* omega, const uint32_t* d_x, const uint32_t* d_instances, const instance_layout& lay, uint64_t n_proofs,
                             uint32_t* d_out, hipStream_t stream) {
  if (lay.n_queries == 0 || n_proofs == 0) return ZKHIP_OK;
  return instance_evals_launch(ie_make_domain(k, omega), d_x, 8, d_instances, lay, n_proofs, d_out, stream);
}

int verify_identity_device(const zkhip_vm_program* prog, const uint32_t* d_evals, uint32_t n_evals, const uint32_t* d_challenges, uint32_t k, uint32_t usable_rows,
                           const uint64_t* omega, const uint32_t* d_instances, const instance_layout& lay, uint64_t n_proofs, int32_t* d_status, void* d_report,
                           void* cols_ws, void* vm_ws, size_t vm_ws_bytes, hipStream_t stream, vm_staging* staging) {
  int rc = check_reports_init_device(d_report, 1, stream);
  if (rc != ZKHIP_OK || n_proofs == 0) return rc;
  const uint32_t n_columns = n_evals + ID_DERIVED + lay.n_queries;
  uint32_t* cols = (uint32_t*)cols_ws;
  uint32_t* result = cols + (size_t)n_columns * n_proofs * 8;
  uint32_t* flags = result + n_proofs * 8;
  const identity_domain dom = id_make_domain(k, usable_rows, omega);
  const uint32_t eval_tiles = (n_evals + ID_TILE - 1) / ID_TILE;
  hipLaunchKernelGGL(k_identity_columns, dim3((unsigned)((n_proofs + ID_TILE - 1) / ID_TILE), eval_tiles + 1), dim3(ID_THREADS), 0, stream, (const uint4*)d_evals,
                     n_evals, d_challenges, n_proofs, dom, (uint4*)cols, flags, eval_tiles);
  HIPCHK(hipGetLastError());
  // the instance columns behind the derived ones, x read from the records (the fifth challenge)
  if (lay.n_queries && (rc = instance_evals_launch(ie_make_domain(k, omega), d_challenges + 4 * 8, 5 * 8, d_instances, lay, n_proofs,
                                                   cols + (size_t)(n_evals + ID_DERIVED) * n_proofs * 8, stream)) != ZKHIP_OK) return rc;
  std::vector<const void*> columns(n_columns);
  for (uint32_t c = 0; c < n_columns; c++) columns[c] = cols + (size_t)c * n_proofs * 8;
  // a proof is a row of its own: a window launch over a domain of ONE row, so that column i is simply n_proofs elements and nothing wraps (the
  // program names no rotation but 0 and neither PREV nor ROWPOW: verify_identity_validate).  The interpreter, whatever the shape.
  vm_call c;
  c.progs = prog; c.d_columns = columns.data(); c.n_columns = n_columns; c.log_rows = 0;
  c.form = VM_WINDOW; c.count = n_proofs; c.d_out = result; c.interpreter_only = true;
  c.ws = vm_ws; c.ws_bytes = vm_ws_bytes; c.stream = stream; c.staging = staging;
  if ((rc = row_vm_launch(c)) != ZKHIP_OK) return rc;
  hipLaunchKernelGGL(k_identity_verdict, dim3((unsigned)((n_proofs + 255) / 256)), dim3(256), 0, stream, (const uint4*)result, flags, n_proofs, d_status,
                     (unsigned long long*)d_report);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

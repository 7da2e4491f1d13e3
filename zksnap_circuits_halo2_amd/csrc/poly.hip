// Fr-vector primitives of the prover besides the NTT: `eval_polynomial`, `kate_division`
// ([DEP] halo2-axiom halo2_proofs/src/arithmetic.rs), `BatchInvert::batch_invert` ([DEP] ff crate, used by the
// permutation / lookup grand products) and the grand-product running product itself ([DEP] plonk/permutation/prover.rs:
// z[i+1] = z[i] * v[i]); all reached from create_proof, /root/reference/aggregator/src/wrapper.rs:129.
//
// All four are chunked linear recurrences: a thread owns CH consecutive elements, a first pass produces one aggregate
// per chunk, the aggregates are scanned the same way (1/CH of the work), a second pass re-runs each chunk with its
// incoming carry.  2 multiplies per element, O(log_CH n) launches; the levels of every scan come from scan_plan.hpp.
//   suffix Horner scan  out[i] = a[i] + b * out[i+1]           (kate_division; eval_polynomial is out[0])
//   prefix product      out[0] = 1, out[i+1] = out[i] * v[i]
//   batch inversion     Montgomery's trick per chunk with one inversion (division steps, fe_inverse.hpp) per thread
// Values are kept in the external Montgomery-256 domain throughout: x*2^256 is the radix-2^261 form of x*2^-5 and the
// recurrences are linear in the data, so only the constant multiplier is converted (fp29.hpp).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include "fp29.hpp"
#include "fe_inverse.hpp"
#include "fr_vec.hpp"
#include "scan_plan.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

// elements per thread of the scans: SCAN_CH (scan_plan.hpp).  16, not 32 (round 3, same-box A/B in profiles/r03_batch_invert_ab.txt): 2^15 eval / kate /
// prefix 0.099 / 0.170 / 0.111 -> 0.086 / 0.139 / 0.078 ms, 2^20 0.130 / 0.231 / 0.160 -> 0.117 / 0.196 / 0.120, 2^24 0.367 / 0.980 / 0.854 -> 0.361 / 0.942 /
// 0.805 (8: the large sizes lose).  The batch inversion picks its own chunk length (INV_CH_MAX).
constexpr uint32_t INV_CH_MAX = 32;

// ---- suffix Horner scan ---------------------------------------------------------------------------
// pass A: agg[t] = sum_{i in chunk t} a[i] b^(i - lo)          (the chunk's scan value at its first element, carry-in 0).  One dense array:
// k_horner_agg_batch with one lane computes the same, 3 % slower per launch (profiles/r18_scan_plan.txt), so the single-array form stays
__global__ void __launch_bounds__(256) k_horner_agg(const uint32_t* __restrict__ a, size_t n, const fe_arg* __restrict__ b_dev, uint32_t* __restrict__ agg) {
  const fe_arg b_ext = *b_dev;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  const fe b = fr_const_internal(b_ext);
  fe q = fe_zero();
  size_t i = hi;
  // full blocks of four elements = one 128-byte line per lane: the eight loads of a block are issued together and the line is consumed at
  // once (element by element the same line was touched in four separate iterations, 64 lanes x 64 lines apart, and had to survive in L1)
  for (; i >= lo + 4 && ((i & 3) == 0); i -= 4) {
    uint32_t w0[8], w1[8], w2[8], w3[8];
    load_words(a + (i - 1) * 8, w3); load_words(a + (i - 2) * 8, w2); load_words(a + (i - 3) * 8, w1); load_words(a + (i - 4) * 8, w0);
    q = fe_norm(fe_add(fe_unpack<0>(w3), fe_mul<Fr>(b, q)));
    q = fe_norm(fe_add(fe_unpack<0>(w2), fe_mul<Fr>(b, q)));
    q = fe_norm(fe_add(fe_unpack<0>(w1), fe_mul<Fr>(b, q)));
    q = fe_norm(fe_add(fe_unpack<0>(w0), fe_mul<Fr>(b, q)));
  }
  for (; i-- > lo;) q = fe_norm(fe_add(load_ext(a, i), fe_mul<Fr>(b, q)));   // < 3p, N
  store_canon(agg, t, q);
}

// pass B: out[i] = a[i] + b * out[i+1] with carry-in carry[t+1] (the full scan value at the next chunk's first element)
__global__ void __launch_bounds__(256) k_horner_apply(const uint32_t* __restrict__ a, size_t n, const fe_arg* __restrict__ b_dev,
                                                      const uint32_t* __restrict__ carry, size_t ncarry, uint32_t* __restrict__ out,
                                                      size_t out_shift) {
  const fe_arg b_ext = *b_dev;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  const fe b = fr_const_internal(b_ext);
  fe q = (carry != nullptr && t + 1 < ncarry) ? load_ext(carry, t + 1) : fe_zero();
  size_t i = hi;
  for (; i >= lo + 4 && ((i & 3) == 0); i -= 4) {               // four elements = one 128-byte line per lane, loaded together (see k_horner_agg)
    uint32_t w[4][8];
#pragma unroll
    for (int e = 0; e < 4; e++) load_words(a + (i - 4 + e) * 8, w[e]);
#pragma unroll
    for (int e = 3; e >= 0; e--) {
      q = fe_norm(fe_add(fe_unpack<0>(w[e]), fe_mul<Fr>(b, q)));
      if (i - 4 + e >= out_shift) store_canon(out, i - 4 + e - out_shift, q);     // kate_division drops the scan value at index 0
    }
  }
  for (; i-- > lo;) {
    q = fe_norm(fe_add(load_ext(a, i), fe_mul<Fr>(b, q)));
    if (i >= out_shift) store_canon(out, i - out_shift, q);
  }
}

// batched form of pass A for many polynomials of one length evaluated at one point (multiopen: every advice / fixed / permutation
// polynomial at x): blockIdx.y = polynomial; level 0 reads through a pointer table, deeper levels a dense [count][n] array.
// The last level (n <= CH) is the evaluation itself.
__global__ void __launch_bounds__(256) k_horner_agg_batch(const uint32_t* const* __restrict__ ptrs, const uint32_t* __restrict__ base, size_t n,
                                                          const fe_arg* __restrict__ b_dev, uint32_t* __restrict__ agg, size_t m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  const uint32_t* a = ptrs ? ptrs[blockIdx.y] : base + (size_t)blockIdx.y * n * 8;
  const fe_arg b_ext = *b_dev;
  const fe b = fr_const_internal(b_ext);
  fe q = fe_zero();
  size_t i = hi;
  for (; i >= lo + 4 && ((i & 3) == 0); i -= 4) {               // four elements = one 128-byte line per lane, loaded together (see k_horner_agg)
    uint32_t w[4][8];
#pragma unroll
    for (int e = 0; e < 4; e++) load_words(a + (i - 4 + e) * 8, w[e]);
#pragma unroll
    for (int e = 3; e >= 0; e--) q = fe_norm(fe_add(fe_unpack<0>(w[e]), fe_mul<Fr>(b, q)));
  }
  for (; i-- > lo;) q = fe_norm(fe_add(load_ext(a, i), fe_mul<Fr>(b, q)));
  store_canon(agg + (size_t)blockIdx.y * m * 8, t, q);
}

// ---- prefix product --------------------------------------------------------------------------------
__device__ __forceinline__ void prod_agg_chunk(const uint32_t* __restrict__ v, size_t n, uint32_t* __restrict__ agg, size_t t) {
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  uint32_t w[8];
  load_words(v + lo * 8, w);
  fe acc = fe_unpack<0>(w);                                   // x * 2^256 (external domain)
  size_t i = lo + 1;
  for (; i < hi && (i & 3) != 0; i++) {                       // up to the next 128-byte line
    load_words(v + i * 8, w);
    acc = fe_mul<Fr>(acc, fe_from_ext_lazy(w));               // ext-domain value times internal-form factor stays in the ext domain
  }
  for (; i + 4 <= hi; i += 4) {                               // four elements = one line per lane, loaded together (see k_horner_agg)
    uint32_t ww[4][8];
#pragma unroll
    for (int e = 0; e < 4; e++) load_words(v + (i + e) * 8, ww[e]);
#pragma unroll
    for (int e = 0; e < 4; e++) acc = fe_mul<Fr>(acc, fe_from_ext_lazy(ww[e]));
  }
  for (; i < hi; i++) {
    load_words(v + i * 8, w);
    acc = fe_mul<Fr>(acc, fe_from_ext_lazy(w));
  }
  store_canon(agg, t, acc);
}

// blockIdx.y = one of many independent arrays of n elements, dense; m = chunks of one array
__global__ void __launch_bounds__(256) k_prod_agg_batch(const uint32_t* __restrict__ v, size_t n, uint32_t* __restrict__ agg, size_t m) {
  prod_agg_chunk(v + (size_t)blockIdx.y * n * 8, n, agg + (size_t)blockIdx.y * m * 8, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// out[i] = carry[t] * prod_{lo <= j < i} v[j]   (exclusive); carry == nullptr: carry is 1
__device__ __forceinline__ void prod_apply_chunk(const uint32_t* __restrict__ v, size_t n, const uint32_t* __restrict__ carry, uint32_t* __restrict__ out,
                                                 size_t t) {
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  fe cur;
  if (carry) cur = load_ext(carry, t);
  else {                                                      // 1 in the external domain = 2^256 mod r
#pragma unroll
    for (int i = 0; i < NL; i++) cur.l[i] = Fr::TO_EXT[i];
  }
  uint32_t w[8];
  size_t i = lo;
  for (; i + 4 <= hi && (i & 3) == 0; i += 4) {               // four elements = one line per lane, loaded together (see k_horner_agg); all four
    uint32_t ww[4][8];                                        // are read before any of them is stored: v and out may alias
#pragma unroll
    for (int e = 0; e < 4; e++) load_words(v + (i + e) * 8, ww[e]);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      store_canon(out, i + e, cur);
      cur = fe_mul<Fr>(cur, fe_from_ext_lazy(ww[e]));
    }
  }
  for (; i < hi; i++) {
    load_words(v + i * 8, w);                                 // read before the store: v and out may alias
    const fe f = fe_from_ext_lazy(w);
    store_canon(out, i, cur);
    cur = fe_mul<Fr>(cur, f);
  }
}

__global__ void __launch_bounds__(256) k_prod_apply_batch(const uint32_t* __restrict__ v, size_t n, const uint32_t* __restrict__ carry, size_t m,
                                                          uint32_t* __restrict__ out) {
  prod_apply_chunk(v + (size_t)blockIdx.y * n * 8, n, carry ? carry + (size_t)blockIdx.y * m * 8 : nullptr, out + (size_t)blockIdx.y * n * 8,
                   (size_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// ---- batch inversion (zeros stay zero, like ff::BatchInvert) ------------------------------------------
// a^-1 in Fr, a internal & reduced: division steps instead of the Fermat chain a^(r-2) (fe_inverse.hpp)
__device__ __forceinline__ fe fr_inverse(const fe& a) { return fe_inverse<Fr>(a); }

// One wavefront per workgroup owns a tile of 64 * ch consecutive elements; lane l inverts the elements l, l + 64, l + 128, ... of the tile
// (Montgomery's trick groups ANY elements: with the lanes interleaved every load and store of the wavefront is one contiguous 2 KiB run,
// where consecutive elements per lane -- the layout of rounds 1-4 -- made each of them 64 separate 32-byte pieces 32 * ch bytes apart).
// The parked prefix products are limb-major (scratch[limb][element]) for the same reason.
__global__ void __launch_bounds__(64) k_batch_invert(uint32_t* __restrict__ a, size_t n, uint32_t* __restrict__ scratch, uint32_t ch) {
  const size_t first = (size_t)blockIdx.x * 64 * ch + threadIdx.x;
  if (first >= n) return;
  // x*2^256 read as the internal form of x' = x*2^-5.  prefix products of the non-zero x' (internal form), parked in scratch
  const fe one = fe_one<Fr>();
  fe pref = one;
  uint32_t w[8];
  uint32_t cnt = 0;
  for (size_t i = first; cnt < ch && i < n; i += 64, cnt++) {
    load_words(a + i * 8, w);
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) o |= w[k];
#pragma unroll
    for (int k = 0; k < NL; k++) scratch[(size_t)k * n + i] = pref.l[k];
    if (o) pref = fe_mul<Fr>(pref, fe_unpack<0>(w));
  }
  // inverse of the product, rescaled once so that the outputs come out in the external domain:
  // x'^-1 (internal) = x^-1 * 2^266; times 2^251 (Montgomery) -> x^-1 * 2^256
  fe c251 = fe_zero();
  c251.l[8] = 1u << (251 - 232);
  fe inv = fe_mul<Fr>(fr_inverse(pref), c251);
  for (uint32_t j = cnt; j-- > 0;) {
    const size_t i = first + (size_t)j * 64;
    load_words(a + i * 8, w);
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) o |= w[k];
    if (!o) continue;
    fe pre;
#pragma unroll
    for (int k = 0; k < NL; k++) pre.l[k] = scratch[(size_t)k * n + i];
    fe out = fe_mul<Fr>(inv, pre);
    inv = fe_mul<Fr>(inv, fe_unpack<0>(w));
    uint32_t wo[8];
    fe_pack(fe_canon_lt2p<Fr>(out), wo);
    store_words(a + i * 8, wo);
  }
}

// ---- host orchestration ------------------------------------------------------------------------------
// Every scan walks one scan_plan (scan_plan.hpp) of its workspace: up, level k - 1 is reduced into level k for k = 1 .. L; down, level k is
// scanned in place from the carries in level k + 1 for k = L .. 1, and level 0 -- the caller's array -- last, into the caller's output.
// plan.n[k + 1] is the number of chunks of level k; one launch per step, `lanes` independent arrays as blockIdx.y.
static inline dim3 grid_for(size_t threads, int block, size_t lanes = 1) { return dim3((unsigned)((threads + block - 1) / block), (unsigned)lanes); }

// a constant that arrives from the host travels as a kernel argument (by value: the caller's memory is free when the launch returns, and
// nothing waits for the stream -- a copy from the caller's memory would need a synchronisation) and is parked in device memory by one thread
// out[0] = v, out[l] = out[l - 1]^CH for l <= levels: the multipliers of every level of a scan
constexpr int POW_LEVELS = 7;             // 16^7 = 2^28 elements; 8 constants = the 256 bytes the scans reserve
__global__ void k_store_const(fe_arg v, fe_arg* __restrict__ out, uint32_t levels) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  out[0] = v;
  if (levels == 0) return;
  fe r = fr_const_internal(v);
  fe k;
#pragma unroll
  for (int i = 0; i < NL; i++) k.l[i] = Fr::TO_EXT[i];
#pragma unroll 1
  for (uint32_t l = 1; l <= levels; l++) {
    static_assert(SCAN_CH == 16, "b^CH below is four squarings");
#pragma unroll
    for (int q = 0; q < 4; q++) r = fe_sqr<Fr>(r);              // b^16 (products of values < 2p stay < 2p)
    uint32_t w[8];
    fe_pack(fe_canon_lt2p<Fr>(fe_mul<Fr>(k, r)), w);
#pragma unroll
    for (int i = 0; i < 8; i++) out[l].w[i] = w[i];
  }
}
// d[k] = host^(CH^k) for every level k of the plan: level k is scanned with the multiplier d[k].  ONE thread computes them up front (a launch
// per level for one power each cost 11 us apiece in the dependent chain)
static int store_const(const uint32_t host[8], fe_arg* d, hipStream_t stream, const scan_plan& plan) {
  fe_arg v;
  memcpy(v.w, host, 32);
  hipLaunchKernelGGL(k_store_const, dim3(1), dim3(64), 0, stream, v, d, (uint32_t)(plan.L < POW_LEVELS ? plan.L : POW_LEVELS));
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}
// the same, parked in the last 256 bytes of the workspace
static int stage_const(const uint32_t host[8], const scan_plan& plan, void* ws, size_t ws_bytes, hipStream_t stream, const fe_arg** out) {
  fe_arg* d = (fe_arg*)((char*)ws + ws_bytes - 256);
  *out = d;
  return store_const(host, d, stream, plan);
}

// the evaluations of `count` polynomials of plan.n[0] coefficients: up through the levels and one step further, where the single aggregate of
// every polynomial is its evaluation.  Level 0 is read through the pointer table d_ptrs; without one it is the single dense array d_a.
static int horner_eval(const uint32_t* const* d_ptrs, const uint32_t* d_a, size_t count, const scan_plan& plan, const fe_arg* b, uint32_t* d_results,
                       void* ws, hipStream_t stream) {
  for (int k = 1; k <= plan.L + 1; k++) {
    const uint32_t* src = k == 1 ? d_a : plan.level<const uint32_t>(ws, k - 1);
    uint32_t* agg = k <= plan.L ? plan.level<uint32_t>(ws, k) : d_results;
    if (d_ptrs) hipLaunchKernelGGL(k_horner_agg_batch, grid_for(plan.n[k], 256, count), dim3(256), 0, stream, k == 1 ? d_ptrs : nullptr, src, plan.n[k - 1], b + (k - 1), agg, plan.n[k]);
    else hipLaunchKernelGGL(k_horner_agg, grid_for(plan.n[k], 256), dim3(256), 0, stream, src, plan.n[k - 1], b + (k - 1), agg);
  }
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// eval_polynomial: result (8 words, device) = sum a[i] x^i
int fr_eval_polynomial_device(const uint32_t* d_a, size_t n, const uint32_t x_host[8], uint32_t* d_result, void* ws, size_t ws_bytes,
                              hipStream_t stream) {
  if (n == 0) { HIPCHK(hipMemsetAsync(d_result, 0, 32, stream)); return ZKHIP_OK; }
  if (ws_bytes < poly_workspace_bytes(n)) { set_error("eval_polynomial: workspace too small"); return ZKHIP_EINVAL; }
  const scan_plan plan(n, 32);
  const fe_arg* b = nullptr;
  int rc = stage_const(x_host, plan, ws, ws_bytes, stream, &b);
  if (rc != ZKHIP_OK) return rc;
  return horner_eval(nullptr, d_a, 1, plan, b, d_result, ws, stream);
}

// `count` polynomials of n coefficients each, all evaluated at x: d_results[p] = sum_i poly_p[i] x^i.  One launch per level for the whole
// batch (ceil(log_16 n) levels) instead of one scan per polynomial.  Workspace: [pointer table][256: the multipliers][levels]
int fr_eval_polynomial_batch_device(const void* const* d_polys_host, size_t count, size_t n, const uint32_t x_host[8], uint32_t* d_results,
                                    void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring) {
  if (count == 0) return ZKHIP_OK;
  if (n == 0) { HIPCHK(hipMemsetAsync(d_results, 0, count * 32, stream)); return ZKHIP_OK; }
  if (count > 65535) { set_error("eval_polynomial_batch: more than 65535 polynomials"); return ZKHIP_EINVAL; }
  if (ws_bytes < poly_batch_workspace_bytes(n, count)) { set_error("eval_polynomial_batch: workspace too small"); return ZKHIP_EINVAL; }
  const scan_plan plan(n, 32 * count);
  char* p = (char*)ws;
  const uint32_t** d_ptrs = (const uint32_t**)p;
  p += scan_align(count * 8);
  fe_arg* b = (fe_arg*)p;
  p += 256;
  int rc = upload_args(ring, d_ptrs, d_polys_host, count * 8, stream);        // caller memory: through the pinned ring, no wait for the stream
  if (rc == ZKHIP_OK) rc = store_const(x_host, b, stream, plan);
  if (rc != ZKHIP_OK) return rc;
  return horner_eval(d_ptrs, nullptr, count, plan, b, d_results, p, stream);
}

// kate_division: q[i] = a[i+1] + b q[i+1], i < n-1  (quotient of a(X) by (X - b), remainder dropped).  The suffix Horner scan
// s[i] = sum_{j >= i} a[j] b^(j-i) at index i+1 is q[i]: scan everything, drop index 0
int fr_kate_division_device(const uint32_t* d_a, size_t n, const uint32_t b_host[8], uint32_t* d_q, void* ws, size_t ws_bytes,
                            hipStream_t stream) {
  if (n < 2) return ZKHIP_OK;
  if (ws_bytes < poly_workspace_bytes(n)) { set_error("kate_division: workspace too small"); return ZKHIP_EINVAL; }
  const scan_plan plan(n, 32);
  const fe_arg* b = nullptr;
  int rc = stage_const(b_host, plan, ws, ws_bytes, stream, &b);
  if (rc != ZKHIP_OK) return rc;
  auto level = [&](int k) { return plan.level<uint32_t>(ws, k); };
  for (int k = 1; k <= plan.L; k++)
    hipLaunchKernelGGL(k_horner_agg, grid_for(plan.n[k], 256), dim3(256), 0, stream, k == 1 ? d_a : (const uint32_t*)level(k - 1), plan.n[k - 1], b + (k - 1), level(k));
  for (int k = plan.L; k >= 0; k--)
    hipLaunchKernelGGL(k_horner_apply, grid_for(plan.n[k + 1], 256), dim3(256), 0, stream, k ? (const uint32_t*)level(k) : d_a, plan.n[k], b + k,
                       k < plan.L ? (const uint32_t*)level(k + 1) : (const uint32_t*)nullptr, plan.n[k + 1], k ? level(k) : d_q, (size_t)(k ? 0 : 1));
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// ---- division by the vanishing polynomial of a point set (multi-open: `div_by_vanishing`) ---------------------------------------
// q = floor(a / Z), Z(X) = prod_{i < M} (X - z_i) = X^M + sum_j c_j X^j, in ONE pass structure whatever M: a is read twice and q written once,
// where the fold of M kate_divisions reads 2 M times and writes M times.
//   Division from the top is a linear recurrence whose state is the running remainder R_t = (sum_{j >= t} a_j X^(j - t)) mod Z, M
//   coefficients r_0 .. r_(M-1):   q[t] = r_(M-1) of R_(t+1);   R_t = a[t] + X R_(t+1) - q[t] Z, i.e. r_j <- r_(j-1) - q[t] c_j, r_0 <- a[t] - q[t] c_0.
//   M independent multiplications per element (the fold spends 2 M), and R_t is the interpolant of the M suffix Horner values
//   S_i[t] = sum_{j >= t} a_j z_i^(j - t) over the points -- so the carries of the chunked scheme stay M independent scalars:
//   pass A   per chunk the M Horner aggregates from one load of the chunk (k_roots_agg);
//   levels   the M aggregate arrays scanned as kate_division scans its one, blockIdx.y = root (k_roots_agg_level up, k_roots_apply_level down);
//   pass B   each thread turns its M carries S_i[hi] into R_hi with the M x M matrix V[j][i] = [X^j] Z(X) / ((X - z_i) Z'(z_i)) (Lagrange basis
//            coefficients: host arithmetic on a handful of points, one inversion) and steps the recurrence, one store per element.
// The zero tail q[n - M .. n) needs no code: R_t has degree < n - t, so its top coefficient is zero there.  a(z_i) is the scanned level-1
// aggregate at index 0.  Every multiplier -- z_i^(CH^level), -c_j, V -- is computed on the host (fp29.hpp compiles there) in the internal form
// and travels as a kernel argument: nothing is staged on the device, the constants sit in scalar registers.
struct roots_k { uint32_t l[ZKHIP_MAX_ROOTS][NL]; };                                     // one internal-form canonical constant per root
struct roots_div_k { uint32_t nc[ZKHIP_MAX_ROOTS][NL]; uint32_t v[ZKHIP_MAX_ROOTS][ZKHIP_MAX_ROOTS][NL]; };   // -c_j; V[j][i]

__device__ __forceinline__ fe fe_from_limbs(const uint32_t (&l)[NL]) {
  fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = l[i];
  return r;
}

// pass A for M roots: agg[i * stride + t] = sum_{e in chunk t} a[e] z_i^(e - lo).  M x 9 registers of state per lane, the chunk loaded once.
template <int M>
__global__ void __launch_bounds__(256) k_roots_agg(const uint32_t* __restrict__ a, size_t n, const roots_k zk, uint32_t* __restrict__ agg, size_t stride) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  fe q[M];
#pragma unroll
  for (int r = 0; r < M; r++) q[r] = fe_zero();
  // static_for, not `#pragma unroll`: the body is M multiplications long and the unroller gives up on it, which sends q[] to scratch memory
  auto step = [&](const fe& x) {
    static_for<0, M>([&](auto r) { q[r] = fe_norm(fe_add(x, fe_mul<Fr>(fe_from_limbs(zk.l[r]), q[r]))); });   // < 3p, N (as k_horner_agg)
  };
  size_t i = hi;
  for (; i >= lo + 4 && ((i & 3) == 0); i -= 4) {               // four elements = one 128-byte line per lane, loaded together (see k_horner_agg)
    uint32_t w[4][8];
    static_for<0, 4>([&](auto e) { load_words(a + (i - 4 + e) * 8, w[e]); });
    static_for<0, 4>([&](auto e) { step(fe_unpack<0>(w[3 - e])); });
  }
  for (; i-- > lo;) step(load_ext(a, i));
  static_for<0, M>([&](auto r) { store_canon(agg + (size_t)r * stride * 8, t, q[r]); });
}

// the recursion levels: blockIdx.y = root, dense [m][n] arrays, the level's multipliers z_i^(CH^level) in zk
__global__ void __launch_bounds__(256) k_roots_agg_level(const uint32_t* __restrict__ base, size_t n, const roots_k zk, uint32_t* __restrict__ agg, size_t m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  const uint32_t* a = base + (size_t)blockIdx.y * n * 8;
  const fe b = fe_from_limbs(zk.l[blockIdx.y]);
  fe q = fe_zero();
  for (size_t i = hi; i-- > lo;) q = fe_norm(fe_add(load_ext(a, i), fe_mul<Fr>(b, q)));
  store_canon(agg + (size_t)blockIdx.y * m * 8, t, q);
}
// in place: arr[i] <- arr[i] + b * arr[i + 1] (suffix scan) with carry-in carry[t + 1]; a thread reads and writes its own chunk only, top down
__global__ void __launch_bounds__(256) k_roots_apply_level(uint32_t* base, size_t n, const roots_k zk, const uint32_t* carry_base, size_t ncarry) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  uint32_t* a = base + (size_t)blockIdx.y * n * 8;
  const fe b = fe_from_limbs(zk.l[blockIdx.y]);
  fe q = (carry_base != nullptr && t + 1 < ncarry) ? load_ext(carry_base + (size_t)blockIdx.y * ncarry * 8, t + 1) : fe_zero();
  for (size_t i = hi; i-- > lo;) {
    q = fe_norm(fe_add(load_ext(a, i), fe_mul<Fr>(b, q)));
    store_canon(a, i, q);
  }
}

// pass B.  Magnitudes: V, nc canonical (< p); a carry is canonical, so each product of the conversion is < p (p^2 / (p 2^261) + 1) < 1.01 p and
// r_j < 1.01 M p.  In the loop q is soft-reduced (< 2p + 2^233 < 3p, N) before it is stored and multiplied: q nc_j < 1.02 p, and an r_j
// collects at most M - 1 such products on top of its start (or M and one a[t] < p) before it becomes q: value < 2.03 M p < 17 p < 2^261 for M = 8,
// the bound of fe_reduce_soft.  Limbs: every term is N-limbed (< 2^29), r_j is a plain sum of at most M + 1 of them: < 2^32 up to M = 7; M = 8 carries
// once per step.  Only q, normalised, is ever a multiplication operand.
template <int M>
__global__ void __launch_bounds__(256) k_roots_div(const uint32_t* __restrict__ a, size_t n, const roots_div_k k, const uint32_t* __restrict__ carry,
                                                   size_t ncarry, uint32_t* __restrict__ out, uint32_t* __restrict__ evals) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lo = t * SCAN_CH;
  if (lo >= n) return;
  const size_t hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  fe r[M];
#pragma unroll
  for (int j = 0; j < M; j++) r[j] = fe_zero();
  if (carry != nullptr && t + 1 < ncarry) {
    fe s[M];
    static_for<0, M>([&](auto i) { s[i] = load_ext(carry + (size_t)i * ncarry * 8, t + 1); });
    static_for<0, M>([&](auto j) {
      fe acc = fe_zero();
      static_for<0, M / 2>([&](auto h) {                        // two products per reduction: 9 * 2 * 2^58 + 9 * 2^58 + 2^35 < 2^64 (fe_mul_add), all limbs < 2^29
        constexpr int i = 2 * h;
        acc = fe_add(acc, fe_mul_add<Fr>(fe_from_limbs(k.v[j][i]), s[i], fe_from_limbs(k.v[j][i + 1]), s[i + 1]));
      });
      if (M & 1) acc = fe_add(acc, fe_mul<Fr>(fe_from_limbs(k.v[j][M - 1]), s[M - 1]));
      r[j] = fe_norm(acc);
    });
  }
  if (evals != nullptr && t == 0 && carry != nullptr) {        // a(z_i): the scan of the level-1 aggregates at index 0 (canonical already)
#pragma unroll
    for (int i = 0; i < M; i++) {
      uint32_t w[8];
      load_words(carry + (size_t)i * ncarry * 8, w);
      store_words(evals + i * 8, w);
    }
  }
  auto step = [&](const fe& x, size_t idx) {                  // static_for: see k_roots_agg
    const fe q = fe_reduce_soft<Fr>(fe_norm(r[M - 1]));
    store_canon(out, idx, q);
    static_for<1, M>([&](auto jj) {
      constexpr int j = M - jj;                                 // M - 1 .. 1: r[j - 1] is read before it is replaced
      r[j] = fe_add(r[j - 1], fe_mul<Fr>(fe_from_limbs(k.nc[j]), q));
      if (M > 7) r[j] = fe_norm(r[j]);
    });
    r[0] = fe_add(x, fe_mul<Fr>(fe_from_limbs(k.nc[0]), q));
  };
  size_t i = hi;
  for (; i >= lo + 4 && ((i & 3) == 0); i -= 4) {               // four elements = one 128-byte line per lane, loaded together (see k_horner_agg)
    uint32_t w[4][8];
    static_for<0, 4>([&](auto e) { load_words(a + (i - 4 + e) * 8, w[e]); });
    static_for<0, 4>([&](auto e) { step(fe_unpack<0>(w[3 - e]), i - 1 - e); });
  }
  for (; i-- > lo;) step(load_ext(a, i), i);
}

// host arithmetic on the points (internal form, canonical values)
static fe h_mul(const fe& a, const fe& b) { return fe_canon_lt2p<Fr>(fe_mul<Fr>(a, b)); }
static fe h_add(const fe& a, const fe& b) { return fe_canon_lt2p<Fr>(fe_norm(fe_add(a, b))); }
static fe h_neg(const fe& a) {
  if (fe_is_zero_limbs(a)) return a;
  fe r;
  int32_t borrow = 0;
  for (int i = 0; i < NL; i++) {
    int32_t t = (int32_t)Fr::P[i] - (int32_t)a.l[i] + borrow;
    borrow = t >> 31;
    r.l[i] = i < NL - 1 ? ((uint32_t)t & LMASK) : (uint32_t)t;
  }
  return r;
}
static fe h_sub(const fe& a, const fe& b) { return h_add(a, h_neg(b)); }
static fe h_from_ext(const uint32_t w[8]) {
  uint32_t ww[8];
  memcpy(ww, w, 32);
  return h_mul(fe_const<Fr>(Fr::FROM_EXT), fe_unpack<0>(ww));
}
static fe h_inverse(const fe& a) {                            // a^(r - 2): the bits of r - 2 from the limbs of r
  uint32_t e[NL];
  for (int i = 0; i < NL; i++) e[i] = Fr::P[i];
  e[0] -= 2;                                                   // the low limb of r is 0x10000001: no borrow
  fe acc = fe_one<Fr>();
  for (int bit = LB * NL - 1; bit >= 0; bit--) {
    acc = h_mul(acc, acc);
    if ((e[bit / LB] >> (bit % LB)) & 1) acc = h_mul(acc, a);
  }
  return acc;
}
static void h_store(const fe& a, uint32_t (&l)[NL]) { for (int i = 0; i < NL; i++) l[i] = a.l[i]; }

// f(std::integral_constant<int, M>) for the run-time root count m in 1 .. ZKHIP_MAX_ROOTS: the kernels take it as a template argument
template <int M = 1, class F>
static void with_root_count(uint32_t m, F&& f) {
  if (m == M) f(std::integral_constant<int, M>{});
  else if constexpr (M < ZKHIP_MAX_ROOTS) with_root_count<M + 1>(m, f);
}

int fr_divide_by_roots_device(const uint32_t* d_a, size_t n, const uint32_t (*roots_host)[8], uint32_t m, uint32_t* d_q, uint32_t* d_evals, void* ws,
                              size_t ws_bytes, hipStream_t stream) {
  if (m == 0 || m > ZKHIP_MAX_ROOTS) { set_error("divide_by_roots: %u roots (1 .. %d)", m, ZKHIP_MAX_ROOTS); return ZKHIP_EINVAL; }
  if (n == 0) {
    if (d_evals) HIPCHK(hipMemsetAsync(d_evals, 0, (size_t)m * 32, stream));
    return ZKHIP_OK;
  }
  if (ws_bytes < poly_roots_workspace_bytes(n, m)) { set_error("divide_by_roots: workspace too small"); return ZKHIP_EINVAL; }
  if (m == 1 && !d_evals) {                                   // one root, no evaluation wanted: kate_division as it is, and its one missing element
    int rc = fr_kate_division_device(d_a, n, roots_host[0], d_q, ws, ws_bytes, stream);
    if (rc != ZKHIP_OK) return rc;
    HIPCHK(hipMemsetAsync(d_q + (n - 1) * 8, 0, 32, stream));
    return ZKHIP_OK;
  }
  // constants.  z[i]; Z's coefficients c (monic, degree m); V[j][i] = w_i [X^j] Z / (X - z_i) with w_i = 1 / prod_{j != i} (z_i - z_j)
  fe z[ZKHIP_MAX_ROOTS], c[ZKHIP_MAX_ROOTS + 1], w[ZKHIP_MAX_ROOTS];
  for (uint32_t i = 0; i < m; i++) z[i] = h_from_ext(roots_host[i]);
  c[0] = fe_one<Fr>();
  for (uint32_t i = 0; i < m; i++) {                          // c <- c * (X - z_i)
    c[i + 1] = c[i];
    for (uint32_t j = i; j >= 1; j--) c[j] = h_sub(c[j - 1], h_mul(z[i], c[j]));
    c[0] = h_neg(h_mul(z[i], c[0]));
  }
  fe den = fe_one<Fr>();                                      // one inversion: 1 / prod_i Z'(z_i), then w_i = that times the other derivatives
  fe dz[ZKHIP_MAX_ROOTS];
  for (uint32_t i = 0; i < m; i++) {
    dz[i] = fe_one<Fr>();
    for (uint32_t j = 0; j < m; j++) if (j != i) dz[i] = h_mul(dz[i], h_sub(z[i], z[j]));
    den = h_mul(den, dz[i]);
  }
  if (fe_is_zero_limbs(den)) { set_error("divide_by_roots: two equal roots"); return ZKHIP_EINVAL; }
  const fe den_inv = h_inverse(den);
  for (uint32_t i = 0; i < m; i++) {
    w[i] = den_inv;
    for (uint32_t j = 0; j < m; j++) if (j != i) w[i] = h_mul(w[i], dz[j]);
  }
  roots_div_k dk;
  memset(&dk, 0, sizeof dk);
  for (uint32_t j = 0; j < m; j++) h_store(h_neg(c[j]), dk.nc[j]);
  for (uint32_t i = 0; i < m; i++) {                          // Z / (X - z_i) by synthetic division from the top: d_(m-1) = 1, d_(j-1) = c_j + z_i d_j
    fe d = fe_one<Fr>();
    for (uint32_t j = m; j-- > 0;) {
      h_store(h_mul(w[i], d), dk.v[j][i]);
      d = h_add(c[j], h_mul(z[i], d));
    }
  }
  roots_k zk;
  memset(&zk, 0, sizeof zk);
  for (uint32_t i = 0; i < m; i++) h_store(z[i], zk.l[i]);
  auto next_level = [&]() {                                   // z_i <- z_i^CH
    static_assert(SCAN_CH == 16, "z^CH below is four squarings");
    for (uint32_t i = 0; i < m; i++) { for (int s = 0; s < 4; s++) z[i] = h_mul(z[i], z[i]); h_store(z[i], zk.l[i]); }
  };

  const scan_plan plan(n, 32 * (size_t)m);
  auto level = [&](int k) { return plan.level<uint32_t>(ws, k); };
  const uint32_t* carry = plan.L ? level(1) : nullptr;
  // up.  Level 1 (with one chunk and no carries: the evaluations themselves) takes all m aggregates from one load of a chunk
  if (plan.L || d_evals)
    with_root_count(m, [&](auto M) {
      hipLaunchKernelGGL(k_roots_agg<M>, grid_for(plan.n[1], 256), dim3(256), 0, stream, d_a, n, zk, plan.L ? level(1) : d_evals, plan.n[1]);
    });
  roots_k zks[SCAN_MAX_LEVELS + 1];                           // the multipliers of level k: z^(CH^k)
  for (int k = 1; k <= plan.L; k++) {
    next_level();
    zks[k] = zk;
    if (k < plan.L) hipLaunchKernelGGL(k_roots_agg_level, grid_for(plan.n[k + 1], 256, m), dim3(256), 0, stream, (const uint32_t*)level(k), plan.n[k], zk, level(k + 1), plan.n[k + 1]);
  }
  for (int k = plan.L; k >= 1; k--)                           // down: every level in place with the scanned level above as carries
    hipLaunchKernelGGL(k_roots_apply_level, grid_for(plan.n[k + 1], 256, m), dim3(256), 0, stream, level(k), plan.n[k], zks[k],
                       k < plan.L ? (const uint32_t*)level(k + 1) : (const uint32_t*)nullptr, plan.n[k + 1]);
  with_root_count(m, [&](auto M) {
    hipLaunchKernelGGL(k_roots_div<M>, grid_for(plan.n[1], 256), dim3(256), 0, stream, d_a, n, dk, carry, plan.n[1], d_q, d_evals);
  });
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// exclusive prefix products of `batch` dense arrays of n elements each: out[b][0] = 1.  d_out may be d_v: each lane reads before it writes
static int prefix_product_batch(const uint32_t* d_v, uint32_t* d_out, size_t n, uint32_t batch, void* ws, hipStream_t stream) {
  const scan_plan plan(n, 32 * (size_t)batch);
  auto level = [&](int k) { return plan.level<uint32_t>(ws, k); };
  for (int k = 1; k <= plan.L; k++)                            // up: the chunk products of every level
    hipLaunchKernelGGL(k_prod_agg_batch, grid_for(plan.n[k], 256, batch), dim3(256), 0, stream, k == 1 ? d_v : (const uint32_t*)level(k - 1), plan.n[k - 1], level(k), plan.n[k]);
  for (int k = plan.L; k >= 0; k--)                            // down: every level in place, with the scanned level above as carries
    hipLaunchKernelGGL(k_prod_apply_batch, grid_for(plan.n[k + 1], 256, batch), dim3(256), 0, stream, k ? (const uint32_t*)level(k) : d_v, plan.n[k],
                       k < plan.L ? (const uint32_t*)level(k + 1) : (const uint32_t*)nullptr, plan.n[k + 1], k ? level(k) : d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// exclusive prefix product: out[0] = 1, out[i] = v[0] ... v[i-1]   (out may alias v)
int fr_prefix_product_device(const uint32_t* d_v, size_t n, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  if (ws_bytes < poly_workspace_bytes(n)) { set_error("prefix_product: workspace too small"); return ZKHIP_EINVAL; }
  return prefix_product_batch(d_v, d_out, n, 1, ws, stream);
}

// ---- permutation argument: every set's grand product in one call ----------------------------------------------------------------
// [DEP] halo2-axiom plonk/permutation/prover.rs `Argument::commit` (reached from create_proof, /root/reference/aggregator/src/wrapper.rs:129):
// the permutation's columns are cut into sets of `chunk` (= degree - 2) columns; per set and row
//     den = prod_j (v_j[i] + beta sigma_j[i] + gamma)        num = prod_j (v_j[i] + beta delta^c omega^i + gamma),  c = the column's index
//     z_s[0] = z_(s-1)[u] (1 for the first set),  z_s[i + 1] = z_s[i] num[i] / den[i]
// with u the last usable row.  Only the rows below u enter any set's z[u], so with the ratio of the rows >= u forced to 1 the chained
// products of ALL sets are ONE exclusive prefix product over the [sets][n] array: set s starts at the product of the earlier sets' usable
// rows, which is z_(s-1)[u].  Three kernels of (sets x n) threads + the scan, whatever the number of sets (the state-transition and voter
// shapes of the reference have hundreds of columns at k = 13 .. 15: one call per set was 5 launches of 2^13 threads each, 135 times).

// table[i] = scale * base^(i << shift) in the INTERNAL form (x 2^261), canonical words: fe_unpack<0> of an entry is a reduced operand
__global__ void __launch_bounds__(256) k_pow_table_internal(fe_arg base, fe_arg scale, int has_scale, uint32_t shift, uint32_t count, uint32_t* __restrict__ table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  fe b = fr_const_internal(base);
  for (uint32_t s = 0; s < shift; s++) b = fe_sqr<Fr>(b);
  fe v = fr_pow_u32(b, i);                                                          // < 2p, N
  if (has_scale) v = fe_mul<Fr>(v, fr_const_internal(scale));
  store_canon(table, i, v);
}

// z[s][i] = prod_j (v_j[i] + beta sigma_j[i] + gamma) over the columns of set s, external domain
__global__ void __launch_bounds__(256) k_perm_den(const uint32_t* const* __restrict__ values, const uint32_t* const* __restrict__ sigmas, uint32_t nperm,
                                                  uint32_t chunk, size_t n, const uint32_t* __restrict__ ctab, fe_arg gamma, uint32_t* __restrict__ z) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = blockIdx.y, lo = s * chunk, cnt = nperm - lo < chunk ? nperm - lo : chunk;
  const fe b = load_ext(ctab, 0), g_int = load_ext(ctab, 1);                          // beta, gamma in the internal form (canonical: < p, N)
  // first column in the external domain (beta_internal x sigma_external is external), the others in the internal one: external x internal
  // products stay external, so the result needs no conversion.  Sums of three: limbs < 3 * 2^29.
  fe acc = fe_add(fe_add(load_ext(values[lo], i), fe_mul<Fr>(b, load_ext(sigmas[lo], i))), fe_unpack<0>(gamma.w));     // < 4p
  for (uint32_t j = 1; j < cnt; j++) {
    uint32_t wv[8], ws[8];
    load_words(values[lo + j] + i * 8, wv);
    load_words(sigmas[lo + j] + i * 8, ws);
    const fe t = fe_add(fe_add(fe_unpack<5>(wv), fe_mul<Fr>(b, fe_unpack<5>(ws))), g_int);                              // < 36p
    acc = fe_mul<Fr>(fe_norm(acc), t);                                                                                 // 4 * 36 < 169: < 2p, N
  }
  if (cnt == 1) acc = fe_mul<Fr>(fe_norm(acc), fe_one<Fr>());                                                         // reduce the lone sum
  store_canon(z + (size_t)s * n * 8, i, acc);
}

// z[s][i] <- z[s][i] * prod_j (v_j[i] + (beta delta^c) omega^i + gamma) for i < usable, 1 for the rows from `usable` on
__global__ void __launch_bounds__(256) k_perm_num_mul(const uint32_t* const* __restrict__ values, uint32_t nperm, uint32_t chunk, size_t n, size_t usable,
                                                      const uint32_t* __restrict__ ctab, const uint32_t* __restrict__ dtab, const uint32_t* __restrict__ pow_lo,
                                                      const uint32_t* __restrict__ pow_hi, uint32_t h, uint32_t* __restrict__ z) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = blockIdx.y, lo = s * chunk, cnt = nperm - lo < chunk ? nperm - lo : chunk;
  uint32_t* zs = z + (size_t)s * n * 8;
  if (i >= usable) {                                                                  // 1 in the external domain = 2^256 mod r
    fe one;
#pragma unroll
    for (int k = 0; k < NL; k++) one.l[k] = Fr::TO_EXT[k];
    store_canon(zs, i, one);
    return;
  }
  const fe g_int = load_ext(ctab, 1);
  const fe x = fe_mul<Fr>(load_ext(pow_lo, i & ((1u << h) - 1)), load_ext(pow_hi, i >> h));   // omega^i, internal, < 2p (table entries are internal forms)
  fe acc = fe_zero();
  for (uint32_t j = 0; j < cnt; j++) {
    uint32_t wv[8];
    load_words(values[lo + j] + i * 8, wv);
    const fe t = fe_add(fe_add(fe_unpack<5>(wv), fe_mul<Fr>(load_ext(dtab, lo + j), x)), g_int);   // internal, < 36p, limbs < 3 * 2^29
    acc = j == 0 ? t : fe_mul<Fr>(fe_norm(acc), t);                                              // 36 * 36 / 169 + 1 < 9p, then < 3p, < 2p: N
  }
  store_canon(zs, i, fe_mul<Fr>(load_ext(zs, i), fe_norm(acc)));                                 // external (1 / den) x internal: external, < 2p
}

int fr_permutation_products_device(const void* const* d_values_host, const void* const* d_sigmas_host, uint32_t nperm, uint32_t chunk, uint32_t log_n,
                                   size_t usable, const uint32_t beta[8], const uint32_t gamma[8], const uint32_t delta[8], const uint32_t omega[8],
                                   uint32_t* d_z, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring) {
  if (nperm == 0) return ZKHIP_OK;
  const size_t n = (size_t)1 << log_n, nsets = (nperm + chunk - 1) / chunk;
  if (nsets > 65535) { set_error("permutation_products: more than 65535 sets"); return ZKHIP_EINVAL; }
  if (ws_bytes < perm_workspace_bytes(nperm, chunk, log_n)) { set_error("permutation_products: workspace too small"); return ZKHIP_EINVAL; }
  const uint32_t h = (log_n + 1) / 2;
  char* p = (char*)ws;
  const uint32_t** d_ptrs = (const uint32_t**)p;                  // [values ..., sigmas ...]
  p += (((size_t)nperm * 16 + 255) / 256) * 256;
  uint32_t* dtab = (uint32_t*)p;
  p += (((size_t)nperm * 32 + 255) / 256) * 256;
  uint32_t* pow_lo = (uint32_t*)p;
  p += ((size_t)1 << h) * 32;
  uint32_t* pow_hi = (uint32_t*)p;
  p += (n >> h) * 32;
  uint32_t* ctab = (uint32_t*)p;                                  // beta, gamma in the internal form: converted once, not per row
  p += 64;
  p = (char*)ws + ((((size_t)(p - (char*)ws)) + 255) / 256) * 256;
  const size_t rest = ws_bytes - (size_t)(p - (char*)ws);
  int rc = upload_args(ring, d_ptrs, d_values_host, (size_t)nperm * 8, stream);          // caller memory: through the pinned ring, no wait for the stream
  if (rc == ZKHIP_OK) rc = upload_args(ring, d_ptrs + nperm, d_sigmas_host, (size_t)nperm * 8, stream);
  if (rc != ZKHIP_OK) return rc;
  fe_arg b, g, d, w;
  memcpy(b.w, beta, 32); memcpy(g.w, gamma, 32); memcpy(d.w, delta, 32); memcpy(w.w, omega, 32);
  hipLaunchKernelGGL(k_pow_table_internal, dim3(1), dim3(256), 0, stream, d, b, 1, 0u, 1u, ctab);            // delta^0 beta
  hipLaunchKernelGGL(k_pow_table_internal, dim3(1), dim3(256), 0, stream, d, g, 1, 0u, 1u, ctab + 8);        // delta^0 gamma
  hipLaunchKernelGGL(k_pow_table_internal, grid_for(nperm, 256), dim3(256), 0, stream, d, b, 1, 0u, nperm, dtab);
  hipLaunchKernelGGL(k_pow_table_internal, grid_for((size_t)1 << h, 256), dim3(256), 0, stream, w, w, 0, 0u, 1u << h, pow_lo);
  hipLaunchKernelGGL(k_pow_table_internal, grid_for(n >> h, 256), dim3(256), 0, stream, w, w, 0, h, (uint32_t)(n >> h), pow_hi);
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nsets);
  hipLaunchKernelGGL(k_perm_den, grid, dim3(256), 0, stream, (const uint32_t* const*)d_ptrs, (const uint32_t* const*)(d_ptrs + nperm), nperm, chunk, n, (const uint32_t*)ctab, g, d_z);
  HIPCHK(hipGetLastError());
  prof_mark(stream, "perm_den");
  rc = fr_batch_invert_device(d_z, nsets * n, p, rest, stream);
  if (rc != ZKHIP_OK) return rc;
  prof_mark(stream, "perm_invert");
  hipLaunchKernelGGL(k_perm_num_mul, grid, dim3(256), 0, stream, (const uint32_t* const*)d_ptrs, nperm, chunk, n, usable, (const uint32_t*)ctab, (const uint32_t*)dtab,
                     (const uint32_t*)pow_lo, (const uint32_t*)pow_hi, h, d_z);
  HIPCHK(hipGetLastError());
  prof_mark(stream, "perm_num");
  rc = fr_prefix_product_device(d_z, nsets * n, d_z, p, rest, stream);
  prof_mark(stream, "perm_scan");
  return rc;
}

// ---- lookup argument: every lookup's grand product in one call ------------------------------------------------------------------------------
// [DEP] halo2-axiom plonk/lookup/prover.rs `commit_product`: z[0] = 1, z[i + 1] = z[i] (a[i] + beta)(s[i] + gamma) / ((a'[i] + beta)(s'[i] + gamma)) over
// the usable rows.  As with the permutation sets: denominators of all lookups, ONE batch inversion, numerators, one exclusive prefix product with
// the ratio of the rows >= usable forced to 1 (those rows of A' / S' are the caller's blinding rows, or not written yet: they are not read).  Lookups
// do not chain, so the scan restarts at every lookup: its kernels take the lookup as blockIdx.y (a chained scan would need every column divided by
// its own row 0 afterwards: an inversion and a multiply per element more).
__global__ void __launch_bounds__(256) k_lookup_den(const uint32_t* __restrict__ pa, const uint32_t* __restrict__ ps, size_t n, size_t usable, fe_arg beta,
                                                    fe_arg gamma, uint32_t* __restrict__ z) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t off = (size_t)blockIdx.y * n;
  fe acc;
  if (i >= usable) {                                                                  // 1 in the external domain = 2^256 mod r
#pragma unroll
    for (int k = 0; k < NL; k++) acc.l[k] = Fr::TO_EXT[k];
  } else {
    uint32_t ws[8];
    load_words(ps + (off + i) * 8, ws);
    const fe a = fe_add(load_ext(pa, off + i), fe_unpack<0>(beta.w));                 // external, < 2p
    const fe t = fe_add(fe_unpack<5>(ws), fr_const_internal(gamma));                  // internal, < 34p
    acc = fe_mul<Fr>(fe_norm(a), t);                                                  // external x internal: external, < 2p
  }
  store_canon(z, off + i, acc);
}

// z[l][i] <- z[l][i] (a_l[i] + beta)(s_l[i] + gamma) for i < usable; the rows from `usable` on keep their 1
__global__ void __launch_bounds__(256) k_lookup_num_mul(const uint32_t* const* __restrict__ cols, uint32_t n_lookups, size_t n, size_t usable, fe_arg beta,
                                                        fe_arg gamma, uint32_t* __restrict__ z) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= usable) return;
  const uint32_t l = blockIdx.y;
  uint32_t wa[8], ws[8];
  load_words(cols[l] + i * 8, wa);
  load_words(cols[n_lookups + l] + i * 8, ws);
  const fe a = fe_add(fe_unpack<5>(wa), fr_const_internal(beta));                     // internal, < 34p
  const fe t = fe_add(fe_unpack<5>(ws), fr_const_internal(gamma));
  const fe num = fe_mul<Fr>(fe_norm(a), t);                                           // 34 * 34 / 169 + 1 < 8p, then < 2p below
  uint32_t* zl = z + (size_t)l * n * 8;
  store_canon(zl, i, fe_mul<Fr>(load_ext(zl, i), fe_norm(num)));                      // external (1 / den) x internal: external
}

int fr_lookup_products_device(const void* const* d_inputs_host, const void* const* d_tables_host, const uint32_t* d_permuted_inputs, const uint32_t* d_permuted_tables,
                              uint32_t n_lookups, uint32_t log_n, size_t usable, const uint32_t beta[8], const uint32_t gamma[8], uint32_t* d_z, void* ws,
                              size_t ws_bytes, hipStream_t stream, arg_ring* ring) {
  if (n_lookups == 0) return ZKHIP_OK;
  const size_t n = (size_t)1 << log_n;
  if (n_lookups > 65535) { set_error("lookup_products: more than 65535 lookups"); return ZKHIP_EINVAL; }
  if (ws_bytes < lookup_products_workspace_bytes(n_lookups, log_n)) { set_error("lookup_products: workspace too small"); return ZKHIP_EINVAL; }
  char* p = (char*)ws;
  const uint32_t** d_ptrs = (const uint32_t**)p;                  // [inputs ..., tables ...]
  p += (((size_t)n_lookups * 16 + 255) / 256) * 256;
  const size_t rest = ws_bytes - (size_t)(p - (char*)ws);
  int rc = upload_args(ring, d_ptrs, d_inputs_host, (size_t)n_lookups * 8, stream);
  if (rc == ZKHIP_OK) rc = upload_args(ring, d_ptrs + n_lookups, d_tables_host, (size_t)n_lookups * 8, stream);
  if (rc != ZKHIP_OK) return rc;
  fe_arg b, g;
  memcpy(b.w, beta, 32); memcpy(g.w, gamma, 32);
  const dim3 grid((unsigned)((n + 255) / 256), n_lookups);
  hipLaunchKernelGGL(k_lookup_den, grid, dim3(256), 0, stream, d_permuted_inputs, d_permuted_tables, n, usable, b, g, d_z);
  HIPCHK(hipGetLastError());
  rc = fr_batch_invert_device(d_z, (size_t)n_lookups * n, p, rest, stream);
  if (rc != ZKHIP_OK) return rc;
  if (usable) hipLaunchKernelGGL(k_lookup_num_mul, dim3((unsigned)((usable + 255) / 256), n_lookups), dim3(256), 0, stream, (const uint32_t* const*)d_ptrs, n_lookups, n,
                                 usable, b, g, d_z);
  HIPCHK(hipGetLastError());
  return prefix_product_batch(d_z, d_z, n, n_lookups, p, stream);
}

// ---- linear combination of many columns: out[i] = sum_j c_j col_j[i] -------------------------------------------------------------------
// The y- / v-combinations and L(X) of the multi-open provers ([DEP] poly/kzg/multiopen/shplonk/prover.rs: hundreds of polynomials at the
// voter / state-transition column counts).  As a row program this is a chain of `count` dependent multiply-adds per row -- at 2^13 rows
// 128 wavefronts walking 650 instructions one after the other.  Here the columns are cut into groups of LC_GROUP: thread (row, group) adds
// its group's products two at a time under ONE Montgomery reduction (fe_mul_add), a second kernel adds the groups' partial sums; with one
// group the first kernel writes the result itself.  Coefficients are converted to the internal form once, by `count` threads.
constexpr uint32_t LC_GROUP = 32;

__global__ void __launch_bounds__(256) k_to_internal(const uint32_t* __restrict__ ext, uint32_t count, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  fe_arg c;
#pragma unroll
  for (int k = 0; k < 8; k++) c.w[k] = ext[(size_t)i * 8 + k];
  store_canon(out, i, fr_const_internal(c));
}

__global__ void __launch_bounds__(256) k_lincomb(const uint32_t* const* __restrict__ cols, const uint32_t* __restrict__ coeff_int, uint32_t count, size_t n,
                                                 uint32_t* __restrict__ out /* [groups][n] */) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t lo = blockIdx.y * LC_GROUP, hi = lo + LC_GROUP < count ? lo + LC_GROUP : count;
  fe acc = fe_zero();
  uint32_t j = lo;
  for (; j + 1 < hi; j += 2) {          // internal-form coefficient x external value = external; both operands N-form < p: each pair < 2p
    const fe t = fe_mul_add<Fr>(load_ext(coeff_int, j), load_ext(cols[j], i), load_ext(coeff_int, j + 1), load_ext(cols[j + 1], i));
    acc = fe_norm(fe_add(acc, t));
  }
  if (j < hi) acc = fe_norm(fe_add(acc, fe_mul<Fr>(load_ext(coeff_int, j), load_ext(cols[j], i))));
  store_canon(out + (size_t)blockIdx.y * n * 8, i, fe_reduce_soft<Fr>(acc));       // < 34p < 2^261 -> < 2p + 2^233 -> canonical
}

// out[i] = sum_g partial[g][i]
__global__ void __launch_bounds__(256) k_sum_columns(const uint32_t* __restrict__ partial, uint32_t groups, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe acc = load_ext(partial, i);
  for (uint32_t g = 1; g < groups; g++) {
    acc = fe_add(acc, load_ext(partial + (size_t)g * n * 8, i));
    if ((g & 3) == 3) acc = fe_norm(acc);           // four more canonical values per round: limbs stay below 2^32
    if ((g & 63) == 63) acc = fe_reduce_soft<Fr>(acc);     // ... and the value below 2^261 (~169 p) whatever the number of groups
  }
  store_canon(out, i, fe_reduce_soft<Fr>(fe_norm(acc)));
}

size_t lincomb_workspace_bytes(size_t count, size_t n) {
  const size_t groups = (count + LC_GROUP - 1) / LC_GROUP;
  return ((count * 8 + 255) / 256) * 256 + 2 * ((count * 32 + 255) / 256) * 256 + (groups > 1 ? groups * n * 32 : 0) + 256;
}

int fr_linear_combination_device(const void* const* d_cols_host, const uint32_t* coeffs_host, size_t count, size_t n, uint32_t* d_out, void* ws, size_t ws_bytes,
                                 hipStream_t stream, arg_ring* ring) {
  if (n == 0) return ZKHIP_OK;
  if (count == 0) { HIPCHK(hipMemsetAsync(d_out, 0, n * 32, stream)); return ZKHIP_OK; }
  const size_t groups = (count + LC_GROUP - 1) / LC_GROUP;
  if (groups > 65535) { set_error("linear_combination: more than %u columns", 65535u * LC_GROUP); return ZKHIP_EINVAL; }
  if (ws_bytes < lincomb_workspace_bytes(count, n)) { set_error("linear_combination: workspace too small"); return ZKHIP_EINVAL; }
  char* p = (char*)ws;
  const uint32_t** d_ptrs = (const uint32_t**)p;
  p += ((count * 8 + 255) / 256) * 256;
  uint32_t* d_ext = (uint32_t*)p;
  p += ((count * 32 + 255) / 256) * 256;
  uint32_t* d_int = (uint32_t*)p;
  p += ((count * 32 + 255) / 256) * 256;
  uint32_t* partial = (uint32_t*)p;
  int rc = upload_args(ring, d_ptrs, d_cols_host, count * 8, stream);          // caller memory: through the pinned ring, no wait for the stream
  if (rc == ZKHIP_OK) rc = upload_args(ring, d_ext, coeffs_host, count * 32, stream);
  if (rc != ZKHIP_OK) return rc;
  hipLaunchKernelGGL(k_to_internal, grid_for(count, 256), dim3(256), 0, stream, (const uint32_t*)d_ext, (uint32_t)count, d_int);
  hipLaunchKernelGGL(k_lincomb, dim3((unsigned)((n + 255) / 256), (unsigned)groups), dim3(256), 0, stream, (const uint32_t* const*)d_ptrs, (const uint32_t*)d_int,
                     (uint32_t)count, n, groups > 1 ? partial : d_out);
  if (groups > 1) hipLaunchKernelGGL(k_sum_columns, grid_for(n, 256), dim3(256), 0, stream, (const uint32_t*)partial, (uint32_t)groups, n, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int fr_batch_invert_device(uint32_t* d_a, size_t n, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  if (ws_bytes < poly_workspace_bytes(n)) { set_error("batch_invert: workspace too small"); return ZKHIP_EINVAL; }
  // elements per thread: 3 multiplications each + one inversion (~50 multiplications' worth since it is division steps, fe_inverse.hpp).
  // Full chunks when there are enough of them to fill the chip; shorter ones below that, where the call is the latency of one thread.
  uint32_t ch = INV_CH_MAX;
  while (ch > 4 && n / ch < 65536) ch >>= 1;
  // one wavefront per workgroup: with few waves per CU, 128-thread workgroups land pairwise on the same two SIMDs (measured: 1024 waves take
  // 0.098 ms as 512 workgroups of 128 threads, 0.063 ms as 1024 of 64 or 256 of 256 -- profiles/r03_batch_invert_ab.txt)
  hipLaunchKernelGGL(k_batch_invert, grid_for((n + ch - 1) / ch, 64), dim3(64), 0, stream, d_a, n, (uint32_t*)ws, ch);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// ---- the proving key's Lagrange cosets in closed form (zkhip_lagrange_cosets_row_shards_device) -------------------------------------------
// At X = zeta ext_omega^g:  l_i(X) = omega^i (X^n - 1) / (n (X - omega^i)), so
//   l0 = Zn / d0,  l_last = Zn omega^u / d1,  sum_{i in A} l_i = Zn Nm / D       (Zn = (X^n - 1) / n, d0 = X - 1, d1 = X - omega^u)
// with D = prod_{i in A} (X - omega^i) and Nm / D = sum_{i in A} omega^i / (X - omega^i) built up one term at a time.  A is the shorter side
// of the active rows: {0 .. u-1} (l_active = the sum) or {u .. n-1} (l_active = 1 - the sum).  The zeta coset misses the subgroup, so no
// denominator vanishes.  One inversion per lane, the interleaved-lane layout of k_batch_invert: lane l takes window elements l, l + 64, ...
// of its tile.  The forward pass parks the prefix products of den = d0 d1 D, and D and Nm, in the three output slots themselves (internal
// form, canonical); the backward pass steps X back, recomputes d0, d1, and overwrites each slot with its external-form result.
// Window element t is global row g = (start + t) mod 2^ext_k; X and X^n advance by ext_omega^64 and ext_omega^(64 n) per element of a lane.
struct lagrange_consts {
  fe_arg zeta, ext_omega, step, step_inv, step_n, step_n_inv, n_inv, omega, omega_u, omega_a0;
};

__global__ void __launch_bounds__(64) k_lagrange_cosets(uint32_t* __restrict__ out_l0, uint32_t* __restrict__ out_last, uint32_t* __restrict__ out_active,
                                                        size_t W, uint64_t start, uint32_t k, uint32_t ext_k, uint32_t ch, uint32_t n_terms, int active_is_sum,
                                                        lagrange_consts c) {
  const size_t first = (size_t)blockIdx.x * 64 * ch + threadIdx.x;
  if (first >= W) return;
  const uint64_t mask = ((uint64_t)1 << ext_k) - 1;
  const fe one = fe_one<Fr>();
  const fe w = fr_const_internal(c.omega), w_u = fr_const_internal(c.omega_u), w_a0 = fr_const_internal(c.omega_a0);
  const fe step = fr_const_internal(c.step), step_n = fr_const_internal(c.step_n);
  // the lane's first X = zeta ext_omega^g and X^n (k squarings)
  fe x = fe_mul<Fr>(fr_const_internal(c.zeta), fr_pow_u32(fr_const_internal(c.ext_omega), (uint32_t)((start + first) & mask)));
  fe xn = x;
  for (uint32_t s = 0; s < k; s++) xn = fe_sqr<Fr>(xn);
  fe pref = one;
  uint32_t cnt = 0;
  for (size_t i = first; cnt < ch && i < W; i += 64, cnt++) {
    const fe d0 = fe_norm(fe_sub_red(x, one, Fr::P4_S1)), d1 = fe_norm(fe_sub_red(x, w_u, Fr::P4_S1));   // < 6p, N
    fe D = one, nm = fe_zero(), wi = w_a0;
    for (uint32_t a = 0; a < n_terms; a++) {
      const fe d = fe_norm(fe_sub_red(x, wi, Fr::P4_S1));
      nm = fe_norm(fe_add(fe_mul<Fr>(nm, d), fe_mul<Fr>(wi, D)));      // < 4p, N
      D = fe_mul<Fr>(D, d);
      wi = fe_mul<Fr>(wi, w);
    }
    uint32_t wv[8];
    fe_pack(fe_canon_lt2p<Fr>(pref), wv); store_words(out_l0 + i * 8, wv);
    fe_pack(fe_canon_lt2p<Fr>(D), wv); store_words(out_last + i * 8, wv);
    fe_pack(fe_canon_lt3p<Fr>(fe_reduce_soft<Fr>(nm)), wv); store_words(out_active + i * 8, wv);
    pref = fe_mul<Fr>(pref, fe_mul<Fr>(fe_mul<Fr>(d0, d1), D));
    x = fe_mul<Fr>(x, step);
    xn = fe_mul<Fr>(xn, step_n);
  }
  fe inv = fe_inverse<Fr>(pref);
  const fe step_inv = fr_const_internal(c.step_inv), step_n_inv = fr_const_internal(c.step_n_inv), n_inv = fr_const_internal(c.n_inv);
  for (uint32_t j = cnt; j-- > 0;) {
    const size_t i = first + (size_t)j * 64;
    x = fe_mul<Fr>(x, step_inv);
    xn = fe_mul<Fr>(xn, step_n_inv);
    const fe d0 = fe_norm(fe_sub_red(x, one, Fr::P4_S1)), d1 = fe_norm(fe_sub_red(x, w_u, Fr::P4_S1));
    const fe zn = fe_mul<Fr>(fe_norm(fe_sub_red(xn, one, Fr::P4_S1)), n_inv);
    uint32_t wv[8];
    load_words(out_l0 + i * 8, wv);
    const fe pre = fe_unpack<0>(wv);
    load_words(out_last + i * 8, wv);
    const fe D = fe_unpack<0>(wv);
    load_words(out_active + i * 8, wv);
    const fe nm = fe_unpack<0>(wv);
    const fe d01 = fe_mul<Fr>(d0, d1);
    const fe inv_den = fe_mul<Fr>(inv, pre);                       // 1 / (d0 d1 D)
    inv = fe_mul<Fr>(inv, fe_mul<Fr>(d01, D));
    const fe zi = fe_mul<Fr>(zn, inv_den);
    const fe l0 = fe_mul<Fr>(zi, fe_mul<Fr>(d1, D));
    const fe ll = fe_mul<Fr>(fe_mul<Fr>(zi, w_u), fe_mul<Fr>(d0, D));
    fe la = fe_mul<Fr>(fe_mul<Fr>(zi, nm), d01);
    if (!active_is_sum) la = fe_norm(fe_sub_red(one, la, Fr::P4_S1));
    fe_to_ext<Fr>(l0, wv); store_words(out_l0 + i * 8, wv);
    fe_to_ext<Fr>(ll, wv); store_words(out_last + i * 8, wv);
    fe_to_ext<Fr>(la, wv); store_words(out_active + i * 8, wv);
  }
}

int fr_lagrange_cosets_window_device(uint32_t* out_l0, uint32_t* out_last, uint32_t* out_active, size_t W, uint64_t start, uint32_t k, uint32_t ext_k,
                                     uint32_t n_terms, int active_is_sum, const uint32_t consts[10][8], hipStream_t stream) {
  if (W == 0) return ZKHIP_OK;
  lagrange_consts c;
  memcpy(&c, consts, sizeof(c));
  static_assert(sizeof(lagrange_consts) == 10 * 32, "ten constants");
  uint32_t ch = INV_CH_MAX;
  while (ch > 4 && W / ch < 65536) ch >>= 1;
  hipLaunchKernelGGL(k_lagrange_cosets, grid_for((W + ch - 1) / ch, 64), dim3(64), 0, stream, out_l0, out_last, out_active, W, start, k, ext_k, ch, n_terms,
                     active_is_sum, c);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

// The Paillier tally (include/zkhip.h, "Paillier tally"): ciphertexts are integers mod n^2, the homomorphic sum of two votes is their product
// (`paillier_add_native`), and the `prev_vote` of every round of a batch is an exclusive prefix product down a column of ciphertexts.  The
// reference folds one ballot at a time (/root/reference/aggregator/src/utils.rs:337-341); here the fold is a chunked scan over the ring of
// modn.hpp, SCAN_CH ballots per lane and one column per blockIdx.y, driven by the level plan of scan_plan.hpp as the scans of poly.hip are:
//
//   k_pl_agg<TOP>     lane (t, c) multiplies chunk t of column c into agg[c][t].  TOP: the elements are the caller's ballots (canonical, any
//                     384-bit integer, ballot-major) and are converted at the load; below the top they are the Montgomery values of the level above.
//   k_pl_scan         the exclusive scan of one level's aggregates in place, each chunk started from its carry (or from 1).
//   k_pl_apply        the top level again: chunk t of column c starts from carry[c][t] * init[c] and stores the running product in front of every
//                     ballot -- row i of `running` is the reference's prev_vote of round i -- and the tally behind the last one.
//
// Values stay in Montgomery form between the passes: 2 + 2/16 multiplications per ballot by the scan, one to convert it at each of its two
// loads and one to convert each stored row.  The context of the modulus is a kernel argument (modn.hpp).
//
// k_pl_mul is `paillier_add_native` over two arrays; k_pl_encrypt is `paillier_enc_native`, one lane per ciphertext, both powers by the plain
// left-to-right ladder: g^m with the lane's own exponent (a divergent branch per bit), r^n with the exponent read from the kernel's
// arguments, so that its branch is uniform over the wave.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "modn.hpp"
#include "scan_plan.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

constexpr int PL_BLOCK = 64;           // one wave: a multiplication is ~300 multiply-adds, the lanes are worth spreading over the SIMDs
constexpr int PL_W = ZKHIP_PAILLIER_WORDS;

struct pl_words3 {                     // n as a kernel argument: the shared exponent of the encryption
  uint32_t w[6];
};

__device__ __forceinline__ modn pl_load(const uint64_t* __restrict__ p) {
  uint64_t w[PL_W];
#pragma unroll
  for (int i = 0; i < PL_W; i++) w[i] = p[i];
  return modn_from_words(w);
}
__device__ __forceinline__ void pl_store(uint64_t* __restrict__ p, const modn& a) {
  uint64_t w[PL_W];
  modn_to_words(a, w);
#pragma unroll
  for (int i = 0; i < PL_W; i++) p[i] = w[i];
}

// out[i] = a[i] b[i] mod N.  a R mod N is reduced whatever a was; times any b < 2^384 it is a b mod N, reduced.  Each lane reads its two inputs
// before it writes: d_out may be either of them.
__global__ void __launch_bounds__(PL_BLOCK) k_pl_mul(const modn_ctx ctx, const uint64_t* a, const uint64_t* b, size_t count, uint64_t* out) {
  const size_t i = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (i >= count) return;
  const modn x = pl_load(a + i * PL_W), y = pl_load(b + i * PL_W);
  pl_store(out + i * PL_W, modn_mul(y, modn_to_mont(x, ctx), ctx));
}

// element i of column c of a level: TOP the ballots [n][n_cols] canonical, else the level's own array [n_cols][n] of Montgomery values
template <bool TOP>
__device__ __forceinline__ modn pl_elem(const modn_ctx& ctx, const uint64_t* __restrict__ v, size_t n, uint32_t n_cols, uint32_t c, size_t i) {
  if (TOP) return modn_to_mont(pl_load(v + (i * n_cols + c) * PL_W), ctx);
  return pl_load(v + ((size_t)c * n + i) * PL_W);
}

// agg[c][t] = the product of chunk t of column c, Montgomery form; m = chunks of a column
template <bool TOP>
__global__ void __launch_bounds__(PL_BLOCK) k_pl_agg(const modn_ctx ctx, const uint64_t* __restrict__ v, size_t n, uint32_t n_cols, uint64_t* __restrict__ agg, size_t m) {
  const size_t t = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (t >= m) return;
  const size_t lo = t * SCAN_CH, hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  for (uint32_t c = blockIdx.y; c < n_cols; c += gridDim.y) {
    modn acc = pl_elem<TOP>(ctx, v, n, n_cols, c, lo);
    for (size_t i = lo + 1; i < hi; i++) acc = modn_mul(acc, pl_elem<TOP>(ctx, v, n, n_cols, c, i), ctx);
    pl_store(agg + ((size_t)c * m + t) * PL_W, acc);
  }
}

// in place over v[n_cols][n] (Montgomery): v[c][i] = carry[c][t] * prod_{lo <= j < i} v[c][j]; carry == nullptr: 1.  m = chunks of a column
__global__ void __launch_bounds__(PL_BLOCK) k_pl_scan(const modn_ctx ctx, uint64_t* __restrict__ v, size_t n, uint32_t n_cols, const uint64_t* __restrict__ carry, size_t m) {
  const size_t t = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (t >= m) return;
  const size_t lo = t * SCAN_CH, hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  for (uint32_t c = blockIdx.y; c < n_cols; c += gridDim.y) {
    modn cur = carry ? pl_load(carry + ((size_t)c * m + t) * PL_W) : modn_one(ctx);
    for (size_t i = lo; i < hi; i++) {
      uint64_t* at = v + ((size_t)c * n + i) * PL_W;
      const modn f = pl_load(at);                             // read before the store: the scan is in place
      pl_store(at, cur);
      if (i + 1 < hi) cur = modn_mul(cur, f, ctx);
    }
  }
}

// running[i][c] = init[c] * prod_{j < i} ballots[j][c] mod N for 0 <= i <= n, canonical.  carry[c][t] (Montgomery; nullptr: 1) is the product of the
// chunks before t.  Lane 0 exists for n == 0 too and writes row 0.
__global__ void __launch_bounds__(PL_BLOCK) k_pl_apply(const modn_ctx ctx, const uint64_t* __restrict__ ballots, size_t n, uint32_t n_cols, const uint64_t* __restrict__ init,
                                                      const uint64_t* __restrict__ carry, size_t m, uint64_t* __restrict__ running) {
  const size_t t = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (t >= m && t != 0) return;
  const size_t lo = t * SCAN_CH, hi = lo + SCAN_CH < n ? lo + SCAN_CH : n;
  for (uint32_t c = blockIdx.y; c < n_cols; c += gridDim.y) {
    modn cur = init ? modn_to_mont(pl_load(init + (size_t)c * PL_W), ctx) : modn_one(ctx);
    if (carry) cur = modn_mul(cur, pl_load(carry + ((size_t)c * m + t) * PL_W), ctx);
    for (size_t i = lo; i < hi; i++) {
      pl_store(running + (i * n_cols + c) * PL_W, modn_from_mont(cur, ctx));
      cur = modn_mul(cur, pl_elem<true>(ctx, ballots, n, n_cols, c, i), ctx);
    }
    if (hi == n) pl_store(running + (n * n_cols + c) * PL_W, modn_from_mont(cur, ctx));
  }
}

// out[i] = g^m[i] r[i]^n mod N.  g_mont: g R mod N, converted on the host.  m: 4 words per lane, r: 3 words per lane (any value: r >= n is reduced
// mod N by the conversion, as `BigUint` arithmetic would)
__global__ void __launch_bounds__(PL_BLOCK) k_pl_encrypt(const modn_ctx ctx, const modn g_mont, const pl_words3 n_exp, const uint64_t* __restrict__ m, const uint64_t* __restrict__ r,
                                                        size_t count, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (i >= count) return;
  const modn gm = modn_pow(g_mont, reinterpret_cast<const uint32_t*>(m + i * 4), 8, ctx);   // little-endian words: the ladder reads one per 32 steps
  const modn rm = modn_to_mont(modn_from_words(r + i * 3, 3), ctx);
  const modn rn = modn_pow(rm, n_exp.w, 6, ctx);              // the exponent is a kernel argument: the ladder's branch is uniform over the wave
  pl_store(out + i * PL_W, modn_from_mont(modn_mul(gm, rn, ctx), ctx));
}

static inline dim3 pl_grid(size_t lanes, uint32_t n_cols) {
  return dim3((unsigned)((lanes + PL_BLOCK - 1) / PL_BLOCK), n_cols < 65535u ? n_cols : 65535u);
}

// false for an even n or n < 3: Montgomery needs an odd modulus
bool paillier_context(const uint64_t n[3], modn_ctx* ctx) {
  uint32_t N[MODN_L];
  modn_square_words(n, 3, N);
  return modn_ctx_build(N, ctx);
}

int paillier_mul_device(const modn_ctx& ctx, const uint64_t* d_a, const uint64_t* d_b, size_t count, uint64_t* d_out, hipStream_t stream) {
  if (count == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_pl_mul, pl_grid(count, 1), dim3(PL_BLOCK), 0, stream, ctx, d_a, d_b, count, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int paillier_tally_device(const modn_ctx& ctx, const uint64_t* d_ballots, size_t n_ballots, uint32_t n_cols, const uint64_t* d_init, uint64_t* d_running, void* ws,
                          size_t ws_bytes, hipStream_t stream) {
  if (ws_bytes < paillier_tally_workspace_bytes(n_ballots, n_cols)) { set_error("paillier_tally: workspace too small"); return ZKHIP_EINVAL; }
  const scan_plan plan(n_ballots, (size_t)n_cols * PL_W * 8);
  auto level = [&](int k) { return plan.level<uint64_t>(ws, k); };
  for (int k = 1; k <= plan.L; k++) {                         // up: the chunk products of every level until one chunk holds a column
    if (k == 1) hipLaunchKernelGGL(k_pl_agg<true>, pl_grid(plan.n[1], n_cols), dim3(PL_BLOCK), 0, stream, ctx, d_ballots, n_ballots, n_cols, level(1), plan.n[1]);
    else hipLaunchKernelGGL(k_pl_agg<false>, pl_grid(plan.n[k], n_cols), dim3(PL_BLOCK), 0, stream, ctx, (const uint64_t*)level(k - 1), plan.n[k - 1], n_cols, level(k), plan.n[k]);
  }
  for (int k = plan.L; k >= 1; k--)                           // down: every level scanned in place from the carries of the level above it
    hipLaunchKernelGGL(k_pl_scan, pl_grid(plan.n[k + 1], n_cols), dim3(PL_BLOCK), 0, stream, ctx, level(k), plan.n[k], n_cols,
                       k < plan.L ? (const uint64_t*)level(k + 1) : (const uint64_t*)nullptr, plan.n[k + 1]);
  hipLaunchKernelGGL(k_pl_apply, pl_grid(plan.n[1] ? plan.n[1] : 1, n_cols), dim3(PL_BLOCK), 0, stream, ctx, d_ballots, n_ballots, n_cols, d_init,
                     plan.L ? (const uint64_t*)level(1) : (const uint64_t*)nullptr, plan.n[1], d_running);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int paillier_encrypt_device(const modn_ctx& ctx, const uint64_t n[3], const uint64_t g[6], const uint64_t* d_m, const uint64_t* d_r, size_t count, uint64_t* d_out,
                            hipStream_t stream) {
  if (count == 0) return ZKHIP_OK;
  const modn g_mont = modn_to_mont(modn_from_words(g), ctx);
  pl_words3 e;
  for (int i = 0; i < 3; i++) {
    e.w[2 * i] = (uint32_t)n[i];
    e.w[2 * i + 1] = (uint32_t)(n[i] >> 32);
  }
  hipLaunchKernelGGL(k_pl_encrypt, pl_grid(count, 1), dim3(PL_BLOCK), 0, stream, ctx, g_mont, e, d_m, d_r, count, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

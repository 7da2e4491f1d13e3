// The row MSM (include/zkhip.h, "KZG accumulators"): n_rows independent small multi-scalar multiplications in one launch set,
//     out[i] = sum_{j < n_own} rows[i][j] own[i][j]  +  sum_{j >= n_own} rows[i][j] shared[j - n_own],
// the two points a KZG accumulator is made of, for every proof of a batch at once (`PlonkSuccinctVerifier::verify` of the reference,
// aggregator/src/wrapper.rs:433-536, returns them per snark; `KzgAs` absorbs them one by one).  The bucket MSM of msm.hip
// is the wrong tool: a row has 33 (wrapper) or 954 (voter) columns, its own points differ from row to row, and there are B of them.
//
// Shape (row_msm.hpp has the arithmetic): a workgroup is one wavefront; lane j of chunk c multiplies column 64 c + j with a GLV joint ladder
// -- k = k1 + lambda k2, |k_i| < 2^127 (glv.hpp), so 128 doublings and at most 128 additions of one of +-P, +-phi(P), +-P +- phi(P) instead of
// 254 and ~127 -- and a tree in LDS adds the wavefront's 64 terms.  The table entry is chosen by selects on the limbs, not by a branch per
// entry and not by an index: the three additions would serialise in a divergent wavefront, and an indexed table would live in scratch.
// Rows wider than a chunk leave one XYZZ partial sum per chunk, and a second launch adds them per row.
// The ladder is a dependent chain of ~128 (doubling + addition) ~ 3000 field products per lane whatever B is: the call is latency-bound
// until the chip is full of wavefronts.
//
// Also here: the kernels of kzg_limbs.hpp (a point <-> six Fr limbs), one point per lane.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ec.hpp"
#include "glv.hpp"
#include "kzg_limbs.hpp"
#include "msm_digits.hpp"
#include "row_msm.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {
namespace {

constexpr uint32_t XW = 4 * NL;                  // words of an XYZZ point (ROW_MSM_XYZZ_BYTES / 4)
static_assert(XW * 4 == ROW_MSM_XYZZ_BYTES, "row_msm.hpp sizes the partial sums");
constexpr uint32_t TREE_SLOTS = ROW_MSM_LANES / 2;

// the exchange array is word-major ([word][slot]): the lanes of a wavefront touch consecutive banks
ZK_D void xch_put(uint32_t* xch, uint32_t slot, const xyzz& a) {
#pragma unroll
  for (int i = 0; i < NL; i++) {
    xch[(0 * NL + i) * TREE_SLOTS + slot] = a.X.l[i];
    xch[(1 * NL + i) * TREE_SLOTS + slot] = a.Y.l[i];
    xch[(2 * NL + i) * TREE_SLOTS + slot] = a.ZZ.l[i];
    xch[(3 * NL + i) * TREE_SLOTS + slot] = a.ZZZ.l[i];
  }
}
ZK_D xyzz xch_get(const uint32_t* xch, uint32_t slot) {
  xyzz a;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    a.X.l[i] = xch[(0 * NL + i) * TREE_SLOTS + slot];
    a.Y.l[i] = xch[(1 * NL + i) * TREE_SLOTS + slot];
    a.ZZ.l[i] = xch[(2 * NL + i) * TREE_SLOTS + slot];
    a.ZZZ.l[i] = xch[(3 * NL + i) * TREE_SLOTS + slot];
  }
  return a;
}

// lane 0 returns the sum of the 64 lanes' points.  Every lane of the workgroup calls it (barriers inside).
ZK_D xyzz tree_sum(xyzz acc, uint32_t* xch, uint32_t lane) {
#pragma unroll 1
  for (uint32_t s = TREE_SLOTS; s >= 1; s >>= 1) {
    __syncthreads();                                               // the level above has read its slots
    if (lane >= s && lane < 2 * s) xch_put(xch, lane - s, acc);
    __syncthreads();
    if (lane < s) acc = xyzz_add(acc, xch_get(xch, lane));         // equal points double, opposite points cancel (ec.hpp)
  }
  return acc;
}

ZK_D fe fe_pick(bool first, const fe& a, const fe& b) {
  fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = first ? a.l[i] : b.l[i];
  return r;
}

// scalar (external Montgomery words of Fr, any 256-bit value) * the affine point `idx` of `pts`
ZK_D xyzz column_term(const uint32_t* __restrict__ scalar, const uint32_t* __restrict__ pts, size_t idx) {
  uint32_t k[8];
  load_words(scalar, k);
  fe_pack(fr_ext_to_canon(k), k);                                  // the canonical integer below r
  const affine_words pt = load_affine(pts, idx);
  if (words_zero(k) || affine_is_identity(pt)) return xyzz_identity();
  uint32_t m1[4], m2[4];
  bool s1, s2;
  glv::decompose(k, m1, s1, m2, s2);                               // k = +-m1 +- lambda m2
  const fe one = fe_one<Fq>();
  uint32_t bw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) bw[i] = glv::BETA_EXT[i];
  const fe x = fe_mul<Fq>(one, fe_from_ext_lazy(pt.x));            // < 1.4p, N
  const fe y = fe_mul<Fq>(one, fe_from_ext_lazy(pt.y));
  const fe yn = fe_norm(fe_neg_red(y, Fq::P3_S1));                 // 3p - y < 3p, N
  // the table: T1 = +-P, T2 = +-phi(P) (both with ZZ = ZZZ = 1), T3 = T1 + T2
  xyzz T1, T2;
  T1.X = x;
  T1.Y = fe_pick(s1, yn, y);
  T2.X = fe_mul<Fq>(fe_mul<Fq>(one, fe_from_ext_lazy(bw)), x);
  T2.Y = fe_pick(s2, yn, y);
  T1.ZZ = T1.ZZZ = T2.ZZ = T2.ZZZ = one;
  xyzz T3 = T1;
  xyzz_madd_nz(T3, T2.X, T2.Y);                                    // (beta x = x only at x = 0: the same-x branch doubles or cancels)
  xyzz acc = xyzz_identity();
#pragma unroll 1
  for (int bit = 0; bit < 128; bit++) {                            // MSB first; the magnitudes are shifted so that every index is static
    acc = xyzz_dbl(acc);
    const uint32_t b1 = m1[3] >> 31, b2 = m2[3] >> 31;
#pragma unroll
    for (int i = 3; i > 0; i--) {
      m1[i] = (m1[i] << 1) | (m1[i - 1] >> 31);
      m2[i] = (m2[i] << 1) | (m2[i - 1] >> 31);
    }
    m1[0] <<= 1;
    m2[0] <<= 1;
    if (b1 | b2) {
      xyzz B;
      B.X = fe_pick(b1 & b2, T3.X, fe_pick(b1, T1.X, T2.X));
      B.Y = fe_pick(b1 & b2, T3.Y, fe_pick(b1, T1.Y, T2.Y));
      B.ZZ = fe_pick(b1 & b2, T3.ZZ, one);
      B.ZZZ = fe_pick(b1 & b2, T3.ZZZ, one);
      acc = xyzz_add(acc, B);
    }
  }
  return acc;
}

ZK_D void store_partial(uint32_t* p, const xyzz& a) {
  uint4* q = reinterpret_cast<uint4*>(p);
  uint32_t w[XW];
#pragma unroll
  for (int i = 0; i < NL; i++) { w[i] = a.X.l[i]; w[NL + i] = a.Y.l[i]; w[2 * NL + i] = a.ZZ.l[i]; w[3 * NL + i] = a.ZZZ.l[i]; }
#pragma unroll
  for (int i = 0; i < (int)XW / 4; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
ZK_D xyzz load_partial(const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint32_t w[XW];
#pragma unroll
  for (int i = 0; i < (int)XW / 4; i++) { const uint4 v = q[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
  xyzz a;
#pragma unroll
  for (int i = 0; i < NL; i++) { a.X.l[i] = w[i]; a.Y.l[i] = w[NL + i]; a.ZZ.l[i] = w[2 * NL + i]; a.ZZZ.l[i] = w[3 * NL + i]; }
  return a;
}

// unit u = (row u / chunks, chunk u % chunks).  out_jac (rows of one chunk): the row's result; else partials[u].
__global__ void __launch_bounds__(ROW_MSM_LANES) k_row_msm_ladder(const uint32_t* __restrict__ rows, uint32_t n_cols, const uint32_t* __restrict__ own, uint32_t n_own,
                                                                  uint64_t own_stride, const uint32_t* __restrict__ shared_pts, uint32_t chunks, uint32_t units,
                                                                  uint32_t* __restrict__ partials, uint32_t* __restrict__ out_jac) {
  __shared__ uint32_t xch[XW * TREE_SLOTS];
  const uint32_t lane = threadIdx.x;
#pragma unroll 1
  for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {        // units <= 2^31 and the grid <= 2^16: no wrap
    const uint32_t row = u / chunks, col = (u - row * chunks) * ROW_MSM_LANES + lane;
    xyzz acc = xyzz_identity();
    if (col < n_cols) {
      const uint32_t* scalar = rows + ((size_t)row * n_cols + col) * 8;
      // ONE ladder site: the point's array and index are selected, so own and shared columns of a wavefront run the same loop together
      const bool mine = col < n_own;
      acc = column_term(scalar, mine ? own : shared_pts, mine ? (size_t)row * own_stride + col : (size_t)(col - n_own));
    }
    acc = tree_sum(acc, xch, lane);
    if (lane == 0) {
      if (out_jac) store_jacobian(acc, out_jac + (size_t)row * 24);
      else store_partial(partials + (size_t)u * XW, acc);
    }
  }
}

__global__ void __launch_bounds__(ROW_MSM_LANES) k_row_msm_finish(const uint32_t* __restrict__ partials, uint32_t chunks, uint32_t n_rows, uint32_t* __restrict__ out_jac) {
  __shared__ uint32_t xch[XW * TREE_SLOTS];
  const uint32_t lane = threadIdx.x;
#pragma unroll 1
  for (uint32_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    xyzz acc = xyzz_identity();
#pragma unroll 1
    for (uint32_t c = lane; c < chunks; c += ROW_MSM_LANES) acc = xyzz_add(acc, load_partial(partials + ((size_t)row * chunks + c) * XW));
    acc = tree_sum(acc, xch, lane);
    if (lane == 0) store_jacobian(acc, out_jac + (size_t)row * 24);
  }
}

__global__ void __launch_bounds__(64) k_kzg_limbs_encode(const uint64_t* __restrict__ affine, uint32_t n, uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t pt[8], limbs[24];
  for (int j = 0; j < 8; j++) pt[j] = affine[(size_t)i * 8 + j];
  kzg_limbs::encode_point(pt, limbs);
  for (int j = 0; j < 24; j++) out[(size_t)i * 24 + j] = limbs[j];
}

__global__ void __launch_bounds__(64) k_kzg_limbs_decode(const uint64_t* __restrict__ in, uint32_t n, uint64_t* __restrict__ affine, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t pt[8], limbs[24];
  for (int j = 0; j < 24; j++) limbs[j] = in[(size_t)i * 24 + j];
  status[i] = kzg_limbs::decode_point(limbs, pt);
  for (int j = 0; j < 8; j++) affine[(size_t)i * 8 + j] = pt[j];
}

}  // namespace

size_t g1_row_msm_workspace(size_t n_rows, size_t n_cols) {
  row_msm_plan p;
  return row_msm_make_plan(n_rows, n_cols, &p) ? p.partial_bytes : 0;
}

// the arguments have passed row_msm_refusal (capi.hip)
int g1_row_msm_device(const uint32_t* d_rows, size_t n_cols, const uint32_t* d_own, size_t n_own, size_t own_stride, const uint32_t* d_shared, size_t n_rows,
                      uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream) {
  row_msm_plan p;
  if (!row_msm_make_plan(n_rows, n_cols, &p)) { set_error("g1_row_msm: bad shape"); return ZKHIP_EINVAL; }
  if (p.stages == 0) return ZKHIP_OK;
  if (ws_bytes < p.partial_bytes) { set_error("g1_row_msm: workspace too small"); return ZKHIP_EINVAL; }
  hipLaunchKernelGGL(k_row_msm_ladder, dim3(p.grid1), dim3(ROW_MSM_LANES), 0, stream, d_rows, (uint32_t)n_cols, d_own, (uint32_t)n_own, (uint64_t)own_stride, d_shared, p.chunks,
                     (uint32_t)p.units, (uint32_t*)ws, p.stages == 1 ? d_out : (uint32_t*)nullptr);
  if (p.stages == 2) hipLaunchKernelGGL(k_row_msm_finish, dim3(p.grid2), dim3(ROW_MSM_LANES), 0, stream, (const uint32_t*)ws, p.chunks, (uint32_t)n_rows, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int kzg_limbs_encode_device(const uint64_t* d_affine, size_t n, uint64_t* d_out, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_kzg_limbs_encode, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_affine, (uint32_t)n, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int kzg_limbs_decode_device(const uint64_t* d_in, size_t n, uint64_t* d_affine, uint32_t* d_status, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_kzg_limbs_decode, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_in, (uint32_t)n, d_affine, d_status);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

// Elementwise field / curve kernels behind the zkhip_test_* parity hooks:
// they expose the device arithmetic of fp29.hpp / ec.hpp in the external memory format so tests can diff it
// against the oracle.  Not used by the MSM / NTT paths themselves.
#include <hip/hip_runtime.h>
#include "ec_quad.hpp"
#include "ec2_quad.hpp"
#include "fe_lift.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

template <class P>
__global__ void __launch_bounds__(256) k_field_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wa[8], wb[8], wo[8];
  load_words(a + i * 8, wa);
  load_words(b + i * 8, wb);
  fe one = fe_one<P>();
  fe x = fe_mul<P>(one, fe_from_ext_lazy(wa));   // x * 2^261, reduced
  fe y = fe_mul<P>(one, fe_from_ext_lazy(wb));
  fe r;
  switch (op) {
    case 0: r = fe_mul<P>(x, y); break;
    case 1: r = fe_add(x, y); break;
    case 2: r = fe_sub_red(x, y, P::P3_S1); break;
    default: r = fe_sqr<P>(x); break;
  }
  fe_to_ext<P>(r, wo);
  store_words(out + i * 8, wo);
}

__global__ void __launch_bounds__(128) k_g1_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  affine_words pa = load_affine(a, i), pb = load_affine(b, i);
  xyzz acc = xyzz_identity();
  if (!affine_is_identity(pa)) xyzz_madd(acc, fe_from_ext_lazy(pa.x), fe_from_ext_lazy(pa.y));
  if (op == 1) {
    acc = xyzz_dbl(acc);
  } else if (!affine_is_identity(pb)) {
    fe y2 = fe_from_ext_lazy(pb.y);
    if (op == 2) y2 = fe_neg_red(y2, Fq::P64_S1);
    xyzz_madd(acc, fe_from_ext_lazy(pb.x), y2);
  }
  store_jacobian(acc, out + i * 24);
}

// ---- the shapes the MSM kernels instantiate (ops documented at zkhip_test_*_op in zkhip.h) -----------------------------------------------
// `op & 256`: every operand of the formula under test is first lifted to the largest representative below its documented bound
// (fe_lift.hpp), so the formula runs at the top of the operand range its call-site comments allow; the residues, and so the expected
// outputs, are those of the plain op.

// 4 = fe_mul<P, true>, 5 = fe_sqr<P, true> (the asm-block column chains of mac_blocks.hpp), 6 / 7 = fe_mul_add<P, false / true>:
// out[i] = a[i] b[i] + a[i ^ 1] b[i ^ 1] (n even)
template <class P>
__global__ void __launch_bounds__(256) k_field_op_shapes(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool lift = (op & 256) != 0;
  op &= 255;
  uint32_t wa[8], wb[8], wo[8];
  load_words(a + i * 8, wa);
  load_words(b + i * 8, wb);
  const fe one = fe_one<P>();
  fe x = fe_mul<P>(one, fe_from_ext_lazy(wa)), y = fe_mul<P>(one, fe_from_ext_lazy(wb));
  fe r;
  if (op == 4) {
    if (lift) { x = fe_lift<P>(x, 2); y = fe_lift_lazy<P>(y, 5); }                // N x limbs < 2^31.5
    r = fe_mul<P, true>(x, y);
  } else if (op == 5) {
    if (lift) x = fe_lift_lazy<P>(x, 2);                                          // limbs < 2^30.3
    r = fe_sqr<P, true>(x);
  } else {
    load_words(a + (i ^ 1) * 8, wa);
    load_words(b + (i ^ 1) * 8, wb);
    fe z = fe_mul<P>(one, fe_from_ext_lazy(wa)), w = fe_mul<P>(one, fe_from_ext_lazy(wb));
    if (lift) { x = fe_lift<P>(x, 2); z = fe_lift<P>(z, 2); y = fe_lift_lazy<P>(y, 3); w = fe_lift_lazy<P>(w, 2); }   // ec.hpp's Y3: R T + PPP (6p - Y1)
    r = op == 6 ? fe_mul_add<P, false>(x, y, z, w) : fe_mul_add<P, true>(x, y, z, w);
  }
  fe_to_ext<P>(r, wo);
  store_words(out + i * 8, wo);
}

// 5 = a[i] + b[i], 6 = a[i] - b[i] through xyzz_madd<true> twice (the bucket kernels' mixed addition: Y3 under one reduction)
__global__ void __launch_bounds__(128) k_g1_op_chain(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool lift = (op & 256) != 0;
  op &= 255;
  affine_words pa = load_affine(a, i), pb = load_affine(b, i);
  xyzz acc = xyzz_identity();
  if (!affine_is_identity(pa)) {
    fe x1 = fe_from_ext_lazy(pa.x), y1 = fe_from_ext_lazy(pa.y);
    if (lift) { x1 = fe_lift<Fq>(x1, 64); y1 = fe_lift<Fq>(y1, 64); }
    xyzz_madd<true>(acc, x1, y1);
  }
  if (lift) acc = xyzz_lift(acc);                                                 // X 9p, Y 5p, ZZ / ZZZ 2p
  if (!affine_is_identity(pb)) {
    fe x2 = fe_from_ext_lazy(pb.x), y2 = fe_from_ext_lazy(pb.y);
    if (op == 6) y2 = fe_neg_red(y2, Fq::P64_S1);
    if (lift) { x2 = fe_lift<Fq>(x2, 64); y2 = fe_lift<Fq>(y2, 64); }
    xyzz_madd<true>(acc, x2, y2);
  }
  store_jacobian(acc, out + i * 24);
}

ZK_D void affine2_coords_lazy(const affine2_words& p, fe2& x, fe2& y) {          // as k2_accumulate unpacks them: no multiplication, value < 32p
  uint32_t w[8];
  fe* f[4] = {&x.c0, &x.c1, &y.c0, &y.c1};
#pragma unroll
  for (int c = 0; c < 4; c++) {
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = p.w[8 * c + k];
    *f[c] = fe_from_ext_lazy(w);
  }
}

// G2, one thread per row.  7 = a + b, 8 = a - b through xyzz2_madd_lazy<true> twice and xyzz2_to_std; 9 = 2a + b through
// xyzz2_add_lazy<true>; 10 = the same sum with both operands in the 288-byte work format (rows 2i, 2i + 1 of `work`): even rows through
// xyzz2_add_lazy_mem<true>, odd rows through xyzz2_add_lazy_regmem<true>; 11 = xyzz2_add_lazy<true>(2a, 2a): xyzz2_dbl_lazy_core
__global__ void __launch_bounds__(64) k2_formula_op(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                                                    uint32_t* __restrict__ work, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool lift = (op & 256) != 0;
  op &= 255;
  const affine2_words pa = load_affine2(a, i), pb = load_affine2(b, i);
  fe2 x, y;
  xyzz2 r;
  if (op <= 8) {
    r = xyzz2_identity();
    if (!affine2_is_identity(pa)) {
      affine2_coords_lazy(pa, x, y);
      if (lift) { x = f2_lift(x, 32); y = f2_lift(y, 32); }
      xyzz2_madd_lazy<true>(r, x, y, false);
    }
    if (lift) r = xyzz2_lift(r, 2, 5, 2);                                         // the accumulator invariant: X 2p, Y 5p, ZZ / ZZZ 2p
    if (!affine2_is_identity(pb)) {
      affine2_coords_lazy(pb, x, y);
      if (lift) { x = f2_lift(x, 32); y = f2_lift(y, 32); }
      xyzz2_madd_lazy<true>(r, x, y, op == 8);
    }
    r = xyzz2_to_std(r);
  } else {
    xyzz2 A = xyzz2_identity(), B = xyzz2_identity();
    if (!affine2_is_identity(pa)) { affine2_coords(pa, false, x, y); xyzz2_madd(A, x, y); A = xyzz2_dbl(A); }
    if (!affine2_is_identity(pb)) { affine2_coords(pb, false, x, y); xyzz2_madd(B, x, y); }
    if (lift) { A = xyzz2_lift(A, 2, 2, 2); B = xyzz2_lift(B, 2, 2, 2); }         // standard form: every component below 2p + 2^233
    if (op == 9) r = xyzz2_add_lazy<true>(A, B);
    else if (op == 11) r = xyzz2_add_lazy<true>(A, A);
    else {
      store_xyzz2(work, 2 * i, A);
      store_xyzz2(work, 2 * i + 1, B);
      r = (i & 1) ? xyzz2_add_lazy_regmem<true>(A, work, 2 * i + 1) : xyzz2_add_lazy_mem<true>(work, 2 * i, work, 2 * i + 1);
    }
  }
  store_jacobian2(r, out + i * 48);
}

// G2, four lanes per row: the lazy quad chains of the window fold (ops 5 = 4a + b, 6 = 16a of k2_test_op_quad) with the lazy quad point
// lifted to the top of ec2_quad.hpp's invariant between the links: X, Y 2p; ZZ, ZZZ components 5p; the stored operand b 2p
__global__ void __launch_bounds__(64) k2_formula_op_quad(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, size_t n) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = gid >> 2;
  const uint32_t q = (uint32_t)(gid & 3);
  if (i >= n) return;                                   // whole quads leave together
  op &= 255;
  const affine2_words pa = load_affine2(a, i), pb = load_affine2(b, i);
  xyzz2 A = xyzz2_identity(), B = xyzz2_identity();
  fe2 x, y;
  if (!affine2_is_identity(pa)) { affine2_coords(pa, false, x, y); xyzz2_madd(A, x, y); A = xyzz2_dbl(A); }
  if (!affine2_is_identity(pb)) { affine2_coords(pb, false, x, y); xyzz2_madd(B, x, y); }
  xyzz2 r = xyzz2_dbl_quad_lazy(xyzz2_lift(A, 2, 2, 5), q);
  if (op == 5) r = xyzz2_add_quad_lazy(xyzz2_lift(r, 2, 2, 5), xyzz2_lift(B, 2, 2, 2), q);
  else r = xyzz2_dbl_quad_lazy(xyzz2_lift(xyzz2_dbl_quad_lazy(xyzz2_lift(r, 2, 2, 5), q), 2, 2, 5), q);
  r = xyzz2_quad_to_std(xyzz2_lift(r, 2, 2, 5));
  if (q == 0) store_jacobian2(r, out + i * 48);
}

// quad-cooperative formulas (ec_quad.hpp), 4 lanes per element: op 3 = 2a + 2b, op 4 = 4a
__global__ void __launch_bounds__(128) k_g1_op_quad(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = gid >> 2;
  const uint32_t q = (uint32_t)gid & 3;
  if (i >= n) return;                                   // whole quads leave together
  affine_words pa = load_affine(a, i), pb = load_affine(b, i);
  xyzz A = xyzz_identity(), B = xyzz_identity();
  if (!affine_is_identity(pa)) xyzz_madd(A, fe_from_ext_lazy(pa.x), fe_from_ext_lazy(pa.y));
  if (!affine_is_identity(pb)) xyzz_madd(B, fe_from_ext_lazy(pb.x), fe_from_ext_lazy(pb.y));
  xyzz r;
  if (op == 3) r = xyzz_add_quad(xyzz_dbl_quad(A, q), xyzz_dbl_quad(B, q), q);
  else r = xyzz_dbl_quad(xyzz_dbl_quad(A, q), q);
  if (q == 0) store_jacobian(r, out + i * 24);
}

// `G1Affine::read_raw` check of halo2curves [DEP] (what `SerdeFormat::RawBytes` readers run on every point of an SRS or key file):
// both coordinates canonical Montgomery residues (< q) and (x, y) = (0, 0) or y^2 = x^3 + 3.  first_bad receives the smallest
// index that fails (stays n when every point passes).
__device__ __forceinline__ bool words_below_q(const uint32_t (&w)[8]) {
  const fe v = fe_unpack<0>(w);                   // the raw 256-bit integer as limbs
  bool lt = false, eq = true;
#pragma unroll
  for (int i = NL - 1; i >= 0; i--) {
    lt = lt || (eq && v.l[i] < Fq::P[i]);
    eq = eq && v.l[i] == Fq::P[i];
  }
  return lt;
}

__global__ void __launch_bounds__(256) k_g1_check(const uint32_t* __restrict__ pts, size_t n, unsigned long long* __restrict__ first_bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const affine_words p = load_affine(pts, i);
  if (affine_is_identity(p)) return;
  bool ok = words_below_q(p.x) && words_below_q(p.y);
  if (ok) {
    const fe one = fe_one<Fq>();
    const fe x = fe_mul<Fq>(one, fe_from_ext_lazy(p.x)), y = fe_mul<Fq>(one, fe_from_ext_lazy(p.y));   // internal form, < 2p
    const fe lhs = fe_sqr<Fq>(y);
    const fe x3 = fe_mul<Fq>(fe_sqr<Fq>(x), x);
    const fe three = fe_norm(fe_add(fe_add(one, one), one));                   // 3 in internal form, < 3p
    const fe rhs = fe_norm(fe_add(x3, three));                                 // < 5p, N form
    const fe diff = fe_mul<Fq>(one, fe_sub_red(lhs, rhs, Fq::P6_S1));          // same residue, < 2p
    ok = fe_mulout_is_zero<Fq>(diff);
  }
  if (!ok) atomicMin(first_bad, (unsigned long long)i);
}

int g1_check_points_device(const uint32_t* d_points, size_t n, unsigned long long* d_first_bad, hipStream_t stream) {
  const unsigned long long init = (unsigned long long)n;
  if (hipMemcpyAsync(d_first_bad, &init, 8, hipMemcpyHostToDevice, stream) != hipSuccess) { set_error("g1_check: upload failed"); return ZKHIP_EHIP; }
  if (hipStreamSynchronize(stream) != hipSuccess) return ZKHIP_EHIP;      // `init` is a stack variable
  if (n) hipLaunchKernelGGL(k_g1_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_points, n, d_first_bad);
  return hipGetLastError() == hipSuccess ? ZKHIP_OK : ZKHIP_EHIP;
}

int test_field_op(int field, int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, size_t n, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if ((op & 255) >= 4) {
    if (field == 0) hipLaunchKernelGGL(k_field_op_shapes<FqParams>, grid, block, 0, stream, op, d_a, d_b, d_out, n);
    else hipLaunchKernelGGL(k_field_op_shapes<FrParams>, grid, block, 0, stream, op, d_a, d_b, d_out, n);
  } else if (field == 0) hipLaunchKernelGGL(k_field_op<FqParams>, grid, block, 0, stream, op, d_a, d_b, d_out, n);
  else hipLaunchKernelGGL(k_field_op<FrParams>, grid, block, 0, stream, op, d_a, d_b, d_out, n);
  return hipGetLastError() == hipSuccess ? ZKHIP_OK : ZKHIP_EHIP;
}

int test_g1_op(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, size_t n, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  if ((op & 255) >= 5) hipLaunchKernelGGL(k_g1_op_chain, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, stream, op, d_a, d_b, d_out, n);
  else if (op >= 3) hipLaunchKernelGGL(k_g1_op_quad, dim3((unsigned)((4 * n + 127) / 128)), dim3(128), 0, stream, op, d_a, d_b, d_out, n);
  else hipLaunchKernelGGL(k_g1_op, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, stream, op, d_a, d_b, d_out, n);
  return hipGetLastError() == hipSuccess ? ZKHIP_OK : ZKHIP_EHIP;
}

// the G2 ops that run the bucket kernels' shapes (7 .. 11) and every lifted op (256 + 5 .. 256 + 11); d_work: 2 n work points (op 10)
int test_g2_formula_op(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, uint32_t* d_work, size_t n, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  if ((op & 255) <= 6) hipLaunchKernelGGL(k2_formula_op_quad, dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, stream, op, d_a, d_b, d_out, n);
  else hipLaunchKernelGGL(k2_formula_op, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, op, d_a, d_b, d_out, d_work, n);
  return hipGetLastError() == hipSuccess ? ZKHIP_OK : ZKHIP_EHIP;
}

}  // namespace zkhip

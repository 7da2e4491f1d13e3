// The pairing check kernel: is prod_i e(g1[i], g2[i]) the identity of Gt?  (include/zkhip.h, "pairing check"; the arithmetic is pairing.hpp)
//
// ONE workgroup of 256 threads, quad p (lanes 4p .. 4p + 3) owns pair p: it keeps its own f and T and runs the whole Miller loop with the quad
// policy, so that the 64 chains of ~4 k dependent Fq2 products run side by side and each product costs the latency of one Fq product.  All quads
// stay active through the loop: an idle slot (p >= n) or a pair with an identity runs the same instructions on zero words and ends with f = 1.
// The 64 Miller values then meet in LDS (108 words = 432 bytes each in internal form, 27 KiB) and are multiplied by a log-depth tree of quads;
// quad 0 runs the final exponentiation and lane 0 writes the verdict with an ordinary vector store.  The Gt value never leaves the kernel.
#include "zkhip_internal.hpp"
#include "pairing.hpp"

namespace zkhip {

constexpr int F12_WORDS = 12 * NL;       // 108

#define ZK_F12_MEMBERS(a) {&a.c0.c0.c0, &a.c0.c0.c1, &a.c0.c1.c0, &a.c0.c1.c1, &a.c0.c2.c0, &a.c0.c2.c1, \
                           &a.c1.c0.c0, &a.c1.c0.c1, &a.c1.c1.c0, &a.c1.c1.c1, &a.c1.c2.c0, &a.c1.c2.c1}

ZK_D void f12_to_lds(uint32_t* slot, const fe12& a) {
  const fe* f[12] = ZK_F12_MEMBERS(a);
#pragma unroll
  for (int k = 0; k < 12; k++)
#pragma unroll
    for (int i = 0; i < NL; i++) slot[NL * k + i] = f[k]->l[i];
}
ZK_D fe12 f12_from_lds(const uint32_t* slot) {
  fe12 a;
  fe* f[12] = ZK_F12_MEMBERS(a);
#pragma unroll
  for (int k = 0; k < 12; k++)
#pragma unroll
    for (int i = 0; i < NL; i++) f[k]->l[i] = slot[NL * k + i];
  return a;
}

__global__ __launch_bounds__(256) void k_pairing_check(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2, uint32_t n, uint32_t* __restrict__ ok) {
  __shared__ uint32_t lds[ZKHIP_MAX_PAIRS * F12_WORDS];
  const uint32_t p = threadIdx.x >> 2, q = threadIdx.x & 3;
  const f2_quad m{q};
  const bool idle = p >= n;                                  // uniform over the quad
  uint32_t w1[16], w2[32];
#pragma unroll
  for (int i = 0; i < 16; i++) w1[i] = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) w2[i] = 0;
  if (!idle) {                                               // p < n <= ZKHIP_MAX_PAIRS: inside the two arrays
    const uint4* a = reinterpret_cast<const uint4*>(g1 + (size_t)p * 16);
    const uint4* b = reinterpret_cast<const uint4*>(g2 + (size_t)p * 32);
#pragma unroll
    for (int i = 0; i < 4; i++) { const uint4 v = a[i]; w1[4 * i] = v.x; w1[4 * i + 1] = v.y; w1[4 * i + 2] = v.z; w1[4 * i + 3] = v.w; }
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint4 v = b[i]; w2[4 * i] = v.x; w2[4 * i + 1] = v.y; w2[4 * i + 2] = v.z; w2[4 * i + 3] = v.w; }
  }
  const fe12 f = miller_loop_words(w1, w2, idle, m);
  if (q == 0) f12_to_lds(lds + p * F12_WORDS, f);
  __syncthreads();
  // the product tree: quads below the stride multiply their value by the one a stride above (whole quads branch together)
  for (uint32_t stride = ZKHIP_MAX_PAIRS / 2; stride >= 1; stride >>= 1) {
    if (p < stride) {
      const fe12 r = f12_mul(f12_from_lds(lds + p * F12_WORDS), f12_from_lds(lds + (p + stride) * F12_WORDS), m);
      if (q == 0) f12_to_lds(lds + p * F12_WORDS, r);
    }
    __syncthreads();
  }
  if (p != 0) return;
  const bool one = f12_is_one(final_exponentiation(f12_from_lds(lds), m));
  if (q == 0) *ok = one ? 1u : 0u;
}

int pairing_check_device(const uint32_t* d_g1, const uint32_t* d_g2, size_t n, uint32_t* d_ok, hipStream_t stream) {
  hipLaunchKernelGGL(k_pairing_check, dim3(1), dim3(256), 0, stream, d_g1, d_g2, (uint32_t)n, d_ok);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// ---- test hook: one tower operation through either policy ---------------------------------------------------------------------------------
// (the operation reads and writes global memory directly; the four lanes of the quad store the same words)
__global__ __launch_bounds__(64) void k_fq12_op_quad(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const f2_quad m{threadIdx.x & 3};                          // launched with 4 threads: one quad, identical arguments
  pairing_test_op(op, a, b, out, m);
}
__global__ __launch_bounds__(64) void k_fq12_op_single(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const f2_single m;
  pairing_test_op(op, a, b, out, m);
}

int test_fq12_op(int op, int which, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, hipStream_t stream) {
  if (which & 1) {
    hipLaunchKernelGGL(k_fq12_op_quad, dim3(1), dim3(4), 0, stream, op, d_a, d_b, d_out);
    HIPCHK(hipGetLastError());
  }
  if (which & 2) {
    hipLaunchKernelGGL(k_fq12_op_single, dim3(1), dim3(1), 0, stream, op, d_a, d_b, d_out + 96);
    HIPCHK(hipGetLastError());
  }
  return ZKHIP_OK;
}

}  // namespace zkhip

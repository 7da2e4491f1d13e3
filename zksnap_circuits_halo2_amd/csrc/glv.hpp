// The GLV split of a BN254 scalar (device): k = k1 + lambda k2 mod r with |k1|, |k2| < 2^127, phi(x, y) = (beta x, y) = lambda (x, y).
// For the row MSM's joint ladder (row_msm.hip).  The namespace's body is, line for line, `namespace glv` of msm.hip, where the constants are
// derived, bounded and pinned (tests/test_oracle.py reads them from that file's text, so they stay there; tests/test_kzg_limbs_host.py fails when
// the two texts differ).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace zkhip {
namespace glv {
__device__ constexpr uint32_t G1[3] = {0xc7e0b3d7u, 0xd91d232eu, 0x2u};
__device__ constexpr uint32_t G2[5] = {0x391eb18eu, 0x7a7bd9d4u, 0xa773d2cfu, 0x4ccef014u, 0x2u};
__device__ constexpr uint32_t A1[2] = {0x94d213e3u, 0x89d32568u};                               // = b2
__device__ constexpr uint32_t A2[4] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u};
__device__ constexpr uint32_t NB1[4] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u};    // -b1
// beta (the cube root of unity in Fq with phi = lambda for this lambda), Montgomery-256 words
__device__ constexpr uint32_t BETA_EXT[8] = {0xd782e155u, 0x71930c11u, 0xffbe3323u, 0xa6bb947cu, 0xd4741444u, 0xaa303344u, 0x26594943u, 0x2c3b3f0du};

// out[0 .. NO) = low NO words of a (NA words) * b (NB words)
template <int NA, int NB, int NO>
__device__ __forceinline__ void mul_low(const uint32_t (&a)[NA], const uint32_t* __restrict__ b, uint32_t (&out)[NO]) {
#pragma unroll
  for (int i = 0; i < NO; i++) out[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      if (i + j < NO) {
        const uint64_t t = (uint64_t)a[i] * b[j] + out[i + j] + carry;
        out[i + j] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
      }
    }
    if (i + NB < NO) out[i + NB] = carry;      // (this word has not been written by an earlier row: rows ascend)
  }
}

// magnitude (4 words) and sign of a two's-complement 160-bit value whose magnitude is below 2^127
__device__ __forceinline__ bool abs160(uint32_t (&v)[5], uint32_t (&mag)[4]) {
  const bool neg = (v[4] >> 31) != 0;
  uint32_t carry = neg ? 1u : 0u;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t w = neg ? ~v[i] : v[i];
    const uint32_t t = w + carry;
    carry = (t < w) ? 1u : 0u;
    mag[i] = t;
  }
  return neg;
}

// k (canonical, 8 words) -> |k1|, sign(k1), |k2|, sign(k2)
__device__ __forceinline__ void decompose(const uint32_t (&k)[8], uint32_t (&m1)[4], bool& s1, uint32_t (&m2)[4], bool& s2) {
  uint32_t t1[11], t2[13];
  mul_low<8, 3, 11>(k, G1, t1);
  mul_low<8, 5, 13>(k, G2, t2);
  const uint32_t c1[2] = {t1[8], t1[9]};                           // < 2^64
  const uint32_t c2[4] = {t2[8], t2[9], t2[10], t2[11]};           // < 2^127
  uint32_t p[5], q[5], v[5];
  mul_low<2, 2, 5>(c1, A1, p);                                     // c1 a1 (< 2^128: exact in 5 words)
  mul_low<4, 4, 5>(c2, A2, q);                                     // c2 a2 mod 2^160
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {                                    // v = k - p - q mod 2^160
    const uint64_t d = (uint64_t)k[i] - p[i] - q[i] - borrow;
    v[i] = (uint32_t)d;
    borrow = (d >> 32) ? ((~(d >> 32) + 1) & 3) : 0;               // 0, 1 or 2 borrowed
  }
  s1 = abs160(v, m1);
  mul_low<2, 4, 5>(c1, NB1, p);                                    // c1 (-b1) mod 2^160
  mul_low<4, 2, 5>(c2, A1, q);                                     // c2 b2 (b2 = a1)
  borrow = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {                                    // v = p - q mod 2^160
    const uint64_t d = (uint64_t)p[i] - q[i] - borrow;
    v[i] = (uint32_t)d;
    borrow = (d >> 32) ? 1 : 0;
  }
  s2 = abs160(v, m2);
}
}  // namespace glv
}  // namespace zkhip

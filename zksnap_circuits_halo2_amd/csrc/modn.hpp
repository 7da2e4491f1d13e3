// Montgomery arithmetic modulo an odd N < 2^384 that is known only at run time: twelve 32-bit limbs, R = 2^384.
//
// The ring of the Paillier tally (paillier.hip): N = n^2 with n the caller's public key, 352 bits for the reference's ENC_BIT_LEN = 176 and up to
// 384.  fp29.hpp cannot express it: its modulus is a compile-time constant and its nine 29-bit limbs live on seven spare bits that a modulus
// just under 2^384 does not have.  So the limbs here are full words, every value between two calls is FULLY reduced (< N), and a product runs
// through a 13th carry word and one conditional subtraction.
//
// The context (modulus, -N^-1 mod 2^32, R mod N, R^2 mod N) is built on the host per call with shifts and subtractions and handed to a kernel BY
// VALUE: its limbs are kernel arguments, uniform over the wave, and every m * N[j] of the reduction multiplies a vector register by a scalar one
// (the `vs` shape of mac_blocks.hpp; the compiler picks it from the plain C below).
//
//   modn_mul(a, b)    a b R^-1 mod N, fully reduced, for ANY a < 2^384 and b < N (or a < N and any b): a b < R N, so the CIOS sum
//                     (a b + m N) / R is below 2 N and one subtraction reduces it.  Two unreduced operands are NOT allowed.
//   modn_to_mont(a)   modn_mul(a, R^2 mod N) = a R mod N: R^2 mod N is reduced, so a may be any 384-bit integer -- an input >= N is reduced the
//                     way `BigUint %` reduces it, and nothing has to refuse it.
//   modn_from_mont(a) modn_mul(a, 1).
//   modn_pow(b, e)    the plain left-to-right ladder over the bits of e, b in Montgomery form; e = 0 gives 1 for every b (0 included).
//
// Everything is host and device code and compiles with plain g++ (tests/cpp/modn_host_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MODN_HD __host__ __device__ __forceinline__
#else
#define MODN_HD inline
#endif

namespace zkhip {

constexpr int MODN_L = 12;             // limbs of a value: 384 bits

struct modn {
  uint32_t l[MODN_L];
};

struct modn_ctx {
  uint32_t n[MODN_L];                  // the modulus N, odd, >= 3
  uint32_t one[MODN_L];                // R mod N: 1 in Montgomery form
  uint32_t r2[MODN_L];                 // R^2 mod N
  uint32_t ninv;                       // -N^-1 mod 2^32
};

MODN_HD modn modn_zero() {
  modn r;
#pragma unroll
  for (int i = 0; i < MODN_L; i++) r.l[i] = 0;
  return r;
}

MODN_HD modn modn_one(const modn_ctx& c) {
  modn r;
#pragma unroll
  for (int i = 0; i < MODN_L; i++) r.l[i] = c.one[i];
  return r;
}

// six little-endian 64-bit words <-> twelve limbs
MODN_HD modn modn_from_words(const uint64_t* w, int words = 6) {
  modn r = modn_zero();
#pragma unroll
  for (int i = 0; i < 6; i++) {
    if (i < words) {
      r.l[2 * i] = (uint32_t)w[i];
      r.l[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
  }
  return r;
}
MODN_HD void modn_to_words(const modn& a, uint64_t* w) {
#pragma unroll
  for (int i = 0; i < 6; i++) w[i] = (uint64_t)a.l[2 * i] | ((uint64_t)a.l[2 * i + 1] << 32);
}

// a b R^-1 mod N (CIOS, Koc-Acar-Kaliski 1996): one of the factors < N, the other < 2^384; the result < N
MODN_HD modn modn_mul(const modn& a, const modn& b, const modn_ctx& c) {
  uint32_t t[MODN_L + 2];
#pragma unroll
  for (int i = 0; i < MODN_L + 2; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < MODN_L; i++) {
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < MODN_L; j++) {
      acc += (uint64_t)a.l[j] * b.l[i] + t[j];               // < 2^64: (2^32 - 1)^2 + 2 (2^32 - 1)
      t[j] = (uint32_t)acc;
      acc >>= 32;
    }
    acc += t[MODN_L];
    t[MODN_L] = (uint32_t)acc;
    t[MODN_L + 1] = (uint32_t)(acc >> 32);
    const uint32_t m = t[0] * c.ninv;
    acc = ((uint64_t)m * c.n[0] + t[0]) >> 32;                // the low word is 0 by the choice of m
#pragma unroll
    for (int j = 1; j < MODN_L; j++) {
      acc += (uint64_t)m * c.n[j] + t[j];
      t[j - 1] = (uint32_t)acc;
      acc >>= 32;
    }
    acc += t[MODN_L];
    t[MODN_L - 1] = (uint32_t)acc;
    t[MODN_L] = t[MODN_L + 1] + (uint32_t)(acc >> 32);        // the sum stays below 2 N < 2^385: this word is 0 or 1
  }
  // t (13 words) < 2 N: subtract N once when t >= N
  modn d;
  uint64_t borrow = 0;
#pragma unroll
  for (int j = 0; j < MODN_L; j++) {
    const uint64_t s = (uint64_t)t[j] - c.n[j] - borrow;
    d.l[j] = (uint32_t)s;
    borrow = (s >> 32) & 1;
  }
  const bool take = t[MODN_L] != 0 || borrow == 0;           // the carry word set, or no borrow out of the 12 words: t >= N
  modn r;
#pragma unroll
  for (int j = 0; j < MODN_L; j++) r.l[j] = take ? d.l[j] : t[j];
  return r;
}

MODN_HD modn modn_to_mont(const modn& a, const modn_ctx& c) {
  modn r2;
#pragma unroll
  for (int i = 0; i < MODN_L; i++) r2.l[i] = c.r2[i];
  return modn_mul(a, r2, c);
}

MODN_HD modn modn_from_mont(const modn& a, const modn_ctx& c) {
  modn one = modn_zero();
  one.l[0] = 1;
  return modn_mul(a, one, c);
}

// base^e, base in Montgomery form (< N), e = `words` little-endian 32-bit words; the result in Montgomery form
MODN_HD modn modn_pow(const modn& base, const uint32_t* e, int words, const modn_ctx& c) {
  modn acc = modn_one(c);
  for (int w = words - 1; w >= 0; w--) {
    uint32_t bits = e[w];                                     // one read per 32 steps: e may be global memory or a kernel argument
    for (int i = 0; i < 32; i++, bits <<= 1) {
      acc = modn_mul(acc, acc, c);
      if (bits >> 31) acc = modn_mul(acc, base, c);
    }
  }
  return acc;
}

// ---- host: the context of a modulus ------------------------------------------------------------------------------------------------
// 2 x mod N for x < N (a 13th bit kept across the shift)
inline void modn_double_mod(uint32_t x[MODN_L], const uint32_t n[MODN_L]) {
  uint32_t top = 0;
  for (int j = 0; j < MODN_L; j++) {
    const uint32_t next = x[j] >> 31;
    x[j] = (x[j] << 1) | top;
    top = next;
  }
  uint32_t d[MODN_L];
  uint64_t borrow = 0;
  for (int j = 0; j < MODN_L; j++) {
    const uint64_t s = (uint64_t)x[j] - n[j] - borrow;
    d[j] = (uint32_t)s;
    borrow = (s >> 32) & 1;
  }
  if (top || !borrow)
    for (int j = 0; j < MODN_L; j++) x[j] = d[j];
}

// false (nothing written) for an even N or N < 3
inline bool modn_ctx_build(const uint32_t n[MODN_L], modn_ctx* out) {
  bool high = false;
  for (int j = 1; j < MODN_L; j++) high |= n[j] != 0;
  if (!(n[0] & 1) || (!high && n[0] < 3)) return false;
  for (int j = 0; j < MODN_L; j++) out->n[j] = n[j];
  uint32_t inv = n[0];                                        // Newton: correct to 3, 6, 12, 24, 48 bits
  for (int i = 0; i < 4; i++) inv *= 2u - n[0] * inv;
  out->ninv = 0u - inv;
  uint32_t x[MODN_L] = {1};                                   // 1 < N; 384 doublings: R mod N; 384 more: R^2 mod N
  for (int i = 0; i < 32 * MODN_L; i++) modn_double_mod(x, n);
  for (int j = 0; j < MODN_L; j++) out->one[j] = x[j];
  for (int i = 0; i < 32 * MODN_L; i++) modn_double_mod(x, n);
  for (int j = 0; j < MODN_L; j++) out->r2[j] = x[j];
  return true;
}

// n (`words` 64-bit words, at most 3) squared, schoolbook: the modulus of a Paillier key
inline void modn_square_words(const uint64_t* n, int words, uint32_t out[MODN_L]) {
  uint32_t a[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < words && i < 3; i++) {
    a[2 * i] = (uint32_t)n[i];
    a[2 * i + 1] = (uint32_t)(n[i] >> 32);
  }
  for (int j = 0; j < MODN_L; j++) out[j] = 0;
  for (int i = 0; i < 6; i++) {
    uint64_t carry = 0;
    for (int j = 0; j < 6; j++) {
      const uint64_t s = (uint64_t)a[i] * a[j] + out[i + j] + carry;
      out[i + j] = (uint32_t)s;
      carry = s >> 32;
    }
    for (int k = i + 6; carry && k < MODN_L; k++) {
      const uint64_t s = (uint64_t)out[k] + carry;
      out[k] = (uint32_t)s;
      carry = s >> 32;
    }
  }
}

}  // namespace zkhip

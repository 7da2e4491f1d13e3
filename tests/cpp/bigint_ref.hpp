// The independent big-integer reference shared by the host checks of the device arithmetic (fp29_host_check.cpp, ec2_host_check.cpp):
// schoolbook 320-bit integers, a 4 x 64-bit Montgomery (CIOS) modular product -- a different radix and algorithm from the code under
// test -- the conversions between that world and the radix-2^29 limb vectors of csrc/fp29.hpp, a SplitMix64 generator and the CHECK macro.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ec.hpp"

using namespace zkhip;
typedef unsigned __int128 u128;

// ---- tiny big-int reference: 320-bit little-endian numbers in 5 x u64 ---------------------------------------------
struct big { uint64_t w[5]; };
static big big_zero() { big r; memset(&r, 0, sizeof(r)); return r; }
static big big_small(uint64_t v) { big r = big_zero(); r.w[0] = v; return r; }
static int big_cmp(const big& a, const big& b) { for (int i = 4; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i] ? 1 : -1; return 0; }
static big big_sub(const big& a, const big& b) { big r; uint64_t br = 0; for (int i = 0; i < 5; i++) { u128 d = (u128)a.w[i] - b.w[i] - br; r.w[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1; } return r; }
static big big_add(const big& a, const big& b) { big r; uint64_t c = 0; for (int i = 0; i < 5; i++) { u128 s = (u128)a.w[i] + b.w[i] + c; r.w[i] = (uint64_t)s; c = (uint64_t)(s >> 64); } return r; }
static big big_shl1(const big& a) { big r; uint64_t c = 0; for (int i = 0; i < 5; i++) { r.w[i] = (a.w[i] << 1) | c; c = a.w[i] >> 63; } return r; }
static big big_mod(big a, const big& p) { while (big_cmp(a, p) >= 0) a = big_sub(a, p); return a; }
// a * b mod p for a, b < p < 2^255, odd p: 4 x 64-bit Montgomery (CIOS) with R = 2^256, then one more Montgomery multiply by
// R^2 to leave the Montgomery domain -- a different radix and algorithm from the code under test.
static uint64_t neg_inv64(uint64_t p0) { uint64_t x = 1; for (int i = 0; i < 6; i++) x *= 2 - p0 * x; return (uint64_t)0 - x; }
static big mont4(const big& a, const big& b, const big& p, uint64_t inv) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    uint64_t carry = 0;
    for (int j = 0; j < 4; j++) { u128 s = (u128)a.w[j] * b.w[i] + t[j] + carry; t[j] = (uint64_t)s; carry = (uint64_t)(s >> 64); }
    u128 s = (u128)t[4] + carry; t[4] = (uint64_t)s; t[5] = (uint64_t)(s >> 64);
    const uint64_t m = t[0] * inv;
    s = (u128)m * p.w[0] + t[0]; carry = (uint64_t)(s >> 64);
    for (int j = 1; j < 4; j++) { s = (u128)m * p.w[j] + t[j] + carry; t[j - 1] = (uint64_t)s; carry = (uint64_t)(s >> 64); }
    s = (u128)t[4] + carry; t[3] = (uint64_t)s; t[4] = t[5] + (uint64_t)(s >> 64);
  }
  big r = big_zero();
  for (int i = 0; i < 5; i++) r.w[i] = t[i];
  return big_mod(r, p);
}
static big r2_for(const big& p) {   // 2^512 mod p by repeated doubling (once per modulus)
  big r = big_zero(); r.w[0] = 1;
  for (int i = 0; i < 512; i++) r = big_mod(big_shl1(r), p);
  return r;
}
static big mulmod(const big& a, const big& b, const big& p) {
  static big cached_p = big_zero(), cached_r2 = big_zero();
  static uint64_t cached_inv = 0;
  if (big_cmp(cached_p, p) != 0) { cached_p = p; cached_r2 = r2_for(p); cached_inv = neg_inv64(p.w[0]); }
  return mont4(mont4(a, b, p, cached_inv), cached_r2, p, cached_inv);   // (ab/R) * R^2 / R = ab
}
static big addmod(const big& a, const big& b, const big& p) { return big_mod(big_add(a, b), p); }
static big submod(const big& a, const big& b, const big& p) { return big_cmp(a, b) >= 0 ? big_sub(a, b) : big_sub(big_add(a, p), b); }
static big powmod(big a, const big& e, const big& p) { big r = big_zero(); r.w[0] = 1; for (int i = 0; i < 256; i++) { if ((e.w[i >> 6] >> (i & 63)) & 1) r = mulmod(r, a, p); a = mulmod(a, a, p); } return r; }
static big invmod(const big& a, const big& p) { big e = p; big two = big_zero(); two.w[0] = 2; e = big_sub(e, two); return powmod(a, e, p); }

template <class P> static big modulus() { big p = big_zero(); for (int i = 0; i < NL; i++) { int bit = LB * i; p.w[bit >> 6] |= (uint64_t)P::P[i] << (bit & 63); if ((bit & 63) + LB > 64 && (bit >> 6) + 1 < 5) p.w[(bit >> 6) + 1] |= (uint64_t)P::P[i] >> (64 - (bit & 63)); } return p; }
static big fe_value(const fe& a) {   // integer value of a (possibly unnormalised) limb vector
  big r = big_zero();
  for (int i = 0; i < NL; i++) { big t = big_zero(); int bit = LB * i; t.w[bit >> 6] = (uint64_t)a.l[i] << (bit & 63); if ((bit & 63) + 32 > 64) t.w[(bit >> 6) + 1] = (uint64_t)a.l[i] >> (64 - (bit & 63)); r = big_add(r, t); }
  return r;
}
static fe fe_from_big(const big& v) { fe r; for (int i = 0; i < NL; i++) { int bit = LB * i; uint64_t x = v.w[bit >> 6] >> (bit & 63); if ((bit & 63) + LB > 64) x |= v.w[(bit >> 6) + 1] << (64 - (bit & 63)); r.l[i] = (uint32_t)x & LMASK; } return r; }

static uint64_t rng_state = 0x5A4B534E41500009ULL;
static uint64_t rnd() { rng_state += 0x9E3779B97F4A7C15ULL; uint64_t z = rng_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
static big rnd_below(const big& p) { big r; for (int i = 0; i < 4; i++) r.w[i] = rnd(); r.w[4] = 0; r.w[3] &= (1ULL << 62) - 1; return big_mod(r, p); }

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { if (fails < 20) printf("FAIL %s (line %d)\n", msg, __LINE__); fails++; } } while (0)

template <class P> static big R261() { big r = big_zero(); r.w[4] = 1ULL << (261 - 256); return big_mod(r, modulus<P>()); }
template <class P> static big to_int(const fe& a, const big& rinv) { return mulmod(big_mod(fe_value(a), modulus<P>()), rinv, modulus<P>()); }   // Montgomery-261 -> plain
template <class P> static fe to_fe(const big& x) { return fe_from_big(mulmod(x, R261<P>(), modulus<P>())); }                                  // plain -> Montgomery-261, canonical

static bool is_N(const fe& a) { for (int i = 0; i < NL - 1; i++) if (a.l[i] > LMASK) return false; return true; }
static big big_times(const big& p, unsigned k) { big kp = big_zero(); for (unsigned i = 0; i < k; i++) kp = big_add(kp, p); return kp; }
static bool below(const fe& a, unsigned k, const big& p) { return big_cmp(fe_value(a), big_times(p, k)) < 0; }

// ---- 640-bit integers for the exact magnitude bounds: out * 2^261 < a b + c d + p 2^261, and value * den < p * num ----------------
struct wide { uint64_t w[10]; };
static wide wide_zero() { wide r; memset(&r, 0, sizeof(r)); return r; }
static wide wide_mul(const big& a, const big& b) {
  wide r = wide_zero();
  for (int i = 0; i < 5; i++) {
    uint64_t carry = 0;
    for (int j = 0; j < 5; j++) { u128 s = (u128)a.w[i] * b.w[j] + r.w[i + j] + carry; r.w[i + j] = (uint64_t)s; carry = (uint64_t)(s >> 64); }
    r.w[i + 5] = carry;
  }
  return r;
}
static wide wide_add(const wide& a, const wide& b) { wide r; uint64_t c = 0; for (int i = 0; i < 10; i++) { u128 s = (u128)a.w[i] + b.w[i] + c; r.w[i] = (uint64_t)s; c = (uint64_t)(s >> 64); } return r; }
static int wide_cmp(const wide& a, const wide& b) { for (int i = 9; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i] ? 1 : -1; return 0; }
static wide wide_shl261(const big& a) { big s = big_zero(); s.w[4] = 1ULL << (261 - 256); return wide_mul(a, s); }
// is the integer value of `a` below (num / den) p ?
static bool below_frac(const fe& a, uint64_t num, uint64_t den, const big& p) { return wide_cmp(wide_mul(fe_value(a), big_small(den)), wide_mul(p, big_small(num))) < 0; }
// the output bound of fe_mul / fe_sqr / fe_mul_add (fp29.hpp): N form and out < p ((a b + c d) / (p 2^261) + 1), on the operands' INTEGER values
static bool mulout_ok(const fe& out, const fe& a, const fe& b, const fe* c, const fe* d, const big& p) {
  wide rhs = wide_add(wide_mul(fe_value(a), fe_value(b)), wide_shl261(p));
  if (c) rhs = wide_add(rhs, wide_mul(fe_value(*c), fe_value(*d)));
  return is_N(out) && wide_cmp(wide_shl261(fe_value(out)), rhs) < 0;
}

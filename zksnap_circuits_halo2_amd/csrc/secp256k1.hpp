// secp256k1: the field mod p = 2^256 - 2^32 - 977 and the group y^2 = x^3 + 7 of order n, for the PLUME check (plume.hip).
//
// fp29.hpp is not the vehicle: its point formulas live on the seven spare bits that nine 29-bit limbs leave above BN254's p, and a 256-bit p
// leaves five.  The field here uses the special form of p instead, with no Montgomery form: eight full 32-bit limbs, a 512-bit product whose
// high half folds into the low one with 2^256 = 2^32 + 977 (mod p), twice, and one conditional subtraction.
//
// REDUCTION DISCIPLINE.  Every value a function returns is CANONICAL (< p), and external values are canonical integers.
//   sk_mul / sk_sqr / sk_mul_small / sk_reduce      take ANY 256-bit operands (p, p + 1, 2^256 - 1 included) and return the canonical result
//   sk_add / sk_sub / sk_neg                        need canonical operands: a + b < 2 p is reduced by one subtraction, a - b by one addition
//   sk_eq / sk_is_zero / sk_is_odd                  compare limbs, so they need canonical operands too
//   sk_inv = a^(p - 2) (0 -> 0), sk_sqrt = a^((p + 1) / 4) (a root iff its square is a): fixed addition chains, 255 squarings and 15 / 13 products
//   sk_scalar_*                                     the same discipline mod the group order n = 2^256 - delta_n, delta_n =
//                                                   0x14551231950B75FC4402DA1732FC9BEBF (129 bits, 1.271 * 2^128): ANY 256-bit operands (a 512-bit one
//                                                   for sk_scalar_reduce512), canonical results (< n).  A value T = lo + hi * 2^256 becomes
//                                                   lo + hi * delta_n, and the bound of every fold is:
//       (1) T < 2^512:         hi <= 2^256 - 1,   T1 = lo + hi delta_n < 2^256 + (2^256 - 1) delta_n < (delta_n + 1) 2^256: thirteen words, hi1 <= delta_n
//       (2) T1:                hi1 <= delta_n,    T2 = lo1 + hi1 delta_n < 2^256 + delta_n^2 < 2.62 * 2^256: nine words, hi2 <= 2
//       (3) T2 (sk_scalar_fold, c < 2^32):        T3 = lo2 + c delta_n < 2^256 + 2^161: the carry is 0 or 1
//       (4) a carry of 1 leaves words < 2^161:    T4 = lo3 + delta_n does not wrap; T4 < 2^256 < 2 n, so one conditional subtraction finishes
//                                                   sk_scalar_add's carry (0 or 1) and sk_scalar_from_digest (no carry) enter at (3); sk_scalar_muladd
//                                                   forms a b + c <= (2^256 - 1)^2 + 2^256 - 1 < 2^512 and enters at (1).
//
// THE GROUP.  Points are projective (X : Y : Z), x = X / Z, y = Y / Z, the identity (0 : 1 : 0).  Addition and doubling are the complete formulas
// for a = 0 of Renes, Costello and Batina (2016), algorithms 7 and 9 with b3 = 21: no branches, correct for P + P, P + (-P), the identity on
// either side and any representative of a point -- the inputs of the PLUME check are a stranger's.  Outside, the identity is the affine pair
// (0, 0): sk_to_affine gives it without a test, because Z = 0 inverts to 0.
//
// sk_lincomb(a, P, b, Q) = a P + b Q by one interleaved ladder (Strauss-Shamir) over the joint table {P, Q, P + Q}: 256 doublings and 256
// additions, the entry chosen by conditional moves (an array indexed at run time would go to scratch) and the identity added where both bits
// are zero.  The scalars are ANY 256-bit integers: the group has prime order n, so a counts mod n and n P is the identity.  sk_mul_proj(k, P) is
// the same ladder over the table {P}, for the signer (plume_sign.hip).  The ladders are branch-free, but nothing here is audited for side
// channels: the signing call is meant for generated populations (tests, probes, simulations), not for a voter's wallet.
//
// Everything is host and device code and compiles with plain g++ (tests/cpp/secp256k1_host_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SK_HD __host__ __device__ __forceinline__
#else
#define SK_HD inline
#endif

namespace zkhip {

struct sk_fe {
  uint32_t l[8];                       // little-endian limbs
};
struct sk_aff {                        // affine, (0, 0) the identity
  sk_fe x, y;
};
struct sk_pt {                         // projective
  sk_fe X, Y, Z;
};

// the four 64-bit words of a constant, most significant first, as it is written
SK_HD sk_fe sk_const(uint64_t w3, uint64_t w2, uint64_t w1, uint64_t w0) {
  sk_fe r;
  r.l[0] = (uint32_t)w0; r.l[1] = (uint32_t)(w0 >> 32);
  r.l[2] = (uint32_t)w1; r.l[3] = (uint32_t)(w1 >> 32);
  r.l[4] = (uint32_t)w2; r.l[5] = (uint32_t)(w2 >> 32);
  r.l[6] = (uint32_t)w3; r.l[7] = (uint32_t)(w3 >> 32);
  return r;
}
SK_HD sk_fe sk_small(uint32_t v) { return sk_const(0, 0, 0, v); }
SK_HD sk_fe sk_order() { return sk_const(0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFEull, 0xBAAEDCE6AF48A03Bull, 0xBFD25E8CD0364141ull); }
SK_HD sk_aff sk_generator() {
  sk_aff g;
  g.x = sk_const(0x79BE667EF9DCBBACull, 0x55A06295CE870B07ull, 0x029BFCDB2DCE28D9ull, 0x59F2815B16F81798ull);
  g.y = sk_const(0x483ADA7726A3C465ull, 0x5DA4FBFC0E1108A8ull, 0xFD17B448A6855419ull, 0x9C47D08FFB10D4B8ull);
  return g;
}

// four little-endian 64-bit words <-> eight limbs
SK_HD sk_fe sk_from_words(const uint64_t* w) {
  sk_fe r;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    r.l[2 * i] = (uint32_t)w[i];
    r.l[2 * i + 1] = (uint32_t)(w[i] >> 32);
  }
  return r;
}
SK_HD void sk_to_words(const sk_fe& a, uint64_t* w) {
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = (uint64_t)a.l[2 * i] | ((uint64_t)a.l[2 * i + 1] << 32);
}

SK_HD sk_fe sk_sel(bool c, const sk_fe& a, const sk_fe& b) {      // c ? a : b, limb by limb
  sk_fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
SK_HD bool sk_is_zero(const sk_fe& a) {
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) v |= a.l[i];
  return v == 0;
}
SK_HD bool sk_eq(const sk_fe& a, const sk_fe& b) {
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) v |= a.l[i] ^ b.l[i];
  return v == 0;
}
SK_HD bool sk_is_odd(const sk_fe& a) { return a.l[0] & 1u; }
// a < b as 256-bit integers (any values): the borrow of a - b
SK_HD bool sk_less(const sk_fe& a, const sk_fe& b) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) borrow = ((uint64_t)a.l[i] - b.l[i] - borrow) >> 63;
  return borrow != 0;
}

// r + delta with delta = 2^256 - p = 2^32 + 977; the carry out of 2^256 is returned.  r - p = r + delta - 2^256: the carry says r >= p.
SK_HD uint32_t sk_add_delta(const sk_fe& a, sk_fe& out) {
  uint64_t acc = (uint64_t)a.l[0] + 977u;
  out.l[0] = (uint32_t)acc;
  acc = (acc >> 32) + a.l[1] + 1u;
  out.l[1] = (uint32_t)acc;
#pragma unroll
  for (int i = 2; i < 8; i++) {
    acc = (acc >> 32) + a.l[i];
    out.l[i] = (uint32_t)acc;
  }
  return (uint32_t)(acc >> 32);
}
// any 256-bit a -> a mod p (a < 2^256 < 2 p: one subtraction)
SK_HD sk_fe sk_reduce(const sk_fe& a) {
  sk_fe t;
  const uint32_t ge = sk_add_delta(a, t);
  return sk_sel(ge != 0, t, a);
}
SK_HD bool sk_is_canonical(const sk_fe& a) {
  sk_fe t;
  return sk_add_delta(a, t) == 0;
}

SK_HD sk_fe sk_add(const sk_fe& a, const sk_fe& b) {
  sk_fe s, t;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    acc = (acc >> 32) + a.l[i] + b.l[i];
    s.l[i] = (uint32_t)acc;
  }
  const uint32_t over = (uint32_t)(acc >> 32);                // a + b >= 2^256 > p: the low words plus delta are a + b - p, and do not wrap again
  const uint32_t ge = sk_add_delta(s, t);
  return sk_sel((over | ge) != 0, t, s);
}
SK_HD sk_fe sk_sub(const sk_fe& a, const sk_fe& b) {
  sk_fe d, t;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    acc = (uint64_t)a.l[i] - b.l[i] - (acc >> 63);
    d.l[i] = (uint32_t)acc;
  }
  const bool under = (acc >> 63) != 0;                        // a < b: the words hold a - b + 2^256, and a - b + p = that minus delta
  acc = (uint64_t)d.l[0] - 977u;
  t.l[0] = (uint32_t)acc;
  acc = (uint64_t)d.l[1] - 1u - (acc >> 63);
  t.l[1] = (uint32_t)acc;
#pragma unroll
  for (int i = 2; i < 8; i++) {
    acc = (uint64_t)d.l[i] - (acc >> 63);
    t.l[i] = (uint32_t)acc;
  }
  return sk_sel(under, t, d);
}
SK_HD sk_fe sk_neg(const sk_fe& a) { return sk_sub(sk_small(0), a); }

// r (eight words) + c * 2^256 with c < 2^33 -> canonical: c * 2^256 = c * delta (mod p) < 2^66 is added, a second wrap adds delta once more (the
// words are then below 2^66 and cannot wrap again), and one subtraction finishes
SK_HD sk_fe sk_fold(const sk_fe& r, uint64_t c) {
  sk_fe o;
  const uint64_t k = c * 977u;                                // < 2^43
  uint64_t acc = (uint64_t)r.l[0] + (uint32_t)k;
  o.l[0] = (uint32_t)acc;
  acc = (acc >> 32) + r.l[1] + (k >> 32) + (uint32_t)c;
  o.l[1] = (uint32_t)acc;
  acc = (acc >> 32) + r.l[2] + (c >> 32);
  o.l[2] = (uint32_t)acc;
#pragma unroll
  for (int i = 3; i < 8; i++) {
    acc = (acc >> 32) + r.l[i];
    o.l[i] = (uint32_t)acc;
  }
  const uint32_t wrap = (uint32_t)(acc >> 32);                // 0 or 1
  acc = (uint64_t)o.l[0] + 977u * wrap;
  o.l[0] = (uint32_t)acc;
  acc = (acc >> 32) + o.l[1] + wrap;
  o.l[1] = (uint32_t)acc;
#pragma unroll
  for (int i = 2; i < 8; i++) {
    acc = (acc >> 32) + o.l[i];
    o.l[i] = (uint32_t)acc;
  }
  return sk_reduce(o);
}
// sixteen little-endian words -> the value mod p: lo + hi * 977 + (hi << 32), the carry folded by sk_fold
SK_HD sk_fe sk_reduce512(const uint32_t* t) {
  sk_fe r;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    acc = (acc >> 32) + t[i] + (uint64_t)t[8 + i] * 977u + (i ? t[7 + i] : 0u);
    r.l[i] = (uint32_t)acc;
  }
  return sk_fold(r, (acc >> 32) + t[15]);                     // < 2^11 + 2^32
}
SK_HD sk_fe sk_mul(const sk_fe& a, const sk_fe& b) {
  uint32_t t[16];
#pragma unroll
  for (int i = 0; i < 16; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t acc = (uint64_t)a.l[i] * b.l[j] + t[i + j] + carry;   // <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
      t[i + j] = (uint32_t)acc;
      carry = acc >> 32;
    }
    t[i + 8] = (uint32_t)carry;
  }
  return sk_reduce512(t);
}
SK_HD sk_fe sk_sqr(const sk_fe& a) { return sk_mul(a, a); }
SK_HD sk_fe sk_mul_small(const sk_fe& a, uint32_t k) {
  sk_fe r;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    acc = (acc >> 32) + (uint64_t)a.l[i] * k;
    r.l[i] = (uint32_t)acc;
  }
  return sk_fold(r, acc >> 32);
}
SK_HD sk_fe sk_sqrn(sk_fe a, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < n; i++) a = sk_sqr(a);
  return a;
}

// a^(2^223 - 1) and the shorter runs of ones the two exponents share: p = 2^256 - 2^32 - 977 is 223 ones, a zero, 22 ones and ten low bits
struct sk_runs {
  sk_fe x2, x22, x223;
};
SK_HD sk_runs sk_pow_runs(const sk_fe& a) {
  sk_runs r;
  r.x2 = sk_mul(sk_sqr(a), a);
  const sk_fe x3 = sk_mul(sk_sqr(r.x2), a);
  const sk_fe x6 = sk_mul(sk_sqrn(x3, 3), x3);
  const sk_fe x9 = sk_mul(sk_sqrn(x6, 3), x3);
  const sk_fe x11 = sk_mul(sk_sqrn(x9, 2), r.x2);
  r.x22 = sk_mul(sk_sqrn(x11, 11), x11);
  const sk_fe x44 = sk_mul(sk_sqrn(r.x22, 22), r.x22);
  const sk_fe x88 = sk_mul(sk_sqrn(x44, 44), x44);
  const sk_fe x176 = sk_mul(sk_sqrn(x88, 88), x88);
  const sk_fe x220 = sk_mul(sk_sqrn(x176, 44), x44);
  r.x223 = sk_mul(sk_sqrn(x220, 3), x3);
  return r;
}
// a^(p - 2): the low 32 bits of p - 2 are 22 ones, 0000 1 0 11 0 1
SK_HD sk_fe sk_inv(const sk_fe& a) {
  const sk_runs r = sk_pow_runs(a);
  sk_fe t = sk_mul(sk_sqrn(r.x223, 23), r.x22);
  t = sk_mul(sk_sqrn(t, 5), a);
  t = sk_mul(sk_sqrn(t, 3), r.x2);
  return sk_mul(sk_sqrn(t, 2), a);
}
// a^((p + 1) / 4): the low 30 bits of the exponent are 22 ones, 0000 11 00.  A square root of a whenever a has one; the caller squares it to know.
SK_HD sk_fe sk_sqrt(const sk_fe& a) {
  const sk_runs r = sk_pow_runs(a);
  sk_fe t = sk_mul(sk_sqrn(r.x223, 23), r.x22);
  t = sk_mul(sk_sqrn(t, 6), r.x2);
  return sk_sqrn(t, 2);
}

// ---- the group ----------------------------------------------------------------------------------------------------------------------------
SK_HD sk_pt sk_identity() {
  sk_pt r;
  r.X = sk_small(0); r.Y = sk_small(1); r.Z = sk_small(0);
  return r;
}
SK_HD sk_pt sk_from_affine(const sk_aff& a) {                // (0, 0) -> the identity
  sk_pt r;
  const bool id = sk_is_zero(a.x) && sk_is_zero(a.y);
  r.X = a.x;
  r.Y = sk_sel(id, sk_small(1), a.y);
  r.Z = sk_small(id ? 0u : 1u);
  return r;
}
SK_HD sk_aff sk_to_affine(const sk_pt& p) {                  // the identity has Z = 0, whose "inverse" is 0: (0, 0) falls out
  const sk_fe zi = sk_inv(p.Z);
  sk_aff r;
  r.x = sk_mul(p.X, zi);
  r.y = sk_mul(p.Y, zi);
  return r;
}
SK_HD sk_aff sk_neg_affine(const sk_aff& a) {
  sk_aff r;
  r.x = a.x;
  r.y = sk_neg(a.y);
  return r;
}
// canonical coordinates and y^2 = x^3 + 7; (0, 0) is not on the curve
SK_HD bool sk_on_curve(const sk_aff& a) {
  if (!sk_is_canonical(a.x) || !sk_is_canonical(a.y)) return false;
  return sk_eq(sk_sqr(a.y), sk_add(sk_mul(sk_sqr(a.x), a.x), sk_small(7)));
}
SK_HD bool sk_scalar_ok(const sk_fe& s) { return sk_less(s, sk_order()); }

// Renes-Costello-Batina algorithm 7 (a = 0, b3 = 3 * 7): 12 products and 2 by b3
SK_HD sk_pt sk_padd(const sk_pt& p, const sk_pt& q) {
  sk_fe t0 = sk_mul(p.X, q.X), t1 = sk_mul(p.Y, q.Y), t2 = sk_mul(p.Z, q.Z);
  sk_fe t3 = sk_mul(sk_add(p.X, p.Y), sk_add(q.X, q.Y));
  t3 = sk_sub(t3, sk_add(t0, t1));
  sk_fe t4 = sk_mul(sk_add(p.Y, p.Z), sk_add(q.Y, q.Z));
  t4 = sk_sub(t4, sk_add(t1, t2));
  sk_fe y3 = sk_mul(sk_add(p.X, p.Z), sk_add(q.X, q.Z));
  y3 = sk_sub(y3, sk_add(t0, t2));
  t0 = sk_add(sk_add(t0, t0), t0);
  t2 = sk_mul_small(t2, 21);
  sk_fe z3 = sk_add(t1, t2);
  t1 = sk_sub(t1, t2);
  y3 = sk_mul_small(y3, 21);
  sk_pt r;
  r.X = sk_sub(sk_mul(t3, t1), sk_mul(t4, y3));
  r.Y = sk_add(sk_mul(t1, z3), sk_mul(y3, t0));
  r.Z = sk_add(sk_mul(z3, t4), sk_mul(t0, t3));
  return r;
}
// algorithm 9: 6 products, 2 squarings and 1 by b3
SK_HD sk_pt sk_pdbl(const sk_pt& p) {
  sk_fe t0 = sk_sqr(p.Y);
  sk_fe z3 = sk_add(t0, t0);
  z3 = sk_add(z3, z3);
  z3 = sk_add(z3, z3);
  sk_fe t1 = sk_mul(p.Y, p.Z);
  sk_fe t2 = sk_mul_small(sk_sqr(p.Z), 21);
  sk_fe x3 = sk_mul(t2, z3);
  sk_fe y3 = sk_add(t0, t2);
  sk_pt r;
  r.Z = sk_mul(t1, z3);
  t2 = sk_add(sk_add(t2, t2), t2);
  t0 = sk_sub(t0, t2);
  r.Y = sk_add(x3, sk_mul(t0, y3));
  x3 = sk_mul(t0, sk_mul(p.X, p.Y));
  r.X = sk_add(x3, x3);
  return r;
}

// a P + b Q, projective.  P and Q affine, (0, 0) the identity; a and b any 256-bit integers.
SK_HD sk_pt sk_lincomb_proj(sk_fe a, const sk_aff& P, sk_fe b, const sk_aff& Q) {
  const sk_pt p = sk_from_affine(P), q = sk_from_affine(Q);
  const sk_pt pq = sk_padd(p, q);
  const sk_fe zero = sk_small(0), one = sk_small(1);
  sk_pt r = sk_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < 256; i++) {
    const bool ba = a.l[7] >> 31, bb = b.l[7] >> 31;          // the top bits; the scalars then move up one place, so no word is indexed
#pragma unroll
    for (int k = 7; k > 0; k--) {
      a.l[k] = (a.l[k] << 1) | (a.l[k - 1] >> 31);
      b.l[k] = (b.l[k] << 1) | (b.l[k - 1] >> 31);
    }
    a.l[0] <<= 1;
    b.l[0] <<= 1;
    sk_pt e;                                                  // neither: the identity, either: P or Q, both: P + Q
    e.X = sk_sel(ba, sk_sel(bb, pq.X, p.X), sk_sel(bb, q.X, zero));
    e.Y = sk_sel(ba, sk_sel(bb, pq.Y, p.Y), sk_sel(bb, q.Y, one));
    e.Z = sk_sel(ba, sk_sel(bb, pq.Z, p.Z), sk_sel(bb, q.Z, zero));
    r = sk_padd(sk_pdbl(r), e);
  }
  return r;
}
SK_HD sk_aff sk_lincomb(const sk_fe& a, const sk_aff& P, const sk_fe& b, const sk_aff& Q) { return sk_to_affine(sk_lincomb_proj(a, P, b, Q)); }

// k P, projective, by the plain left-to-right ladder over the table {P}: 256 doublings and 256 additions, the identity added where the bit is
// zero.  P affine, (0, 0) the identity; k any 256-bit integer.  A third fewer live words than the joint ladder with b = 0.
SK_HD sk_pt sk_mul_proj(sk_fe k, const sk_aff& P) {
  const sk_pt p = sk_from_affine(P);
  const sk_fe zero = sk_small(0), one = sk_small(1);
  sk_pt r = sk_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < 256; i++) {
    const bool bit = k.l[7] >> 31;
#pragma unroll
    for (int j = 7; j > 0; j--) k.l[j] = (k.l[j] << 1) | (k.l[j - 1] >> 31);
    k.l[0] <<= 1;
    sk_pt e;
    e.X = sk_sel(bit, p.X, zero);
    e.Y = sk_sel(bit, p.Y, one);
    e.Z = sk_sel(bit, p.Z, zero);
    r = sk_padd(sk_pdbl(r), e);
  }
  return r;
}

// ---- scalars mod n ------------------------------------------------------------------------------------------------------------------------
// r (eight words) + c * 2^256 with c < 2^32 -> canonical mod n: c * delta_n is added (bound (3) above), a wrap adds delta_n once more, and one
// conditional subtraction finishes: r - n = r + delta_n - 2^256, so the carry of r + delta_n says r >= n.
SK_HD void sk_scalar_delta(uint32_t d[5]) {
  d[0] = 0x2FC9BEBFu; d[1] = 0x402DA173u; d[2] = 0x50B75FC4u; d[3] = 0x45512319u; d[4] = 1u;
}
// out = a + c * delta_n over eight words; the carry out of 2^256 is returned.  c < 2^32.
SK_HD uint32_t sk_scalar_add_delta(const sk_fe& a, uint32_t c, sk_fe& out) {
  uint32_t d[5];
  sk_scalar_delta(d);
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t prod = i < 5 ? (uint64_t)c * d[i] : 0u;    // <= (2^32 - 1)^2; with a.l[i] and the carry <= 2^64 - 1
    acc = (acc >> 32) + a.l[i] + prod;
    out.l[i] = (uint32_t)acc;
  }
  return (uint32_t)(acc >> 32);
}
SK_HD sk_fe sk_scalar_fold(const sk_fe& r, uint32_t c) {
  sk_fe o, t;
  const uint32_t wrap = sk_scalar_add_delta(r, c, o);         // 0 or 1
  sk_scalar_add_delta(o, wrap, t);                            // no carry: where wrap is 1, o < 2^161
  const uint32_t ge = sk_scalar_add_delta(t, 1u, o);
  return sk_sel(ge != 0, o, t);
}
// lo (eight words) + h (NH words) * delta_n -> out (eight words and NH + 5 - 8 more, at least one)
template <int NH>
SK_HD void sk_scalar_fold_wide(const uint32_t* lo, const uint32_t* h, uint32_t* out) {
  constexpr int W = NH + 5 > 9 ? NH + 5 : 9;
  uint32_t d[5];
  sk_scalar_delta(d);
#pragma unroll
  for (int i = 0; i < W; i++) out[i] = i < 8 ? lo[i] : 0u;
#pragma unroll
  for (int i = 0; i < NH; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const uint64_t acc = (uint64_t)h[i] * d[j] + out[i + j] + carry;   // <= 2^64 - 1, as in sk_mul
      out[i + j] = (uint32_t)acc;
      carry = acc >> 32;
    }
#pragma unroll
    for (int k = i + 5; k < W; k++) {                         // the sum stays below 2^(32 W) (bounds (1), (2)): the last carry is zero
      carry += out[k];
      out[k] = (uint32_t)carry;
      carry >>= 32;
    }
  }
}
// sixteen little-endian words -> the value mod n
SK_HD sk_fe sk_scalar_reduce512(const uint32_t* t) {
  uint32_t a[13], b[10];
  sk_scalar_fold_wide<8>(t, t + 8, a);                        // (1): thirteen words, a[8 .. 12] <= delta_n
  sk_scalar_fold_wide<5>(a, a + 8, b);                        // (2): b[8] <= 2, b[9] = 0
  sk_fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = b[i];
  return sk_scalar_fold(r, b[8]);                             // (3), (4)
}
// any 256-bit a -> a mod n
SK_HD sk_fe sk_scalar_reduce(const sk_fe& a) { return sk_scalar_fold(a, 0u); }
SK_HD sk_fe sk_scalar_add(const sk_fe& a, const sk_fe& b) {
  sk_fe s;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    acc = (acc >> 32) + a.l[i] + b.l[i];
    s.l[i] = (uint32_t)acc;
  }
  return sk_scalar_fold(s, (uint32_t)(acc >> 32));
}
// a b + c mod n: the 512-bit product, c added into it ((2^256 - 1)^2 + 2^256 - 1 < 2^512: no carry leaves word 15)
SK_HD sk_fe sk_scalar_muladd(const sk_fe& a, const sk_fe& b, const sk_fe& c) {
  uint32_t t[16];
#pragma unroll
  for (int i = 0; i < 16; i++) t[i] = i < 8 ? c.l[i] : 0u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t acc = (uint64_t)a.l[i] * b.l[j] + t[i + j] + carry;
      t[i + j] = (uint32_t)acc;
      carry = acc >> 32;
    }
#pragma unroll
    for (int k = i + 8; k < 16; k++) {
      carry += t[k];
      t[k] = (uint32_t)carry;
      carry >>= 32;
    }
  }
  return sk_scalar_reduce512(t);
}
SK_HD sk_fe sk_scalar_mul(const sk_fe& a, const sk_fe& b) { return sk_scalar_muladd(a, b, sk_small(0)); }
// a SHA-256 digest (eight big-endian words) read as a big-endian integer, mod n
SK_HD sk_fe sk_scalar_from_digest(const uint32_t d[8]) {
  sk_fe a;
#pragma unroll
  for (int i = 0; i < 8; i++) a.l[i] = d[7 - i];
  return sk_scalar_reduce(a);
}

// `compress_point`: 33 bytes, 02 | 03 then x big-endian, as nine big-endian words whose last holds one byte at the top
SK_HD void sk_compress(const sk_aff& a, uint32_t c[9]) {
  c[0] = ((2u + (a.y.l[0] & 1u)) << 24) | (a.x.l[7] >> 8);
#pragma unroll
  for (int k = 1; k < 8; k++) c[k] = (a.x.l[8 - k] << 24) | (a.x.l[7 - k] >> 8);
  c[8] = a.x.l[0] << 24;
}

}  // namespace zkhip

// The optimal ate pairing on BN254: the tower Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v), xi = 9 + u, over the Fq2 of ec2.hpp; the Miller
// loop over 6x + 2 with T in homogeneous projective coordinates on the twist and the lines evaluated at the affine P; the final exponentiation
// (easy part, then the hard part by the addition chain of Scott, Benger, Charlemagne, Dominguez Perez, Kachisa, "On the final exponentiation for
// calculating pairings on ordinary elliptic curves", Pairing 2009, with the cyclotomic squaring of Granger and Scott, PKC 2010).
//
// Replaces halo2curves bn256::{Fq6, Fq12, multi_miller_loop, MillerLoopResult::final_exponentiation} [DEP] under `verify_proof` and the decider's
// pairing check (/root/reference/aggregator/src/wrapper.rs:117-155, 1140-1158).  Only the VERDICT "the product of pairings is one" is an interface:
// any fixed non-zero power of the reduced pairing gives the same verdicts, so the Gt value never leaves this file's callers.
//
// Every formula is written once over a small policy parameter `M` that supplies the Fq2 product and square:
//   f2_single  f2_mul / f2_sqr of ec2.hpp (Karatsuba, one lane).  Host and device: the CPU tests run it, and it is the device fallback.
//   f2_quad    f2_mul_quad / f2_sqr_quad of ec2_quad.hpp: the four lanes of a quad share every product, so an Fq2 product costs the latency of
//              one Fq product.  All four lanes of the quad must be active and hold identical arguments.
// STANDARD FORM EVERYWHERE: every Fq2 value between operations is in the standard form of ec2.hpp (N form, < 2p + 2^233); nothing is kept lazy
// across operations, and the few lazy steps inside one operation have their bounds written next to them.
// Elements are structs with named members: no run-time-indexed arrays (they would live in scratch memory).
#pragma once
#include "ec2.hpp"
#include "fe_inverse.hpp"
#include "pairing_constants.hpp"
#if defined(__HIPCC__)
#include "ec2_quad.hpp"
#define ZK_HD_NI __host__ __device__ __noinline__
#else
#define ZK_HD_NI inline
#endif

namespace zkhip {

struct fe6 { fe2 c0, c1, c2; };          // c0 + c1 v + c2 v^2
struct fe12 { fe6 c0, c1; };             // c0 + c1 w
struct line12 { fe2 a, b, c; };          // the sparse line value a + b w + c w^3 = (a, 0, 0) + (b, c, 0) w

struct f2_single {
  ZK_HD fe2 mul(const fe2& a, const fe2& b) const { return f2_mul(a, b); }
  ZK_HD fe2 sqr(const fe2& a) const { return f2_sqr(a); }
};
#if defined(__HIPCC__)
struct f2_quad {
  uint32_t q;                            // lane within the quad
  ZK_D fe2 mul(const fe2& a, const fe2& b) const { return f2_mul_quad(a, b, q); }
  ZK_D fe2 sqr(const fe2& a) const { return f2_sqr_quad(a, q); }
};
#endif

// ---- Fq2 helpers -----------------------------------------------------------------------------------------------------------------------
ZK_HD fe2 f2_conj(const fe2& a) { return {a.c0, std_form(fe_neg_red(a.c1, Fq::P4_S1))}; }
ZK_HD fe2 f2_const(const uint32_t (&c0)[NL], const uint32_t (&c1)[NL]) { return {fe_const<Fq>(c0), fe_const<Fq>(c1)}; }   // canonical: standard form
// (9 + u)(a0 + a1 u) = (9 a0 - a1) + (9 a1 + a0) u.  9 a by three normalised doublings and one addition: < 9 (2p + 2^233) < 18.1p, N form;
// 9 a0 + 4p - a1 < 22.1p and 9 a1 + a0 < 20.2p, limbs < 2^31: within std_form's input range (< 2^261 = 169p).
ZK_HD fe2 f2_mul_xi(const fe2& a) {
  const fe n0 = fe_norm(fe_add(fe_norm(fe_dbl(fe_norm(fe_dbl(fe_norm(fe_dbl(a.c0)))))), a.c0));
  const fe n1 = fe_norm(fe_add(fe_norm(fe_dbl(fe_norm(fe_dbl(fe_norm(fe_dbl(a.c1)))))), a.c1));
  return {std_form(fe_sub_red(n0, a.c1, Fq::P4_S1)), std_form(fe_add(n1, a.c0))};
}
// 1 / a through the norm map to Fq: a^-1 = conj(a) / (a0^2 + a1^2).  0 -> 0.
ZK_HD fe2 f2_inverse(const fe2& a) {
  const fe n = fe_add(fe_sqr<Fq>(a.c0), fe_sqr<Fq>(a.c1));      // < 4p, limbs < 2^30: fe_inverse canonicalises first
  const fe i = fe_inverse<Fq>(n);                               // N form, < 2p
  return {std_form(fe_mul<Fq>(a.c0, i)), std_form(fe_neg_red(fe_mul<Fq>(a.c1, i), Fq::P4_S1))};
}
ZK_HD fe2 f2_triple(const fe2& a) { return f2_add(f2_dbl(a), a); }
ZK_HD fe2 f2_select(bool s, const fe2& a, const fe2& b) {       // s ? a : b, limb by limb (no address select: see quad_pick)
  fe2 r;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const uint32_t a0 = a.c0.l[i], b0 = b.c0.l[i], a1 = a.c1.l[i], b1 = b.c1.l[i];
    r.c0.l[i] = s ? a0 : b0;
    r.c1.l[i] = s ? a1 : b1;
  }
  return r;
}
// canonical comparison with a canonical constant
ZK_HD bool fe_equals_canon(const fe& a, const fe& canon) {
  const fe c = fe_canon<Fq>(a);
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) d |= c.l[i] ^ canon.l[i];
  return d == 0;
}

// ---- Fq6 -----------------------------------------------------------------------------------------------------------------------------------
ZK_HD fe6 f6_zero() { return {f2_zero(), f2_zero(), f2_zero()}; }
ZK_HD fe6 f6_one() { return {f2_one(), f2_zero(), f2_zero()}; }
ZK_HD fe6 f6_add(const fe6& a, const fe6& b) { return {f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
ZK_HD fe6 f6_sub(const fe6& a, const fe6& b) { return {f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
ZK_HD fe6 f6_dbl(const fe6& a) { return {f2_dbl(a.c0), f2_dbl(a.c1), f2_dbl(a.c2)}; }
ZK_HD fe6 f6_neg(const fe6& a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
ZK_HD fe6 f6_mul_v(const fe6& a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; }          // v (c0 + c1 v + c2 v^2) = xi c2 + c0 v + c1 v^2

// Karatsuba over Fq2: 6 products
template <class M>
ZK_HD fe6 f6_mul(const fe6& a, const fe6& b, const M m) {
  const fe2 v0 = m.mul(a.c0, b.c0), v1 = m.mul(a.c1, b.c1), v2 = m.mul(a.c2, b.c2);
  const fe2 t12 = f2_sub(f2_sub(m.mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), v1), v2);
  const fe2 t01 = f2_sub(f2_sub(m.mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), v0), v1);
  const fe2 t02 = f2_sub(f2_sub(m.mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), v0), v2);
  return {f2_add(v0, f2_mul_xi(t12)), f2_add(t01, f2_mul_xi(v2)), f2_add(t02, v1)};
}
// Chung-Hasan SQR2: 2 products + 3 squares
template <class M>
ZK_HD fe6 f6_sqr(const fe6& a, const M m) {
  const fe2 s0 = m.sqr(a.c0), s1 = f2_dbl(m.mul(a.c0, a.c1)), s2 = m.sqr(f2_add(f2_sub(a.c0, a.c1), a.c2));
  const fe2 s3 = f2_dbl(m.mul(a.c1, a.c2)), s4 = m.sqr(a.c2);
  return {f2_add(s0, f2_mul_xi(s3)), f2_add(s1, f2_mul_xi(s4)), f2_sub(f2_sub(f2_add(f2_add(s1, s2), s3), s0), s4)};
}
template <class M>
ZK_HD fe6 f6_scale(const fe6& a, const fe2& k, const M m) { return {m.mul(a.c0, k), m.mul(a.c1, k), m.mul(a.c2, k)}; }
// a (b + c v): 6 products
template <class M>
ZK_HD fe6 f6_mul_by_01(const fe6& a, const fe2& b, const fe2& c, const M m) {
  return {f2_add(m.mul(a.c0, b), f2_mul_xi(m.mul(a.c2, c))), f2_add(m.mul(a.c0, c), m.mul(a.c1, b)), f2_add(m.mul(a.c1, c), m.mul(a.c2, b))};
}
// through the norm map to Fq2: t0 = c0^2 - xi c1 c2, t1 = xi c2^2 - c0 c1, t2 = c1^2 - c0 c2, a^-1 = (t0, t1, t2) / (c0 t0 + xi (c2 t1 + c1 t2))
template <class M>
ZK_HD fe6 f6_inverse(const fe6& a, const M m) {
  const fe2 t0 = f2_sub(m.sqr(a.c0), f2_mul_xi(m.mul(a.c1, a.c2)));
  const fe2 t1 = f2_sub(f2_mul_xi(m.sqr(a.c2)), m.mul(a.c0, a.c1));
  const fe2 t2 = f2_sub(m.sqr(a.c1), m.mul(a.c0, a.c2));
  const fe2 n = f2_add(m.mul(a.c0, t0), f2_mul_xi(f2_add(m.mul(a.c2, t1), m.mul(a.c1, t2))));
  const fe2 i = f2_inverse(n);
  return {m.mul(t0, i), m.mul(t1, i), m.mul(t2, i)};
}

// ---- Fq12 ----------------------------------------------------------------------------------------------------------------------------------
ZK_HD fe12 f12_one() { return {f6_one(), f6_zero()}; }
ZK_HD fe12 f12_conj(const fe12& a) { return {a.c0, f6_neg(a.c1)}; }                  // a^(q^6)
ZK_HD fe12 f12_select(bool s, const fe12& a, const fe12& b) {
  return {{f2_select(s, a.c0.c0, b.c0.c0), f2_select(s, a.c0.c1, b.c0.c1), f2_select(s, a.c0.c2, b.c0.c2)},
          {f2_select(s, a.c1.c0, b.c1.c0), f2_select(s, a.c1.c1, b.c1.c1), f2_select(s, a.c1.c2, b.c1.c2)}};
}
// Karatsuba over Fq6: 18 Fq2 products
template <class M>
ZK_HD_NI fe12 f12_mul(const fe12& a, const fe12& b, const M m) {
  const fe6 aa = f6_mul(a.c0, b.c0, m), bb = f6_mul(a.c1, b.c1, m);
  const fe6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1), m);
  return {f6_add(aa, f6_mul_v(bb)), f6_sub(f6_sub(s, aa), bb)};
}
// complex squaring: (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1, 2 a0 a1: 12 Fq2 products
template <class M>
ZK_HD_NI fe12 f12_sqr(const fe12& a, const M m) {
  const fe6 ab = f6_mul(a.c0, a.c1, m);
  const fe6 t = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)), m);
  return {f6_sub(f6_sub(t, ab), f6_mul_v(ab)), f6_dbl(ab)};
}
// through the norm map to Fq6: a^-1 = conj(a) / (a0^2 - v a1^2)
template <class M>
ZK_HD_NI fe12 f12_inverse(const fe12& a, const M m) {
  const fe6 i = f6_inverse(f6_sub(f6_sqr(a.c0, m), f6_mul_v(f6_sqr(a.c1, m))), m);
  return {f6_mul(a.c0, i, m), f6_neg(f6_mul(a.c1, i, m))};
}
// f (a + b w + c w^3) = (f0 a + v f1 (b + c v)) + (f0 (b + c v) + f1 a) w: 3 + 6 + 6 Fq2 products (second half by Karatsuba)
template <class M>
ZK_HD_NI fe12 f12_mul_line(const fe12& f, const line12& l, const M m) {
  const fe6 t0 = f6_scale(f.c0, l.a, m);
  const fe6 t1 = f6_mul_by_01(f.c1, l.b, l.c, m);
  const fe6 s = f6_mul_by_01(f6_add(f.c0, f.c1), f2_add(l.a, l.b), l.c, m);
  return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(s, t0), t1)};
}

// Frobenius a^(q^K), K = 1, 2, 3: the coefficient of w^i is conjugated K times and multiplied by GAMMA_K_i (pairing_constants.hpp)
#define ZK_GAMMA(K, I) f2_const(PairingParams::GAMMA_##K##_##I##_C0, PairingParams::GAMMA_##K##_##I##_C1)
template <int K, class M>
ZK_HD_NI fe12 f12_frobenius(const fe12& a, const M m) {
  static_assert(K >= 1 && K <= 3, "Frobenius power");
  fe12 r;
  if constexpr (K == 1) {
    r.c0.c0 = f2_conj(a.c0.c0);                                        // w^0
    r.c1.c0 = m.mul(f2_conj(a.c1.c0), ZK_GAMMA(1, 1));                 // w^1
    r.c0.c1 = m.mul(f2_conj(a.c0.c1), ZK_GAMMA(1, 2));                 // w^2 = v
    r.c1.c1 = m.mul(f2_conj(a.c1.c1), ZK_GAMMA(1, 3));                 // w^3
    r.c0.c2 = m.mul(f2_conj(a.c0.c2), ZK_GAMMA(1, 4));                 // w^4 = v^2
    r.c1.c2 = m.mul(f2_conj(a.c1.c2), ZK_GAMMA(1, 5));                 // w^5
  } else if constexpr (K == 2) {
    r.c0.c0 = a.c0.c0;
    r.c1.c0 = m.mul(a.c1.c0, ZK_GAMMA(2, 1));
    r.c0.c1 = m.mul(a.c0.c1, ZK_GAMMA(2, 2));
    r.c1.c1 = m.mul(a.c1.c1, ZK_GAMMA(2, 3));
    r.c0.c2 = m.mul(a.c0.c2, ZK_GAMMA(2, 4));
    r.c1.c2 = m.mul(a.c1.c2, ZK_GAMMA(2, 5));
  } else {
    r.c0.c0 = f2_conj(a.c0.c0);
    r.c1.c0 = m.mul(f2_conj(a.c1.c0), ZK_GAMMA(3, 1));
    r.c0.c1 = m.mul(f2_conj(a.c0.c1), ZK_GAMMA(3, 2));
    r.c1.c1 = m.mul(f2_conj(a.c1.c1), ZK_GAMMA(3, 3));
    r.c0.c2 = m.mul(f2_conj(a.c0.c2), ZK_GAMMA(3, 4));
    r.c1.c2 = m.mul(f2_conj(a.c1.c2), ZK_GAMMA(3, 5));
  }
  return r;
}

// a^2 for a in the cyclotomic subgroup (a^(q^4 - q^2 + 1) = 1: everything after the easy part), Granger-Scott: with the three Fq4 elements
// (z0, z1) = (c0.c0, c1.c1), (z2, z3) = (c1.c0, c0.c2), (z4, z5) = (c0.c1, c1.c2): 9 Fq2 products instead of 12, in 3 independent groups
template <class M>
ZK_HD void f4_sqr(const fe2& a, const fe2& b, fe2& t0, fe2& t1, const M m) {      // (a + b y)^2, y^2 = xi: t0 = a^2 + xi b^2, t1 = 2 a b
  const fe2 ab = m.mul(a, b);
  t0 = f2_sub(f2_sub(m.mul(f2_add(a, b), f2_add(f2_mul_xi(b), a)), ab), f2_mul_xi(ab));
  t1 = f2_dbl(ab);
}
template <class M>
ZK_HD_NI fe12 f12_cyclotomic_sqr(const fe12& a, const M m) {
  fe2 t0, t1, t2, t3, t4, t5;
  f4_sqr(a.c0.c0, a.c1.c1, t0, t1, m);
  f4_sqr(a.c1.c0, a.c0.c2, t2, t3, m);
  f4_sqr(a.c0.c1, a.c1.c2, t4, t5, m);
  fe12 r;
  r.c0.c0 = f2_add(f2_dbl(f2_sub(t0, a.c0.c0)), t0);                  // 3 t0 - 2 z0
  r.c1.c1 = f2_add(f2_dbl(f2_add(t1, a.c1.c1)), t1);                  // 3 t1 + 2 z1
  const fe2 x5 = f2_mul_xi(t5);
  r.c1.c0 = f2_add(f2_dbl(f2_add(x5, a.c1.c0)), x5);                  // 3 xi t5 + 2 z2
  r.c0.c2 = f2_add(f2_dbl(f2_sub(t4, a.c0.c2)), t4);                  // 3 t4 - 2 z3
  r.c0.c1 = f2_add(f2_dbl(f2_sub(t2, a.c0.c1)), t2);                  // 3 t2 - 2 z4
  r.c1.c2 = f2_add(f2_dbl(f2_add(t3, a.c1.c2)), t3);                  // 3 t3 + 2 z5
  return r;
}

// a^x for a in the cyclotomic subgroup, x the curve parameter (63 bits, top bit set): plain bits of a compile-time constant, tested uniformly
template <class M>
ZK_HD fe12 f12_pow_x(const fe12& a, const M m) {
  fe12 r = a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 61; i >= 0; i--) {
    r = f12_cyclotomic_sqr(r, m);
    if ((PairingParams::X >> i) & 1) r = f12_mul(r, a, m);
  }
  return r;
}

// ---- Miller loop ---------------------------------------------------------------------------------------------------------------------------
struct g2_proj { fe2 X, Y, Z; };         // x = X / Z, y = Y / Z on the twist

// T <- 2T and the tangent at T evaluated at P = (xp, yp), scaled by 2 Y Z^2 (an Fq2 factor: the final exponentiation removes it):
// with W = 3 X^2, S = Y Z:  l = 2 S Z yp - W Z xp w + (W X - 2 Y S) w^3.   (lambda = W / 2S; l = yp - lambda xp w + (lambda x - y) w^3.)
// 2T: B = X Y S, H = W^2 - 8B, X' = 2 H S, Y' = W (4B - H) - 8 Y^2 S^2, Z' = 8 S^3.  The twist's constant is not used.
template <class M>
ZK_HD_NI line12 miller_double(g2_proj& T, const fe& xp, const fe& yp, const M m) {
  const fe2 W = f2_triple(m.sqr(T.X)), S = m.mul(T.Y, T.Z), YS = m.mul(T.Y, S);
  const fe2 SZ2 = f2_dbl(m.mul(S, T.Z)), WZ = m.mul(W, T.Z);
  line12 l;
  l.a = {std_form(fe_mul<Fq>(SZ2.c0, yp)), std_form(fe_mul<Fq>(SZ2.c1, yp))};
  l.b = f2_neg({std_form(fe_mul<Fq>(WZ.c0, xp)), std_form(fe_mul<Fq>(WZ.c1, xp))});
  l.c = f2_sub(m.mul(W, T.X), f2_dbl(YS));
  const fe2 B = m.mul(T.X, YS), B4 = f2_dbl(f2_dbl(B));
  const fe2 H = f2_sub(m.sqr(W), f2_dbl(B4));
  const fe2 SS = m.sqr(S), YS2 = m.sqr(YS);
  T.X = f2_dbl(m.mul(H, S));
  T.Y = f2_sub(m.mul(W, f2_sub(B4, H)), f2_dbl(f2_dbl(f2_dbl(YS2))));
  T.Z = f2_dbl(f2_dbl(f2_dbl(m.mul(S, SS))));
  return l;
}
// T <- T + Q (Q = (x2, y2) affine, not +-T) and the line through them at P, scaled by v:
// u = y2 Z - Y, v = x2 Z - X:  l = v yp - u xp w + (u x2 - v y2) w^3.
// T + Q: A = u^2 Z - v^3 - 2 v^2 X, X' = v A, Y' = u (v^2 X - A) - v^3 Y, Z' = v^3 Z.
template <class M>
ZK_HD_NI line12 miller_add(g2_proj& T, const fe2& x2, const fe2& y2, const fe& xp, const fe& yp, const M m) {
  const fe2 u = f2_sub(m.mul(y2, T.Z), T.Y), v = f2_sub(m.mul(x2, T.Z), T.X);
  line12 l;
  l.a = {std_form(fe_mul<Fq>(v.c0, yp)), std_form(fe_mul<Fq>(v.c1, yp))};
  l.b = f2_neg({std_form(fe_mul<Fq>(u.c0, xp)), std_form(fe_mul<Fq>(u.c1, xp))});
  l.c = f2_sub(m.mul(u, x2), m.mul(v, y2));
  const fe2 vv = m.sqr(v), vvv = m.mul(v, vv), R = m.mul(vv, T.X);
  const fe2 A = f2_sub(f2_sub(m.mul(m.sqr(u), T.Z), vvv), f2_dbl(R));
  T.Y = f2_sub(m.mul(u, f2_sub(R, A)), m.mul(vvv, T.Y));
  T.X = m.mul(v, A);
  T.Z = m.mul(vvv, T.Z);
  return l;
}

// The Miller value of one pair.  P = (xp, yp) and Q = (xq, yq) affine, standard form; `skip` (either point the identity, or an idle slot)
// runs the same instructions on whatever the coordinates hold and returns 1: nothing diverges.  Points are not checked.
template <class M>
ZK_HD fe12 miller_loop(const fe& xp, const fe& yp, const fe2& xq, const fe2& yq, bool skip, const M m) {
  fe12 f = f12_one();
  g2_proj T = {xq, yq, f2_one()};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 63; i >= 0; i--) {                                      // 6x + 2 = 2^64 + ATE_LOW: the top bit is T = Q, f = 1
    f = f12_sqr(f, m);
    f = f12_mul_line(f, miller_double(T, xp, yp, m), m);
    if ((PairingParams::ATE_LOW >> i) & 1) f = f12_mul_line(f, miller_add(T, xq, yq, xp, yp, m), m);
  }
  // the two closing additions: pi(Q) = (conj(x) GAMMA_1_2, conj(y) GAMMA_1_3), -pi^2(Q) = (x GAMMA_2_2, y) since GAMMA_2_3 = -1
  const fe2 x1 = m.mul(f2_conj(xq), ZK_GAMMA(1, 2)), y1 = m.mul(f2_conj(yq), ZK_GAMMA(1, 3));
  f = f12_mul_line(f, miller_add(T, x1, y1, xp, yp, m), m);
  const fe2 x2 = m.mul(xq, ZK_GAMMA(2, 2));
  f = f12_mul_line(f, miller_add(T, x2, yq, xp, yp, m), m);
  return f12_select(skip, f12_one(), f);
}

// f^((q^12 - 1) / r): easy part f^((q^6 - 1)(q^2 + 1)), then the hard part (q^4 - q^2 + 1) / r by the chain of Scott et al.:
// y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 with y0 = f^(q + q^2 + q^3), y1 = 1/f, y2 = f^(x^2 q^2), y3 = 1/f^(x q), y4 = 1/(f^x f^(x^2 q)),
// y5 = 1/f^(x^2), y6 = 1/(f^(x^3) f^(x^3 q)); in the cyclotomic subgroup 1/a = conj(a).  0 -> 0 (the inverse of 0 is 0).
template <class M>
ZK_HD fe12 final_exponentiation(const fe12& f, const M m) {
  fe12 t = f12_mul(f12_conj(f), f12_inverse(f, m), m);
  t = f12_mul(f12_frobenius<2>(t, m), t, m);
  const fe12 fu = f12_pow_x(t, m), fu2 = f12_pow_x(fu, m), fu3 = f12_pow_x(fu2, m);
  const fe12 y0 = f12_mul(f12_mul(f12_frobenius<1>(t, m), f12_frobenius<2>(t, m), m), f12_frobenius<3>(t, m), m);
  const fe12 y1 = f12_conj(t);
  const fe12 y2 = f12_frobenius<2>(fu2, m);
  const fe12 y3 = f12_conj(f12_frobenius<1>(fu, m));
  const fe12 y4 = f12_conj(f12_mul(fu, f12_frobenius<1>(fu2, m), m));
  const fe12 y5 = f12_conj(fu2);
  const fe12 y6 = f12_conj(f12_mul(fu3, f12_frobenius<1>(fu3, m), m));
  fe12 t0 = f12_mul(f12_mul(f12_cyclotomic_sqr(y6, m), y4, m), y5, m);
  fe12 t1 = f12_mul(f12_mul(y3, y5, m), t0, m);
  t0 = f12_mul(t0, y2, m);
  t1 = f12_cyclotomic_sqr(f12_mul(f12_cyclotomic_sqr(t1, m), t0, m), m);
  t0 = f12_mul(t1, y1, m);
  t1 = f12_mul(t1, y0, m);
  return f12_mul(f12_cyclotomic_sqr(t0, m), t1, m);
}

ZK_HD bool f12_is_one(const fe12& a) {
  const fe one = fe_canon<Fq>(fe_one<Fq>()), zero = fe_zero();
  bool ok = fe_equals_canon(a.c0.c0.c0, one) && fe_equals_canon(a.c0.c0.c1, zero);
  ok = ok && fe_equals_canon(a.c0.c1.c0, zero) && fe_equals_canon(a.c0.c1.c1, zero) && fe_equals_canon(a.c0.c2.c0, zero) && fe_equals_canon(a.c0.c2.c1, zero);
  ok = ok && fe_equals_canon(a.c1.c0.c0, zero) && fe_equals_canon(a.c1.c0.c1, zero) && fe_equals_canon(a.c1.c1.c0, zero) && fe_equals_canon(a.c1.c1.c1, zero);
  ok = ok && fe_equals_canon(a.c1.c2.c0, zero) && fe_equals_canon(a.c1.c2.c1, zero);
  return ok;
}

// ---- external formats ----------------------------------------------------------------------------------------------------------------------
// Fq12 in memory: the 12 Fq coefficients c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1, each 8 u32 words Montgomery-256 (96 words).
ZK_HD fe pairing_fq_in(const uint32_t* w8) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = w8[i];
  return std_form(fe_mul<Fq>(fe_one<Fq>(), fe_from_ext_lazy(w)));
}
ZK_HD void pairing_fq_out(const fe& a, uint32_t* out8) {
  uint32_t w[8];
  fe_to_ext<Fq>(a, w);
#pragma unroll
  for (int i = 0; i < 8; i++) out8[i] = w[i];
}
ZK_HD fe2 pairing_f2_in(const uint32_t* w16) { return {pairing_fq_in(w16), pairing_fq_in(w16 + 8)}; }
ZK_HD void pairing_f2_out(const fe2& a, uint32_t* out16) { pairing_fq_out(a.c0, out16); pairing_fq_out(a.c1, out16 + 8); }
ZK_HD fe12 pairing_f12_in(const uint32_t* w) {
  return {{pairing_f2_in(w), pairing_f2_in(w + 16), pairing_f2_in(w + 32)}, {pairing_f2_in(w + 48), pairing_f2_in(w + 64), pairing_f2_in(w + 80)}};
}
ZK_HD void pairing_f12_out(const fe12& a, uint32_t* out) {
  pairing_f2_out(a.c0.c0, out); pairing_f2_out(a.c0.c1, out + 16); pairing_f2_out(a.c0.c2, out + 32);
  pairing_f2_out(a.c1.c0, out + 48); pairing_f2_out(a.c1.c1, out + 64); pairing_f2_out(a.c1.c2, out + 80);
}
ZK_HD bool pairing_words_all_zero(const uint32_t* w, int n) {
  uint32_t o = 0;
  for (int i = 0; i < n; i++) o |= w[i];
  return o == 0;
}
// one pair from memory (G1Affine 16 words, G2Affine 32 words) -> its Miller value; an identity on either side gives 1
template <class M>
ZK_HD fe12 miller_loop_words(const uint32_t* g1, const uint32_t* g2, bool idle, const M m) {
  const bool skip = idle || pairing_words_all_zero(g1, 16) || pairing_words_all_zero(g2, 32);
  return miller_loop(pairing_fq_in(g1), pairing_fq_in(g1 + 8), pairing_f2_in(g2), pairing_f2_in(g2 + 16), skip, m);
}

// the whole check on one lane: is prod_i e(g1[i], g2[i]) one?  (host: the CPU tests; device: the single-lane fallback / comparison)
template <class M>
ZK_HD bool pairing_check_serial(const uint32_t* g1, const uint32_t* g2, size_t n, const M m) {
  fe12 f = f12_one();
  for (size_t i = 0; i < n; i++) f = f12_mul(f, miller_loop_words(g1 + 16 * i, g2 + 32 * i, false, m), m);
  return f12_is_one(final_exponentiation(f, m));
}

// ---- one tower operation by number: the test hook (zkhip_test_fq12_op) and the host driver of the CPU tests ----------------------------------
// a, b, out: 96 words each.  0 mul, 1 sqr, 2 inverse, 3 / 4 / 5 Frobenius q / q^2 / q^3, 6 cyclotomic square, 7 a times the line whose
// coefficients (a, b, c) are the first three Fq2 of b, 8 the Miller value of the pair a = G1Affine (16 words) | G2Affine (32 words),
// 9 the final exponentiation, 10 conjugation, 11 the whole check of the two pairs a = 2 G1Affine (32 words) | 2 G2Affine (64 words) as one serial
// chain under the policy (out word 0 = the verdict, the rest zero): what the single-lane / quad comparison of tools/verify_time.py times
constexpr int PAIRING_TEST_OPS = 12;
// (every case stores its own result: one result variable assigned in a run-time switch becomes a select between stack addresses)
template <class M>
ZK_HD void pairing_test_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, const M m) {
  if (op == 11) {
    const bool one = pairing_check_serial(a, a + 32, 2, m);
    for (int i = 1; i < 96; i++) out[i] = 0;
    out[0] = one ? 1u : 0u;
  } else if (op == 8) {
    pairing_f12_out(miller_loop_words(a, a + 16, false, m), out);
  } else if (op == 0) {
    pairing_f12_out(f12_mul(pairing_f12_in(a), pairing_f12_in(b), m), out);
  } else if (op == 1) {
    pairing_f12_out(f12_sqr(pairing_f12_in(a), m), out);
  } else if (op == 2) {
    pairing_f12_out(f12_inverse(pairing_f12_in(a), m), out);
  } else if (op == 3) {
    pairing_f12_out(f12_frobenius<1>(pairing_f12_in(a), m), out);
  } else if (op == 4) {
    pairing_f12_out(f12_frobenius<2>(pairing_f12_in(a), m), out);
  } else if (op == 5) {
    pairing_f12_out(f12_frobenius<3>(pairing_f12_in(a), m), out);
  } else if (op == 6) {
    pairing_f12_out(f12_cyclotomic_sqr(pairing_f12_in(a), m), out);
  } else if (op == 7) {
    pairing_f12_out(f12_mul_line(pairing_f12_in(a), line12{pairing_f2_in(b), pairing_f2_in(b + 16), pairing_f2_in(b + 32)}, m), out);
  } else if (op == 9) {
    pairing_f12_out(final_exponentiation(pairing_f12_in(a), m), out);
  } else {
    pairing_f12_out(f12_conj(pairing_f12_in(a)), out);
  }
}

}  // namespace zkhip

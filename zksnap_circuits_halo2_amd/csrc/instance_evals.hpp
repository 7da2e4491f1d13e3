// The evaluations of the instance columns a PLONK verifier needs at its point x (include/zkhip.h, "the quotient identity at x").  With
// halo2's KZG scheme (`QUERY_INSTANCE = false`) an instance polynomial is neither committed nor opened: [DEP] halo2-axiom plonk/verifier.rs
// `verify_proof` evaluates it at x omega^rot from the public inputs, `l_i_range` and an inner product.  For a column of `len` values v_i
// (zeros behind them) and a query at rotation rot, with l_i(omega^rot x) = l_(i - rot)(x) and n = 2^k:
//
//   e = sum_{i < len} v_i l_((i - rot) mod n)(x) = (x^n - 1) / n * sum_{i < len} v_i w_i / (x - w_i),     w_i = omega^(i - rot)
//
// The sum is carried as a running FRACTION N / D, as identity_points.hpp carries the blinding rows: N <- N (x - w) + (v w) D,
// D <- D (x - w), three products per term and no storage.  A query is shared by a GROUP of G lanes: lane g takes the terms
// i = g, g + G, ..., stepping w by omega^G; two fractions join as (N1 D2 + N2 D1) / (D1 D2), log2 G times; ONE inversion per group.
// This file is the arithmetic of one lane and of one join, for host and device (tests/cpp/instance_evals_host_check.cpp runs the groups
// lane by lane under ASan + UBSan); the cross-lane exchange and the memory layout are verify_identity.hip's.
//
// A point of the domain (x^n = 1) may have a zero among the denominators: nothing is inverted and the evaluation is written as zero
// (the identity call's status 2).  Values are in the internal form of fp29.hpp; the output is canonical.
#pragma once
#include "identity_points.hpp"

namespace zkhip {

struct ie_fraction {
  fe num, den;                                  // N form, each < 2p
};

template <class P>
ZK_HD ie_fraction ie_empty() { return ie_fraction{fe_zero(), fe_one<P>()}; }

// f + v w / (x - w).  x, w < 2p; v: any lazily reduced value fe_mul accepts (an element just unpacked from its external words included)
template <class P>
ZK_HD void ie_term(ie_fraction& f, const fe& x, const fe& w, const fe& v) {
  const fe b = ip_sub<P>(x, w);                                              // < 5p, limbs < 2^29
  const fe vw = fe_mul<P>(v, w);                                             // 32p 2p / (169 p) + p < 2p
  f.num = fe_mul_add<P>(f.num, b, vw, f.den);                                // (2p 5p + 2p 2p) / (169 p) + p < 2p
  f.den = fe_mul<P>(f.den, b);
}

// a + b.  Symmetric in its operands: two lanes that exchange their fractions end with the same one.
template <class P>
ZK_HD ie_fraction ie_join(const ie_fraction& a, const ie_fraction& b) {
  ie_fraction r;
  r.num = fe_mul_add<P>(a.num, b.den, b.num, a.den);                         // (2p 2p + 2p 2p) / (169 p) + p < 2p
  r.den = fe_mul<P>(a.den, b.den);
  return r;
}

// Lane g of a group of G: the terms i = g, g + G, ... < len.  x_in, omega_in, omega_g_in (= omega^G): lazily reduced; rot < 2^k, k <= 28;
// value(i) yields v_i (lazily reduced) and is called for i < len only.  The exponent of the first w is (g - rot) mod n: it wraps below zero
// for rot > g.  Lanes of a group run different trip counts (len / G rounded either way); the caller joins them behind the loop.
template <class P, class V>
ZK_HD ie_fraction ie_lane(const fe& x_in, uint32_t k, const fe& omega_in, const fe& omega_g_in, uint32_t rot, uint32_t len, uint32_t g, uint32_t G, V&& value) {
  const fe one = fe_one<P>();
  ie_fraction f = ie_empty<P>();
  if (g >= len) return f;
  const fe x = fe_mul<P>(one, x_in), step = fe_mul<P>(one, omega_g_in);      // < 2p
  const uint32_t n = 1u << k;
  fe w = ip_pow<P>(fe_mul<P>(one, omega_in), (g + n - rot) & (n - 1u));
  for (uint32_t i = g;;) {
    ie_term<P>(f, x, w, value(i));
    i += G;                                                                  // (len <= 2^28, G <= 16: no wrap)
    if (i >= len) break;
    w = fe_mul<P>(w, step);
  }
  return f;
}

// The group's first lane, with the joined fraction: (x^n - 1) / n * N / D, canonical; zero for a point of the domain, nothing inverted.
// An empty sum (len = 0: N = 0, D = 1) gives zero through the same path.
template <class P>
ZK_HD fe ie_finish(const ie_fraction& f, const fe& x_in, uint32_t k, const fe& n_inv) {
  const fe one = fe_one<P>();
  fe xn = fe_mul<P>(one, x_in);
  for (uint32_t i = 0; i < k; i++) xn = fe_sqr<P>(xn);
  if (ip_is_one<P>(fe_canon_lt2p<P>(xn))) return fe_zero();
  const fe c = fe_mul<P>(ip_sub<P>(xn, one), n_inv);                         // (x^n - 1) / n
  return fe_canon_lt2p<P>(fe_mul<P>(fe_mul<P>(c, f.num), fe_inverse<P>(f.den)));
}

}  // namespace zkhip

// CPU unit test of the *device* arithmetic: csrc/fp29.hpp and csrc/ec.hpp are host-compilable, so the lazy radix-2^29
// field and the XYZZ point formulas are exercised here (built with -fsanitize=address,undefined by tests/test_host_arith.py)
// against an independent schoolbook big-integer implementation (bigint_ref.hpp, shared with ec2_host_check.cpp).  Besides equality
// it checks the magnitude discipline the GPU kernels rely on: every stored coordinate is in N form with the documented value bound,
// also when every operand enters at the top of its own bound (fe_lift.hpp).
#include "bigint_ref.hpp"   // the big-integer reference, conversions, rnd() and CHECK
#include "fe_inverse.hpp"
#include "fe_lift.hpp"

template <class P> static void field_tests(const char* name) {
  const big p = modulus<P>(), rinv = invmod(R261<P>(), p);
  for (int it = 0; it < 3000; it++) {
    big x = rnd_below(p), y = rnd_below(p);
    if (it == 0) { x = big_zero(); }
    if (it == 1) { x = big_sub(p, [] { big o = big_zero(); o.w[0] = 1; return o; }()); y = x; }
    fe a = to_fe<P>(x), b = to_fe<P>(y);
    fe m = fe_mul<P>(a, b), s = fe_sqr<P>(a);
    CHECK(is_N(m) && below(m, 2, p) && big_cmp(to_int<P>(m, rinv), mulmod(x, y, p)) == 0, name);
    CHECK(is_N(s) && below(s, 2, p) && big_cmp(to_int<P>(s, rinv), mulmod(x, x, p)) == 0, name);
    // lazy operands: sums of a few elements (limbs < 2^31) times a normalised one, as the point formulas use them
    fe lazy = fe_add(fe_add(a, b), fe_add(a, a));
    CHECK(big_cmp(to_int<P>(fe_mul<P>(b, lazy), rinv), mulmod(y, addmod(addmod(x, y, p), addmod(x, x, p), p), p)) == 0, name);
    CHECK(big_cmp(to_int<P>(fe_sub_red(a, b, P::P3_S1), rinv), submod(x, y, p)) == 0, name);
    CHECK(big_cmp(to_int<P>(fe_norm(lazy), rinv), to_int<P>(lazy, rinv)) == 0 && is_N(fe_norm(lazy)), name);
    fe c = fe_canon<P>(lazy);
    CHECK(below(c, 1, p) && big_cmp(to_int<P>(c, rinv), to_int<P>(lazy, rinv)) == 0, name);
    fe soft = fe_reduce_soft<P>(fe_norm(fe_add(lazy, lazy)));
    CHECK(below(soft, 3, p) && big_cmp(to_int<P>(soft, rinv), to_int<P>(fe_add(lazy, lazy), rinv)) == 0, name);
    CHECK(fe_mulout_is_zero<P>(fe_mul<P>(a, fe_zero())), name);
    // external format round trip: words of x*2^256 <-> internal
    big r256 = big_zero(); r256.w[4] = 1; r256 = big_mod(r256, p);
    big ext = mulmod(x, r256, p);
    uint32_t w[8], w2[8];
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)(ext.w[i >> 1] >> ((i & 1) * 32));
    fe in = fe_from_ext_lazy(w);
    CHECK(big_cmp(to_int<P>(in, rinv), x) == 0, name);
    fe_to_ext<P>(in, w2);
    CHECK(memcmp(w, w2, 32) == 0, name);
  }
  // The unscaled last pass of the NTT (ntt.hip ntt_emit) canonicalises k p + y, k <= 28, with fe_reduce_soft and conditional subtractions and no
  // multiplication.  Every representative k p of zero must come out as the word 0, and every k p + y as y.  The quotient estimate of
  // fe_reduce_soft is at least k - 1 for these k (k p_top / (p_top + 1) > k - 1), so its result is below 2p, not only below 2p + 2^233:
  // one conditional subtraction already gives the canonical value, and the second one of fe_canon_lt3p never fires.
  {
    const big one_b = [] { big o = big_zero(); o.w[0] = 1; return o; }();
    big low_full = big_zero();                                    // eight full 29-bit limbs
    for (int i = 0; i < 3; i++) low_full.w[i] = ~0ULL;
    low_full.w[3] = (1ULL << (8 * LB - 192)) - 1;
    big kp = big_zero();
    for (unsigned k = 0; k <= 28; k++, kp = big_add(kp, p)) {
      for (int it = 0; it < 12; it++) {
        big y = rnd_below(p);
        if (it == 0) y = big_zero();
        if (it == 1) y = one_b;
        if (it == 2) y = big_sub(p, one_b);
        if (it == 3) y = low_full;
        const fe x = fe_from_big(big_add(kp, y));
        CHECK(is_N(x) && big_cmp(fe_value(x), big_add(kp, y)) == 0, name);
        const fe soft = fe_reduce_soft<P>(x);
        CHECK(is_N(soft) && below(soft, 2, p) && big_cmp(big_mod(fe_value(soft), p), y) == 0, name);
        const fe c2 = fe_canon_lt2p<P>(soft), c3 = fe_canon_lt3p<P>(soft);
        CHECK(is_N(c3) && big_cmp(fe_value(c3), y) == 0 && big_cmp(fe_value(c2), y) == 0, name);
        if (it == 0) CHECK(fe_is_zero_limbs(c3) && fe_is_zero_limbs(c2), name);
        uint32_t w[8];
        fe_pack(c3, w);
        for (int i = 0; i < 8; i++) CHECK(w[i] == (uint32_t)(y.w[i >> 1] >> ((i & 1) * 32)), name);
      }
    }
  }
  // inversion by division steps (fe_inverse.hpp) against the big-integer a^(p-2): plain integers and Montgomery-261 values, edge values,
  // and lazily reduced inputs (0 -> 0)
  const big one_b = [] { big o = big_zero(); o.w[0] = 1; return o; }();
  for (int it = 0; it < 600; it++) {
    big x = rnd_below(p);
    if (it == 0) x = big_zero();
    if (it == 1) x = one_b;
    if (it == 2) x = big_sub(p, one_b);
    if (it == 3) { x = big_zero(); x.w[0] = 2; }
    if (it == 4) x = big_sub(p, big_add(one_b, one_b));
    if (it >= 5 && it < 40) { x = big_zero(); x.w[(it - 5) / 9] = 1ULL << (7 * ((it - 5) % 9)); x = big_mod(x, p); }      // single bits
    if (it >= 40 && it < 60) { x = rnd_below(p); x.w[3] = 0; x.w[2] = 0; if (it & 1) x.w[1] = 0; }                       // short values
    const big want = big_cmp(x, big_zero()) == 0 ? big_zero() : invmod(x, p);
    const fe plain = fe_inverse_plain<P>(fe_from_big(x));
    CHECK(is_N(plain) && below(plain, 1, p) && big_cmp(fe_value(plain), want) == 0, name);
    const fe a = to_fe<P>(x);
    const fe inv = fe_inverse<P>(a);
    CHECK(is_N(inv) && below(inv, 2, p) && big_cmp(to_int<P>(inv, rinv), want) == 0, name);
    fe k; for (int i = 0; i < NL; i++) k.l[i] = P::P8_S1[i];
    const fe inv_lazy = fe_inverse<P>(fe_add(fe_add(a, k), k));          // the same element + 16p, limbs up to 2^31
    CHECK(big_cmp(to_int<P>(inv_lazy, rinv), want) == 0, name);
  }
}

// ---- curve: affine reference over the big-int field ---------------------------------------------------------------------
struct apt { big x, y; bool inf; };
static apt a_add(const apt& P, const apt& Q, const big& q) {
  if (P.inf) return Q;
  if (Q.inf) return P;
  big lam;
  if (big_cmp(P.x, Q.x) == 0) {
    if (big_cmp(P.y, Q.y) != 0 || big_cmp(P.y, big_zero()) == 0) return apt{big_zero(), big_zero(), true};
    big three = big_zero(); three.w[0] = 3;
    lam = mulmod(mulmod(three, mulmod(P.x, P.x, q), q), invmod(addmod(P.y, P.y, q), q), q);
  } else lam = mulmod(submod(Q.y, P.y, q), invmod(submod(Q.x, P.x, q), q), q);
  big x3 = submod(submod(mulmod(lam, lam, q), P.x, q), Q.x, q);
  return apt{x3, submod(mulmod(lam, submod(P.x, x3, q), q), P.y, q), false};
}
static apt xyzz_to_affine(const xyzz& a, const big& q, const big& rinv) {
  if (xyzz_is_identity(a)) return apt{big_zero(), big_zero(), true};
  big X = to_int<Fq>(a.X, rinv), Y = to_int<Fq>(a.Y, rinv), ZZ = to_int<Fq>(a.ZZ, rinv), ZZZ = to_int<Fq>(a.ZZZ, rinv);
  return apt{mulmod(X, invmod(ZZ, q), q), mulmod(Y, invmod(ZZZ, q), q), false};
}
static bool same(const apt& a, const apt& b) { return a.inf == b.inf && (a.inf || (big_cmp(a.x, b.x) == 0 && big_cmp(a.y, b.y) == 0)); }
static bool stored_ok(const xyzz& a, const big& q) {   // the stored-point invariant of ec.hpp
  return is_N(a.X) && is_N(a.Y) && is_N(a.ZZ) && is_N(a.ZZZ) && below(a.X, 9, q) && below(a.Y, 5, q) && below(a.ZZ, 2, q) && below(a.ZZZ, 2, q);
}

static void curve_tests() {
  const big q = modulus<Fq>(), rinv = invmod(R261<Fq>(), q);
  apt G; G.x = big_zero(); G.x.w[0] = 1; G.y = big_zero(); G.y.w[0] = 2; G.inf = false;
  std::vector<apt> pts;
  apt cur = G;
  for (int i = 0; i < 40; i++) { pts.push_back(cur); cur = a_add(cur, (i % 3 == 0) ? cur : G, q); }
  auto lazy_in = [&](const big& v) { fe t = to_fe<Fq>(v); fe k; for (int i = 0; i < NL; i++) k.l[i] = Fq::P32_S1[i]; return fe_norm(fe_add(t, k)); };   // same element, value + 32p: as unreduced as a lazy external load
  for (int it = 0; it < 600; it++) {
    // a chain of mixed additions with occasional repeats (doubling path) and negations (cancellation path)
    xyzz acc = xyzz_identity();
    apt ref{big_zero(), big_zero(), true};
    int len = 1 + (int)(rnd() % 12);
    for (int j = 0; j < len; j++) {
      apt P = pts[rnd() % pts.size()];
      uint64_t mode = rnd() % 8;
      if (mode == 0 && !ref.inf) P = ref;                                   // acc += acc  -> doubling inside madd
      if (mode == 1 && !ref.inf) { P = ref; P.y = submod(big_zero(), P.y, q); }   // acc += -acc -> identity
      fe x2 = (j & 1) ? lazy_in(P.x) : to_fe<Fq>(P.x), y2 = (j & 1) ? lazy_in(P.y) : to_fe<Fq>(P.y);
      if (mode == 2) { y2 = fe_neg_red(to_fe<Fq>(P.y), Fq::P64_S1); P.y = submod(big_zero(), P.y, q); x2 = to_fe<Fq>(P.x); }   // negated load
      xyzz_madd(acc, x2, y2);
      ref = a_add(ref, P, q);
      CHECK(xyzz_is_identity(acc) || stored_ok(acc, q), "madd stored-point invariant");
      CHECK(same(xyzz_to_affine(acc, q, rinv), ref), "madd value");
    }
    // general addition / doubling of two accumulated points
    xyzz other = xyzz_identity();
    apt oref{big_zero(), big_zero(), true};
    int len2 = (int)(rnd() % 5);
    for (int j = 0; j < len2; j++) { apt P = pts[rnd() % pts.size()]; xyzz_madd(other, to_fe<Fq>(P.x), to_fe<Fq>(P.y)); oref = a_add(oref, P, q); }
    if (rnd() % 6 == 0) { other = acc; oref = ref; }
    xyzz sum = xyzz_add(acc, other), dbl = xyzz_dbl(acc);
    CHECK(same(xyzz_to_affine(sum, q, rinv), a_add(ref, oref, q)) && (xyzz_is_identity(sum) || stored_ok(sum, q)), "xyzz_add");
    CHECK(same(xyzz_to_affine(dbl, q, rinv), a_add(ref, ref, q)) && (xyzz_is_identity(dbl) || stored_ok(dbl, q)), "xyzz_dbl");
  }
}

// ---- the shapes the MSM kernels instantiate, at the top of their documented operand bounds (fe_lift.hpp) -----------------------------
// fe_mul_add<P, CHAIN> against a b + c d, and fe_mul / fe_sqr at their limb limits.  (On the host both CHAIN values run the portable
// column code; the device's asm-block shape is reached through zkhip_test_field_op ops 4-7.)
template <class P, bool CHAIN> static void mul_add_tests(const char* name) {
  const big p = modulus<P>(), rinv = invmod(R261<P>(), p), one_b = big_small(1), pm1 = big_sub(p, one_b);
  const big edge[3] = {big_zero(), one_b, pm1};
  for (int it = 0; it < 1500; it++) {
    big x = rnd_below(p), y = rnd_below(p), z = rnd_below(p), w = rnd_below(p);
    if (it < 81) { x = edge[it % 3]; y = edge[(it / 3) % 3]; z = edge[(it / 9) % 3]; w = edge[(it / 27) % 3]; }
    if (it >= 81 && it < 120) { z = submod(big_zero(), x, p); w = y; }                      // c = -a, d = b: the sum is = 0 mod p
    if (it >= 120 && it < 130) { x = edge[it % 3]; z = submod(big_zero(), x, p); w = y; }
    const big want = addmod(mulmod(x, y, p), mulmod(z, w, p), p);
    const fe a = to_fe<P>(x), b = to_fe<P>(y), c = to_fe<P>(z), d = to_fe<P>(w);
    const fe r = fe_mul_add<P, CHAIN>(a, b, c, d);
    CHECK(mulout_ok(r, a, b, &c, &d, p) && big_cmp(to_int<P>(r, rinv), want) == 0, name);
    if (it >= 81 && it < 130) CHECK(fe_mulout_is_zero<P>(r) && big_cmp(want, big_zero()) == 0, name);
    // the limit ec.hpp uses: a, c in N form; b with limbs < 3 * 2^29 (T = Q + 10p - X3); d with limbs < 2^30 (6p - Y1)
    const fe aN = fe_lift<P>(a, 2), cN = fe_lift<P>(c, 2), bL = fe_lift_lazy<P>(b, 3), dL = fe_lift_lazy<P>(d, 2);
    CHECK(is_N(aN) && is_N(cN) && !below(aN, 1, p) && below(aN, 2, p) && big_cmp(to_int<P>(bL, rinv), y) == 0 && big_cmp(to_int<P>(dL, rinv), w) == 0, name);
    const fe rl = fe_mul_add<P, CHAIN>(aN, bL, cN, dL);
    CHECK(mulout_ok(rl, aN, bL, &cN, &dL, p) && below(rl, 2, p) && big_cmp(to_int<P>(rl, rinv), want) == 0, name);
    if (it >= 81 && it < 130) CHECK(fe_mulout_is_zero<P>(rl), name);
    // Y3 of xyzz_madd_nz<true> with its own operands at their largest: R < 8p (N), T = Q + 10p - X3 < 12p with X3 small (limb-wise, not
    // normalised), PPP (N, < 2p here: more than its 1.14p), 6p - Y1 with Y1 small: the result must stay below the 1.7p of ec.hpp's comment
    const fe R8 = fe_lift<P>(a, 8), T12 = fe_sub_red(fe_lift<P>(b, 2), fe_canon<P>(d), P::P10_S1), negY = fe_neg_red(d, P::P6_S1);
    const fe y3 = fe_mul_add<P, CHAIN>(R8, T12, cN, negY);
    CHECK(mulout_ok(y3, R8, T12, &cN, &negY, p) && below_frac(y3, 170, 100, p), name);
    CHECK(big_cmp(to_int<P>(y3, rinv), submod(mulmod(x, submod(y, w, p), p), mulmod(z, w, p), p)) == 0, name);
    // fe_mul: N x limbs < 2^31.5 (5 * 2^29 = 2^31.3); fe_sqr: limbs < 2^30.3 (2 * 2^29)
    const fe b5 = fe_lift_lazy<P>(b, 5), a2 = fe_lift_lazy<P>(a, 2);
    const fe m = fe_mul<P, CHAIN>(aN, b5), s = fe_sqr<P, CHAIN>(a2);
    CHECK(mulout_ok(m, aN, b5, nullptr, nullptr, p) && below(m, 2, p) && big_cmp(to_int<P>(m, rinv), mulmod(x, y, p)) == 0, name);
    CHECK(mulout_ok(s, a2, a2, nullptr, nullptr, p) && below(s, 2, p) && big_cmp(to_int<P>(s, rinv), mulmod(x, x, p)) == 0, name);
  }
}

// the chain of curve_tests through xyzz_madd<true> (what the bucket kernels instantiate: Y3 = R T + PPP (6p - Y1) under one reduction),
// unlifted and with every operand lifted to the top of its bound between the links: X 9p, Y 5p, ZZ / ZZZ 2p, x2 / y2 64p
static void chain_shape_curve_tests(bool lifted) {
  const big q = modulus<Fq>(), rinv = invmod(R261<Fq>(), q);
  apt G; G.x = big_small(1); G.y = big_small(2); G.inf = false;
  std::vector<apt> pts;
  apt cur = G;
  for (int i = 0; i < 40; i++) { pts.push_back(cur); cur = a_add(cur, (i % 3 == 0) ? cur : G, q); }
  auto lazy_in = [&](const big& v) { fe t = to_fe<Fq>(v); fe k; for (int i = 0; i < NL; i++) k.l[i] = Fq::P32_S1[i]; return fe_norm(fe_add(t, k)); };
  for (int it = 0; it < 600; it++) {
    xyzz acc = xyzz_identity();
    apt ref{big_zero(), big_zero(), true};
    int len = 1 + (int)(rnd() % 12);
    for (int j = 0; j < len; j++) {
      apt P = pts[rnd() % pts.size()];
      uint64_t mode = rnd() % 8;
      if (mode == 0 && !ref.inf) P = ref;                                   // acc += acc  -> doubling inside madd
      if (mode == 1 && !ref.inf) { P = ref; P.y = submod(big_zero(), P.y, q); }   // acc += -acc -> identity
      fe x2 = (j & 1) ? lazy_in(P.x) : to_fe<Fq>(P.x), y2 = (j & 1) ? lazy_in(P.y) : to_fe<Fq>(P.y);
      if (lifted) { x2 = fe_lift<Fq>(x2, 64); y2 = fe_lift<Fq>(y2, 64); }
      if (mode == 2) { y2 = fe_neg_red(to_fe<Fq>(P.y), Fq::P64_S1); P.y = submod(big_zero(), P.y, q); }   // negated load: 64p - y, already at the top
      if (lifted) { acc = xyzz_lift(acc); CHECK(xyzz_is_identity(acc) || (stored_ok(acc, q) && !below(acc.X, 8, q) && !below(acc.Y, 4, q) && !below(acc.ZZ, 1, q)), "xyzz_lift"); }
      xyzz_madd<true>(acc, x2, y2);
      ref = a_add(ref, P, q);
      CHECK(xyzz_is_identity(acc) || stored_ok(acc, q), lifted ? "madd<true> stored-point invariant (lifted)" : "madd<true> stored-point invariant");
      CHECK(same(xyzz_to_affine(acc, q, rinv), ref), lifted ? "madd<true> value (lifted)" : "madd<true> value");
    }
  }
}

int main() {
  field_tests<FqParams>("Fq");
  field_tests<FrParams>("Fr");
  curve_tests();
  mul_add_tests<FqParams, false>("Fq fe_mul_add<false>");
  mul_add_tests<FqParams, true>("Fq fe_mul_add<true>");
  mul_add_tests<FrParams, false>("Fr fe_mul_add<false>");
  mul_add_tests<FrParams, true>("Fr fe_mul_add<true>");
  chain_shape_curve_tests(false);
  chain_shape_curve_tests(true);
  printf(fails ? "FAILED: %d checks\n" : "fp29/ec host check OK\n", fails);
  return fails ? 1 : 0;
}

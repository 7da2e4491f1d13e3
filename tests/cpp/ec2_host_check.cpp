// CPU unit test of the G2 device arithmetic: csrc/ec2.hpp is host-compilable, so Fq2 and the XYZZ formulas on the twist -- the
// standard-form layer and the lazy layer the G2 MSM's bucket kernels instantiate (f2_mul_lazy / f2_sqr_lazy over fe_mul_add,
// xyzz2_madd_lazy, xyzz2_add_lazy with xyzz2_dbl_lazy_core, xyzz2_to_std) -- run here under ASan + UBSan (tests/test_host_arith.py)
// against an independent big-integer Fq2 and an affine chord-and-tangent reference written in this file.
//
// Values AND magnitudes: every result must satisfy the bound its call-site comment in ec2.hpp states, with the operands lifted to the
// LARGEST representative below their own documented bounds (csrc/fe_lift.hpp; lift_below for the fractional bounds of the comments).
// Random data sits far below those limits, so only the lifted runs tell whether the hand-derived bounds close.  The residue of a lifted
// operand is unchanged: the expected value is that of the unlifted run, from the same reference.
//
// The formulas never use the curve constant, so any (x, y) with y != 0 is a legitimate input: the "points" are a chord-and-tangent walk
// from a random pair (they lie on the a = 0 curve through it), and the equal-x table uses off-curve neighbours on purpose -- in Fq2 one
// component of P^2 vanishes for P = (t, +-t), (t, 0), (0, t), where a zero test that looked at one component would go wrong.
#include "bigint_ref.hpp"
#include "fe_lift.hpp"

static big Q, RINV, TWO_P_233;

// ---- reference: Fq2 = Fq[u] / (u^2 + 1) on big integers, schoolbook ---------------------------------------------------------------------
struct b2 { big c0, c1; };
static b2 b2_zero() { return {big_zero(), big_zero()}; }
static b2 b2_add(const b2& a, const b2& b) { return {addmod(a.c0, b.c0, Q), addmod(a.c1, b.c1, Q)}; }
static b2 b2_sub(const b2& a, const b2& b) { return {submod(a.c0, b.c0, Q), submod(a.c1, b.c1, Q)}; }
static b2 b2_neg(const b2& a) { return b2_sub(b2_zero(), a); }
static b2 b2_mul(const b2& a, const b2& b) {
  return {submod(mulmod(a.c0, b.c0, Q), mulmod(a.c1, b.c1, Q), Q), addmod(mulmod(a.c0, b.c1, Q), mulmod(a.c1, b.c0, Q), Q)};
}
static b2 b2_inv(const b2& a) {   // (a0 - a1 u) / (a0^2 + a1^2)
  const big n = invmod(addmod(mulmod(a.c0, a.c0, Q), mulmod(a.c1, a.c1, Q), Q), Q);
  return {mulmod(a.c0, n, Q), mulmod(submod(big_zero(), a.c1, Q), n, Q)};
}
static bool b2_eq(const b2& a, const b2& b) { return big_cmp(a.c0, b.c0) == 0 && big_cmp(a.c1, b.c1) == 0; }
static bool b2_is_zero(const b2& a) { return b2_eq(a, b2_zero()); }
static b2 b2_rnd() { return {rnd_below(Q), rnd_below(Q)}; }
static b2 b2_rnd_nz() { b2 r = b2_rnd(); while (b2_is_zero(r)) r = b2_rnd(); return r; }

struct a2pt { b2 x, y; bool inf; };
static a2pt a2_inf() { return {b2_zero(), b2_zero(), true}; }
static a2pt a2_neg(const a2pt& P) { return {P.x, b2_neg(P.y), P.inf}; }
// chord and tangent for a = 0; equal x with unequal y is the identity (what the formulas decide from P = 0, R != 0)
static a2pt a2_add(const a2pt& P, const a2pt& S) {
  if (P.inf) return S;
  if (S.inf) return P;
  b2 lam;
  if (b2_eq(P.x, S.x)) {
    if (!b2_eq(P.y, S.y) || b2_is_zero(P.y)) return a2_inf();
    const b2 xx = b2_mul(P.x, P.x);
    lam = b2_mul(b2_add(b2_add(xx, xx), xx), b2_inv(b2_add(P.y, P.y)));
  } else lam = b2_mul(b2_sub(S.y, P.y), b2_inv(b2_sub(S.x, P.x)));
  const b2 x3 = b2_sub(b2_sub(b2_mul(lam, lam), P.x), S.x);
  return {x3, b2_sub(b2_mul(lam, b2_sub(P.x, x3)), P.y), false};
}

// ---- bridges and bounds ------------------------------------------------------------------------------------------------------------------
static fe2 to_fe2(const b2& a) { return {to_fe<Fq>(a.c0), to_fe<Fq>(a.c1)}; }
static b2 f2_int(const fe2& a) { return {to_int<Fq>(a.c0, RINV), to_int<Fq>(a.c1, RINV)}; }
static bool std_ok(const fe& a) { return is_N(a) && big_cmp(fe_value(a), TWO_P_233) < 0; }          // standard form: N, < 2p + 2^233
static bool std2_ok(const fe2& a) { return std_ok(a.c0) && std_ok(a.c1); }
static bool n_below2(const fe2& a, unsigned k) { return is_N(a.c0) && is_N(a.c1) && below(a.c0, k, Q) && below(a.c1, k, Q); }
static bool point_std_ok(const xyzz2& a) { return xyzz2_is_identity(a) || (std2_ok(a.X) && std2_ok(a.Y) && std2_ok(a.ZZ) && std2_ok(a.ZZZ)); }
// the accumulator invariant of xyzz2_madd_lazy: X < 2p + 2^233, Y < 5p, ZZ < 2p, ZZZ < 2p, all N form
static bool acc_ok(const xyzz2& a) { return xyzz2_is_identity(a) || (std2_ok(a.X) && n_below2(a.Y, 5) && n_below2(a.ZZ, 2) && n_below2(a.ZZZ, 2)); }
// (X, Y, ZZ, ZZZ) is the affine point P: X = x ZZ, Y = y ZZZ, ZZ != 0, ZZ^3 = ZZZ^2 -- no inversion, and stricter than comparing quotients
static bool is_point(const xyzz2& a, const a2pt& P) {
  if (xyzz2_is_identity(a) || P.inf) return xyzz2_is_identity(a) && P.inf;
  const b2 X = f2_int(a.X), Y = f2_int(a.Y), ZZ = f2_int(a.ZZ), ZZZ = f2_int(a.ZZZ);
  return !b2_is_zero(ZZ) && b2_eq(X, b2_mul(P.x, ZZ)) && b2_eq(Y, b2_mul(P.y, ZZZ)) && b2_eq(b2_mul(ZZ, b2_mul(ZZ, ZZ)), b2_mul(ZZZ, ZZZ));
}
// the largest representative of a's residue below (num / 100) p, in N form: the fractional bounds of the call-site comments
static fe lift_below(const fe& a, unsigned num) {
  big v = fe_value(fe_canon<Fq>(a));
  const wide lim = wide_mul(Q, big_small(num));
  while (wide_cmp(wide_mul(big_add(v, Q), big_small(100)), lim) < 0) v = big_add(v, Q);
  return fe_from_big(v);
}
static xyzz2 neg_point(const xyzz2& a) { xyzz2 r = a; if (!xyzz2_is_identity(a)) r.Y = f2_neg(a.Y); return r; }

// ---- zero tests --------------------------------------------------------------------------------------------------------------------------
static void zero_tests() {
  const big one = big_small(1);
  for (unsigned k = 0; k < 3; k++) {
    const big kp = big_times(Q, k);
    CHECK(fe_is_zero_lt3p<Fq>(fe_from_big(kp)), "fe_is_zero_lt3p: 0, p, 2p are zero");
    CHECK(!fe_is_zero_lt3p<Fq>(fe_from_big(big_add(kp, one))), "fe_is_zero_lt3p: k p + 1");
    if (k) CHECK(!fe_is_zero_lt3p<Fq>(fe_from_big(big_sub(kp, one))), "fe_is_zero_lt3p: k p - 1");
    for (int i = 0; i < NL; i++) { fe t = fe_from_big(kp); t.l[i] ^= 1u << (i % 7); CHECK(!fe_is_zero_lt3p<Fq>(t), "fe_is_zero_lt3p: one limb off"); }
    // f2_is_zero over standard-form values: every representative of zero below 2p + 2^233 in either component
    for (unsigned j = 0; j < 3; j++) {
      const fe2 z = {fe_from_big(kp), fe_from_big(big_times(Q, j))};
      CHECK(std2_ok(z) && f2_is_zero(z), "f2_is_zero: (k p, j p)");
      const fe2 n0 = {fe_from_big(big_add(kp, one)), z.c1}, n1 = {z.c0, fe_from_big(big_add(big_times(Q, j), one))};
      CHECK(!f2_is_zero(n0) && !f2_is_zero(n1), "f2_is_zero: one component not zero");
    }
  }
  CHECK(big_cmp(fe_value(fe_from_big(big_times(Q, 2))), big_times(Q, 2)) == 0, "2p round trip");
  fe twop; for (int i = 0; i < NL; i++) twop.l[i] = two_p_limb<Fq>(i);
  CHECK(is_N(twop) && big_cmp(fe_value(twop), big_times(Q, 2)) == 0, "two_p_limb");
}

// ---- standard-form layer -------------------------------------------------------------------------------------------------------------------
static std::vector<a2pt> walk_points() {
  std::vector<a2pt> pts;
  const a2pt G = {b2_rnd_nz(), b2_rnd_nz(), false};
  a2pt cur = G;
  for (int i = 0; i < 40; i++) { pts.push_back(cur); cur = a2_add(cur, (i % 3 == 0) ? cur : G); }
  return pts;
}

static void standard_layer_tests(const std::vector<a2pt>& pts) {
  for (int it = 0; it < 400; it++) {
    b2 x = b2_rnd(), y = b2_rnd();
    if (it == 0) x = b2_zero();
    if (it == 1) { x = {big_sub(Q, big_small(1)), big_sub(Q, big_small(1))}; y = x; }
    if (it == 2) { x = {big_small(1), big_zero()}; }
    if (it == 3) y = x;
    // standard-form operands: canonical, and the top representative below 2p
    for (int lift = 1; lift <= 2; lift++) {
      const fe2 a = f2_lift(to_fe2(x), lift), b = f2_lift(to_fe2(y), lift);
      const fe2 m = f2_mul(a, b), s = f2_sqr(a), d = f2_sub(a, b), n = f2_neg(a), ad = f2_add(a, b), db = f2_dbl(a);
      CHECK(std2_ok(m) && b2_eq(f2_int(m), b2_mul(x, y)), "f2_mul");
      CHECK(std2_ok(s) && b2_eq(f2_int(s), b2_mul(x, x)), "f2_sqr");
      CHECK(std2_ok(d) && b2_eq(f2_int(d), b2_sub(x, y)), "f2_sub");
      CHECK(std2_ok(n) && b2_eq(f2_int(n), b2_neg(x)), "f2_neg");
      CHECK(std2_ok(ad) && b2_eq(f2_int(ad), b2_add(x, y)), "f2_add");
      CHECK(std2_ok(db) && b2_eq(f2_int(db), b2_add(x, x)), "f2_dbl");
      CHECK(f2_is_zero(a) == b2_is_zero(x) && f2_is_zero(d) == b2_eq(x, y) && f2_is_zero(f2_add(a, n)), "f2_is_zero");
    }
  }
  for (int it = 0; it < 150; it++) {
    xyzz2 acc = xyzz2_identity();
    a2pt ref = a2_inf();
    const int len = 1 + (int)(rnd() % 8);
    for (int j = 0; j < len; j++) {
      a2pt P = pts[rnd() % pts.size()];
      const uint64_t mode = rnd() % 8;
      if (mode == 0 && !ref.inf) P = ref;
      if (mode == 1 && !ref.inf) P = a2_neg(ref);
      xyzz2_madd(acc, f2_lift(to_fe2(P.x), 1 + (j & 1)), f2_lift(to_fe2(P.y), 1 + (j & 1)));
      ref = a2_add(ref, P);
      CHECK(point_std_ok(acc) && is_point(acc, ref), "xyzz2_madd");
    }
    xyzz2 other = xyzz2_identity();
    a2pt oref = a2_inf();
    const int len2 = (int)(rnd() % 4);
    for (int j = 0; j < len2; j++) { const a2pt P = pts[rnd() % pts.size()]; xyzz2_madd(other, to_fe2(P.x), to_fe2(P.y)); oref = a2_add(oref, P); }
    const uint64_t pick = rnd() % 6;
    if (pick == 0) { other = acc; oref = ref; }
    if (pick == 1) { other = neg_point(acc); oref = a2_neg(ref); }
    const xyzz2 sum = xyzz2_add(acc, other), dbl = xyzz2_dbl(acc);
    CHECK(point_std_ok(sum) && is_point(sum, a2_add(ref, oref)), "xyzz2_add");
    CHECK(point_std_ok(dbl) && is_point(dbl, a2_add(ref, ref)), "xyzz2_dbl");
  }
}

// ---- lazy Fq2 products: every call site of ec2.hpp, operands at the top of the bounds its comment assumes, output below the bound it states.
// Bounds in hundredths of p.  "2p + 2^233" (standard form) is written 200: the lift stays below 2p.
template <bool CHAIN>
static void mul_site(const char* site, unsigned a_num, unsigned b0_num, unsigned b1_num, const uint32_t (&red)[NL], unsigned o0, unsigned o1) {
  const b2 top = {big_sub(Q, big_small(1)), big_sub(Q, big_small(1))};
  for (int it = 0; it < 40; it++) {
    b2 x = b2_rnd(), y = b2_rnd();
    if (it == 0) x = b2_zero();
    if (it == 1) y = b2_zero();
    if (it == 2) { x = top; y = top; }
    if (it == 3) { x = top; y = {top.c0, big_zero()}; }                           // b1 = 0: red - b1 at its largest
    if (it == 4) { x = {big_zero(), top.c1}; y = {big_small(1), big_small(1)}; }
    for (int lifted = 0; lifted < 2; lifted++) {
      fe2 a = to_fe2(x), b = to_fe2(y);
      if (lifted) { a = {lift_below(a.c0, a_num), lift_below(a.c1, a_num)}; b = {lift_below(b.c0, b0_num), lift_below(b.c1, b1_num)}; }
      const fe2 r = f2_mul_lazy<CHAIN>(a, b, red);
      CHECK(is_N(r.c0) && is_N(r.c1) && below_frac(r.c0, o0, 100, Q) && below_frac(r.c1, o1, 100, Q), site);
      CHECK(b2_eq(f2_int(r), b2_mul(x, y)), site);
    }
  }
}
template <bool CHAIN>
static void sqr_site(const char* site, unsigned a_num, const uint32_t (&red)[NL], unsigned o0, unsigned o1) {
  const b2 top = {big_sub(Q, big_small(1)), big_sub(Q, big_small(1))};
  for (int it = 0; it < 40; it++) {
    b2 x = b2_rnd();
    if (it == 0) x = b2_zero();
    if (it == 1) x = top;
    if (it == 2) x = {top.c0, big_zero()};                                        // a1 = 0: a0 - a1 + red at its largest
    if (it == 3) x = {big_zero(), top.c1};
    if (it == 4) x = {big_small(5), big_small(5)};                                // (t, t): c0 of the square is zero
    for (int lifted = 0; lifted < 2; lifted++) {
      fe2 a = to_fe2(x);
      if (lifted) a = {lift_below(a.c0, a_num), lift_below(a.c1, a_num)};
      const fe2 r = f2_sqr_lazy<CHAIN>(a, red);
      CHECK(is_N(r.c0) && is_N(r.c1) && below_frac(r.c0, o0, 100, Q) && below_frac(r.c1, o1, 100, Q), site);
      CHECK(b2_eq(f2_int(r), b2_mul(x, x)), site);
      if (it == 4) CHECK(fe_is_zero_lt3p<Fq>(r.c0) && !fe_mulout_is_zero<Fq>(r.c1), site);
    }
  }
}

template <bool CHAIN>
static void lazy_product_sites() {
  // xyzz2_madd_lazy
  mul_site<CHAIN>("madd U2/S2 = ZZ x2", 200, 3200, 3200, Fq::P64_S1, 214, 176);
  mul_site<CHAIN>("madd PPP = P PP", 614, 203, 145, Fq::P4_S1, 122, 122);
  mul_site<CHAIN>("madd Q = X PP", 200, 203, 145, Fq::P4_S1, 108, 108);
  mul_site<CHAIN>("madd A = R T", 1000, 508, 508, Fq::P8_S1, 178, 178);
  mul_site<CHAIN>("madd B = Y PPP", 500, 122, 122, Fq::P4_S1, 116, 116);
  mul_site<CHAIN>("madd ZZ PP", 200, 203, 145, Fq::P4_S1, 108, 108);
  mul_site<CHAIN>("madd ZZZ PPP", 200, 122, 122, Fq::P4_S1, 107, 107);
  sqr_site<CHAIN>("madd PP = P^2", 614, Fq::P8_S1, 203, 145);
  sqr_site<CHAIN>("madd RR = R^2", 1000, Fq::P12_S1, 360, 220);
  // xyzz2_dbl_lazy_core
  sqr_site<CHAIN>("dbl V = U^2", 402, Fq::P6_S1, 148, 148);
  mul_site<CHAIN>("dbl W = U V", 402, 148, 148, Fq::P4_S1, 113, 113);
  mul_site<CHAIN>("dbl S = X V", 200, 148, 148, Fq::P4_S1, 107, 107);
  sqr_site<CHAIN>("dbl XX = X^2", 200, Fq::P4_S1, 114, 114);
  sqr_site<CHAIN>("dbl MM = M^2", 342, Fq::P6_S1, 138, 138);
  mul_site<CHAIN>("dbl Am = M T", 342, 507, 507, Fq::P8_S1, 126, 126);
  mul_site<CHAIN>("dbl Bm = W Y", 113, 200, 200, Fq::P4_S1, 104, 104);
  mul_site<CHAIN>("dbl ZZ = V ZZ", 148, 200, 200, Fq::P4_S1, 200, 200);        // no bound written: the result must be in standard form
  mul_site<CHAIN>("dbl ZZZ = W ZZZ", 113, 200, 200, Fq::P4_S1, 200, 200);
  // xyzz2_add_lazy_core
  mul_site<CHAIN>("add U1/U2/S1/S2/ZZ12", 200, 200, 200, Fq::P4_S1, 108, 108);
  sqr_site<CHAIN>("add PP = P^2, RR = R^2", 408, Fq::P6_S1, 149, 120);
  mul_site<CHAIN>("add PPP = P PP", 408, 149, 120, Fq::P4_S1, 114, 114);
  mul_site<CHAIN>("add Q = U1 PP", 108, 149, 120, Fq::P4_S1, 104, 104);
  mul_site<CHAIN>("add Am = R T", 408, 504, 504, Fq::P8_S1, 132, 132);
  mul_site<CHAIN>("add Bm = S1 PPP", 108, 114, 114, Fq::P4_S1, 104, 104);
  mul_site<CHAIN>("add ZZ = ZZ12 PP", 108, 149, 120, Fq::P4_S1, 200, 200);      // standard form
  mul_site<CHAIN>("add ZZZ = (ZZZ1 ZZZ2) PPP", 108, 114, 114, Fq::P4_S1, 200, 200);
}

// ---- xyzz2_madd_lazy chains, xyzz2_to_std, xyzz2_add_lazy ---------------------------------------------------------------------------------
template <bool CHAIN>
static void lazy_chain_tests(const std::vector<a2pt>& pts, bool lifted) {
  for (int it = 0; it < 160; it++) {
    xyzz2 acc = xyzz2_identity();
    a2pt ref = a2_inf();
    const int len = 1 + (int)(rnd() % 12);
    for (int j = 0; j < len; j++) {
      a2pt P = pts[rnd() % pts.size()];
      const uint64_t mode = rnd() % 8;
      if (mode == 0 && !ref.inf) P = ref;                                   // acc += acc: the doubling inside the mixed addition
      if (mode == 1 && !ref.inf) P = a2_neg(ref);                           // acc += -acc: the identity
      const bool neg = (rnd() & 1) != 0;                                    // the load is negated: hand over -P with the flag set
      fe2 x2 = to_fe2(P.x), y2 = to_fe2(neg ? b2_neg(P.y) : P.y);
      if (j & 1) { x2 = f2_lift(x2, 17); y2 = f2_lift(y2, 17); }            // an unreduced lazy load
      if (lifted) { x2 = f2_lift(x2, 32); y2 = f2_lift(y2, 32); acc = xyzz2_lift(acc, 2, 5, 2); CHECK(acc_ok(acc) && is_point(acc, ref), "xyzz2_lift"); }
      xyzz2_madd_lazy<CHAIN>(acc, x2, y2, neg);
      ref = a2_add(ref, P);
      CHECK(acc_ok(acc), lifted ? "madd_lazy accumulator invariant (lifted)" : "madd_lazy accumulator invariant");
      CHECK(is_point(acc, ref), lifted ? "madd_lazy value (lifted)" : "madd_lazy value");
    }
    const xyzz2 A = xyzz2_to_std(lifted ? xyzz2_lift(acc, 2, 5, 2) : acc);
    CHECK(point_std_ok(A) && is_point(A, ref), "xyzz2_to_std");
    // a second accumulated point: independent, the same point (both representatives), its opposite, the identity
    xyzz2 other = xyzz2_identity();
    a2pt oref = a2_inf();
    const int len2 = (int)(rnd() % 5);
    for (int j = 0; j < len2; j++) { const a2pt P = pts[rnd() % pts.size()]; xyzz2_madd_lazy<CHAIN>(other, to_fe2(P.x), to_fe2(P.y), false); oref = a2_add(oref, P); }
    xyzz2 B = xyzz2_to_std(other);
    const uint64_t pick = it < 8 ? it % 4 : rnd() % 8;
    if (pick == 0) { B = A; oref = ref; }                                                       // A + A: xyzz2_dbl_lazy_core
    if (pick == 1) { B = xyzz2_lift(xyzz2_to_std(acc), 1, 1, 1); oref = ref; }                 // A + A, another representative
    if (pick == 2) { B = neg_point(A); oref = a2_neg(ref); }                                    // A + (-A)
    if (pick == 3) { B = xyzz2_identity(); oref = a2_inf(); }
    xyzz2 Al = A;
    if (lifted) { Al = xyzz2_lift(A, 2, 2, 2); B = xyzz2_lift(B, 2, 2, 2); }
    const xyzz2 s1 = xyzz2_add_lazy<CHAIN>(Al, B), s2 = xyzz2_add_lazy<CHAIN>(B, Al), s3 = xyzz2_add_lazy<CHAIN>(Al, Al), s4 = xyzz2_add_lazy<CHAIN>(Al, A);
    CHECK(point_std_ok(s1) && is_point(s1, a2_add(ref, oref)), "add_lazy A + B");
    CHECK(point_std_ok(s2) && is_point(s2, a2_add(oref, ref)), "add_lazy B + A");
    CHECK(point_std_ok(s3) && is_point(s3, a2_add(ref, ref)), "add_lazy A + A");
    CHECK(point_std_ok(s4) && is_point(s4, a2_add(ref, ref)), "add_lazy A + A'");
    const xyzz2 id = xyzz2_identity();
    CHECK(xyzz2_is_identity(xyzz2_add_lazy<CHAIN>(id, id)) && is_point(xyzz2_add_lazy<CHAIN>(id, Al), ref) && is_point(xyzz2_add_lazy<CHAIN>(Al, id), ref), "add_lazy identity");
  }
}

// ---- the equal-x table -----------------------------------------------------------------------------------------------------------------------
// accumulator (x1 l^2, y1 l^3, l^2, l^3) for l = 1, l in Fq, l in u Fq and a random l, plus the point (x1 + d, y1 + e) for d, e in {0, (t,t), (t,-t), (t,0), (0,t)}:
// d = e = 0 is the double, d = 0 with e != 0 the identity, d != 0 the chord sum.
static b2 shape(int k, const big& t) {
  const big mt = submod(big_zero(), t, Q), z = big_zero();
  switch (k) { case 0: return {z, z}; case 1: return {t, t}; case 2: return {t, mt}; case 3: return {t, z}; default: return {z, t}; }
}
template <bool CHAIN>
static void equal_x_table() {
  for (int rep = 0; rep < 5; rep++) {
    // P = U2 - X1 = d l^2 keeps d's shape -- a vanishing component of P^2 -- only when l^2 lies in Fq: l = 1 (an accumulator that holds one
    // point), l = (c, 0), l = (0, c); a general l (reps 3, 4) covers the plain case
    b2 lam = b2_rnd_nz();
    if (rep == 0) lam = {big_small(1), big_zero()};
    if (rep == 1) lam = {lam.c0, big_zero()};
    if (rep == 2) lam = {big_zero(), lam.c1};
    if (b2_is_zero(lam)) lam = {big_small(3), big_zero()};
    const b2 x1 = b2_rnd_nz(), l2 = b2_mul(lam, lam), l3 = b2_mul(l2, lam);
    b2 y1 = b2_rnd_nz();
    big t = rnd_below(Q);
    if (rep == 0) t = big_small(1);
    if (rep == 1) t = big_sub(Q, big_small(1));
    if (big_cmp(t, big_zero()) == 0) t = big_small(7);
    const a2pt P1 = {x1, y1, false};
    for (int dk = 0; dk < 5; dk++) for (int ek = 0; ek < 5; ek++) {
      const a2pt P2 = {b2_add(x1, shape(dk, t)), b2_add(y1, shape(ek, t)), false};
      if (b2_is_zero(P2.y) || big_cmp(P2.y.c0, big_zero()) == 0 || big_cmp(P2.y.c1, big_zero()) == 0) continue;     // (never with random y1)
      const a2pt want = a2_add(P1, P2);
      CHECK(want.inf == (dk == 0 && ek != 0), "equal-x table: reference");
      for (int neg = 0; neg < 2; neg++) for (int lifted = 0; lifted < 2; lifted++) {
        xyzz2 acc = {to_fe2(b2_mul(x1, l2)), to_fe2(b2_mul(y1, l3)), to_fe2(l2), to_fe2(l3)};
        fe2 x2 = to_fe2(P2.x), y2 = to_fe2(neg ? b2_neg(P2.y) : P2.y);
        if (lifted) { acc = xyzz2_lift(acc, 2, 5, 2); x2 = f2_lift(x2, 32); y2 = f2_lift(y2, 32); }
        // the general addition on the same pair: B = (x2, y2, 1, 1) as a work point, both orders
        const xyzz2 Astd = xyzz2_to_std(acc);
        xyzz2 B = {to_fe2(P2.x), to_fe2(P2.y), f2_one(), f2_one()};
        if (lifted) B = xyzz2_lift(B, 2, 2, 2);
        xyzz2_madd_lazy<CHAIN>(acc, x2, y2, neg != 0);
        CHECK(acc_ok(acc) && is_point(acc, want), "equal-x table: madd_lazy");
        const xyzz2 s1 = xyzz2_add_lazy<CHAIN>(Astd, B), s2 = xyzz2_add_lazy<CHAIN>(B, Astd);
        CHECK(point_std_ok(s1) && is_point(s1, want) && point_std_ok(s2) && is_point(s2, want), "equal-x table: add_lazy");
        xyzz2 sa = {to_fe2(b2_mul(x1, l2)), to_fe2(b2_mul(y1, l3)), to_fe2(l2), to_fe2(l3)};
        xyzz2_madd(sa, to_fe2(P2.x), to_fe2(P2.y));
        CHECK(point_std_ok(sa) && is_point(sa, want), "equal-x table: xyzz2_madd");
      }
    }
  }
}

int main() {
  Q = modulus<Fq>();
  RINV = invmod(R261<Fq>(), Q);
  TWO_P_233 = big_times(Q, 2);
  { big t = big_zero(); t.w[233 >> 6] = 1ULL << (233 & 63); TWO_P_233 = big_add(TWO_P_233, t); }
  zero_tests();
  const std::vector<a2pt> pts = walk_points();
  standard_layer_tests(pts);
  lazy_product_sites<false>();
  lazy_product_sites<true>();
  for (int lifted = 0; lifted < 2; lifted++) { lazy_chain_tests<false>(pts, lifted != 0); lazy_chain_tests<true>(pts, lifted != 0); }
  equal_x_table<false>();
  equal_x_table<true>();
  printf(fails ? "FAILED: %d checks\n" : "ec2 host check OK\n", fails);
  return fails ? 1 : 0;
}

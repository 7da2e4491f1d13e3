// Test-only helpers (the zkhip_test_* hooks of selftest.hip and the host checks under tests/cpp): replace a field element by the LARGEST
// representative of the same residue below a documented magnitude bound, so that a formula is run at the top of the operand range its
// call-site comments allow rather than where random data happens to sit.  The residue never changes: the expected value of a lifted run is
// that of the unlifted one.  Nothing on the MSM / NTT paths includes this header.
#pragma once
#include "ec2.hpp"

namespace zkhip {

// same residue, N form, value in [(K - 1) p, K p): the top of the bound "N form, value < K p"  (K >= 1, K p < 2^261)
template <class P>
ZK_HD fe fe_lift(const fe& a, int K) {
  fe r = fe_canon<P>(a);
  const fe p = fe_const<P>(P::P);
#pragma unroll 1
  for (int k = 1; k < K; k++) r = fe_norm(fe_add(r, p));
  return r;
}

// same residue, p added limb-wise K - 1 times with no carry propagation: limbs < K 2^29, the non-N operand shapes of fp29.hpp
// ("N x limbs < 2^31.5", "2^30.3 x 2^30.3", fe_mul_add's column bound)
template <class P>
ZK_HD fe fe_lift_lazy(const fe& a, int K) {
  fe r = fe_canon<P>(a);
  const fe p = fe_const<P>(P::P);
#pragma unroll 1
  for (int k = 1; k < K; k++) r = fe_add(r, p);
  return r;
}

ZK_HD fe2 f2_lift(const fe2& a, int K) { return {fe_lift<Fq>(a.c0, K), fe_lift<Fq>(a.c1, K)}; }

// an accumulator of xyzz_madd<true> (ec.hpp) at the top of its stored-point invariant: X < 9p, Y < 5p, ZZ < 2p, ZZZ < 2p
ZK_HD xyzz xyzz_lift(const xyzz& a) {
  if (xyzz_is_identity(a)) return a;
  return {fe_lift<Fq>(a.X, 9), fe_lift<Fq>(a.Y, 5), fe_lift<Fq>(a.ZZ, 2), fe_lift<Fq>(a.ZZZ, 2)};
}

// a G2 point with component bounds KX, KY, KZ (ZZ and ZZZ) times p: xyzz2_madd_lazy's accumulator is (2, 5, 2), a standard-form
// point (2, 2, 2), a lazy quad point of ec2_quad.hpp (2, 2, 5)
ZK_HD xyzz2 xyzz2_lift(const xyzz2& a, int KX, int KY, int KZ) {
  if (xyzz2_is_identity(a)) return a;
  return {f2_lift(a.X, KX), f2_lift(a.Y, KY), f2_lift(a.ZZ, KZ), f2_lift(a.ZZZ, KZ)};
}

}  // namespace zkhip

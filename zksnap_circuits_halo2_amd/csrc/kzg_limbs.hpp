// A KZG accumulator as public inputs: G1 points <-> limbs in Fr.  For the host and the device (one definition of the arithmetic; the host
// forms touch no GPU and work in a process that never initialises HIP).
//
// NORMATIVE
//   A point becomes ZKHIP_KZG_LIMBS * 2 = 6 Fr values: x's canonical integer is cut little-endian into three 88-bit limbs, then y's; each limb
//   is an Fr element in Montgomery words (4 x u64, radix 2^256), like every Fr the library reads or writes.  An accumulator is `lhs` then
//   `rhs`, 12 values: the reference's `[lhs.x, lhs.y, rhs.x, rhs.y].flat_map(fe_to_limbs::<_, _, LIMBS, BITS>)`
//   (aggregator/src/wrapper.rs, RecursionCircuit::new) with LIMBS = 3, BITS = 88.
//   Points are the library's affine memory: x | y, 4 + 4 u64 Montgomery words of Fq, canonical.
//   Encode splits whatever canonical coordinates it is given; it does not ask whether they are a point: (0, 0) gives six zeros.
//   Decode is strict and never a failed call; it writes one status per point:
//       0  accepted
//       1  a limb is >= 2^88
//       2  a coordinate is >= q
//       3  (x, y) is not on y^2 = x^3 + 3; (0, 0) is status 3, as `from_xy` would refuse it
//   (the first that applies, x before y).  A refused point is written as (0, 0).  The six values must be canonical Fr words (below r): a value
//   of r or more has no limb it could stand for and is reported as status 1.
//   Pins:  (1, 2)  |->  [1, 0, 0,  2, 0, 0]
//          the coordinate q - 1  |->  [0x71ca8d3c208c16d87cfd46, 0x45b68181585d97816a9168, 0x30644e72e131a029b850]
#pragma once
#include <cstddef>
#include <cstdint>

#define ZKHIP_KZG_LIMBS 3
#define ZKHIP_KZG_LIMB_BITS 88

#if defined(__HIPCC__)
#define ZK_LIMBS_HD __host__ __device__ inline
#else
#define ZK_LIMBS_HD inline
#endif

namespace zkhip {
namespace kzg_limbs {

struct field64 {
  uint64_t p[4];      // the modulus
  uint64_t inv;       // -p^-1 mod 2^64
  uint64_t r2[4];     // 2^512 mod p
};
// (functions, not objects: a constexpr object of namespace scope is not usable from device code)
ZK_LIMBS_HD constexpr field64 fq() {
  return {{0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull}, 0x87d20782e4866389ull,
          {0xf32cfc5b538afa89ull, 0xb5e71911d44501fbull, 0x47ab1eff0a417ff6ull, 0x06d89f71cab8351full}};
}
ZK_LIMBS_HD constexpr field64 fr() {
  return {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}, 0xc2e1f593efffffffull,
          {0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull}};
}

ZK_LIMBS_HD bool lt4(const uint64_t a[4], const uint64_t b[4]) {
  for (int i = 3; i >= 0; i--)
    if (a[i] != b[i]) return a[i] < b[i];
  return false;
}

// out = a b 2^-256 mod p for a b < 2^256 p (one of them below p is enough); out < p
ZK_LIMBS_HD void mont_mul(const field64& f, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    unsigned __int128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (unsigned __int128)a[j] * b[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * f.inv;
    c = (unsigned __int128)m * f.p[0] + t[0];
    c >>= 64;
    for (int j = 1; j < 4; j++) {
      c += (unsigned __int128)m * f.p[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  uint64_t d[4];
  unsigned __int128 borrow = 0;
  for (int j = 0; j < 4; j++) {
    const unsigned __int128 s = (unsigned __int128)t[j] - f.p[j] - (uint64_t)borrow;
    d[j] = (uint64_t)s;
    borrow = (s >> 64) & 1;
  }
  const bool keep = t[4] == 0 && borrow;       // t < p
  for (int j = 0; j < 4; j++) out[j] = keep ? t[j] : d[j];
}

ZK_LIMBS_HD void from_mont(const field64& f, const uint64_t a[4], uint64_t out[4]) {    // Montgomery words -> the integer
  const uint64_t one[4] = {1, 0, 0, 0};
  mont_mul(f, a, one, out);
}
ZK_LIMBS_HD void to_mont(const field64& f, const uint64_t a[4], uint64_t out[4]) { mont_mul(f, a, f.r2, out); }    // a < p

// one coordinate (Montgomery words of Fq) -> three Fr values
ZK_LIMBS_HD void encode_coordinate(const uint64_t mont[4], uint64_t* fr_out) {
  uint64_t v[4];
  from_mont(fq(), mont, v);
  const uint64_t lo24 = (1ull << 24) - 1;
  const uint64_t limb[3][4] = {{v[0], v[1] & lo24, 0, 0},
                               {(v[1] >> 24) | (v[2] << 40), (v[2] >> 24) & lo24, 0, 0},
                               {(v[2] >> 48) | (v[3] << 16), v[3] >> 48, 0, 0}};
  for (int i = 0; i < 3; i++) to_mont(fr(), limb[i], fr_out + 4 * i);
}

// three Fr values -> the coordinate's Montgomery words of Fq; 0, 1 or 2 as the header's statuses
ZK_LIMBS_HD uint32_t decode_coordinate(const uint64_t* fr_in, uint64_t mont[4]) {
  uint64_t l[3][4];
  for (int i = 0; i < 3; i++) {
    if (!lt4(fr_in + 4 * i, fr().p)) return 1;
    from_mont(fr(), fr_in + 4 * i, l[i]);
    if (l[i][2] | l[i][3] | (l[i][1] >> 24)) return 1;
  }
  if (l[2][1] >> 16) return 2;                                    // bits 256 .. 263 of the value
  const uint64_t v[4] = {l[0][0], l[0][1] | (l[1][0] << 24), (l[1][0] >> 40) | (l[1][1] << 24) | (l[2][0] << 48), (l[2][0] >> 16) | (l[2][1] << 48)};
  if (!lt4(v, fq().p)) return 2;
  to_mont(fq(), v, mont);
  return 0;
}

ZK_LIMBS_HD bool on_curve(const uint64_t x[4], const uint64_t y[4]) {      // Montgomery words, canonical; (0, 0) is not
  const uint64_t three[4] = {0x7a17caa950ad28d7ull, 0x1f6ac17ae15521b9ull, 0x334bea4e696bd284ull, 0x2a1f6744ce179d8eull};      // 3 * 2^256 mod q
  uint64_t yy[4], xx[4], xxx[4];
  mont_mul(fq(), y, y, yy);
  mont_mul(fq(), x, x, xx);
  mont_mul(fq(), xx, x, xxx);
  unsigned __int128 c = 0;                                          // xxx + 3, reduced once (both below q)
  uint64_t s[4], d[4];
  for (int j = 0; j < 4; j++) { c += (unsigned __int128)xxx[j] + three[j]; s[j] = (uint64_t)c; c >>= 64; }
  unsigned __int128 borrow = 0;
  for (int j = 0; j < 4; j++) { const unsigned __int128 t = (unsigned __int128)s[j] - fq().p[j] - (uint64_t)borrow; d[j] = (uint64_t)t; borrow = (t >> 64) & 1; }
  const bool keep = c == 0 && borrow;
  bool same = true;
  for (int j = 0; j < 4; j++) same &= yy[j] == (keep ? s[j] : d[j]);
  return same;
}

ZK_LIMBS_HD void encode_point(const uint64_t* affine, uint64_t* fr_out) {
  encode_coordinate(affine, fr_out);
  encode_coordinate(affine + 4, fr_out + 12);
}

ZK_LIMBS_HD uint32_t decode_point(const uint64_t* fr_in, uint64_t* affine) {
  uint32_t st = decode_coordinate(fr_in, affine);
  if (st == 0) st = decode_coordinate(fr_in + 12, affine + 4);
  if (st == 0 && !on_curve(affine, affine + 4)) st = 3;
  if (st != 0)
    for (int j = 0; j < 8; j++) affine[j] = 0;
  return st;
}

}  // namespace kzg_limbs
}  // namespace zkhip

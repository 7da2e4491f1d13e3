// RFC 9380 hash_to_curve, suite secp256k1_XMD:SHA-256_SSWU_RO_, and the PLUME check built on it (include/zkhip.h, "PLUME nullifiers on
// secp256k1"): H(msg, pk) = hash_to_curve(msg || compress(pk)) with the DST below, as `hash_to_curve` of the reference's
// voter_tests/src/lib.rs:36-55 asks it of the k256 crate.
//
//   h2c_prefix            what a batch shares, built once on the host (h2c_prefix_build, byte by byte): `expand_message_xmd` hashes
//                         Z_pad || msg || compress(pk) || 00 60 00 || DST'.  Z_pad is a block of zeros, so the state behind it is a constant; the rest
//                         is at most three blocks, laid out with 33 zero bytes where the voter's key goes, padding and length included.  The blocks
//                         of b_i = SHA-256(x || i || DST') behind their first eight words are constant too.
//   h2c_hash_to_field     the voter's part: the key's 33 bytes are shifted to byte msg_len -- a shift that is uniform over a batch, done with
//                         funnel shifts and conditional moves, so that no array is indexed at run time -- then b_0 .. b_3 and the two 48-byte
//                         values mod p.
//   h2c_map               simplified SWU on E' (section 6.6.2, both exceptional cases: a zero denominator takes x1 = B' / (Z A')), then the
//                         3-isogeny, whose result stays projective: x = xn / xd and y = y' yn / yd are (xn yd : y' yn xd : xd yd), no inversion.  A zero
//                         isogeny denominator gives the identity.
//   h2c_hash              the sum of the two images, affine: one inversion.
//   plume_challenge       SHA-256 of the six compressed points, 198 bytes at fixed offsets.
//   plume_verdict         the whole check of one voter in one thread; the kernel splits the same pieces over two lanes.
//   plume_sign            `gen_test_nullifier` of one voter in one thread: four single-scalar ladders, H, the challenge mod n, s = r + sk c mod n;
//                         the kernel (plume_sign.hip) splits the ladders over two lanes and shares plume_sign_finish.
//
// Host and device code; plain g++ compiles it (tests/cpp/secp256k1_host_check.cpp).
#pragma once
#include "secp256k1.hpp"
#include "sha256.hpp"

namespace zkhip {

constexpr int H2C_MAX_MSG = 64;        // ZKHIP_PLUME_MAX_MSG
constexpr int H2C_DST_LEN = 49;

struct h2c_prefix {
  uint32_t mid[8];                     // the SHA-256 state behind the block of zeros
  uint32_t m[48];                      // msg || 33 zero bytes || 00 60 00 || DST' || padding, big-endian words
  uint32_t tail[24];                   // words 8 .. 31 of x || i || DST' || padding, the byte i left zero
  uint32_t len;                        // msg_len: where the key goes
  uint32_t blocks;                     // 1 to 3 blocks of m
  uint32_t keyed;                      // 1: the key's 33 bytes follow msg; 0: msg alone is hashed (the RFC's own vectors; the host check only)
};

inline void h2c_put_byte(uint32_t* m, size_t at, uint32_t byte) { m[at >> 2] |= byte << (24 - 8 * (at & 3)); }
// host only.  msg_len <= H2C_MAX_MSG.
inline void h2c_prefix_build(const uint8_t* msg, size_t msg_len, h2c_prefix* p, bool keyed = true) {
  static const char dst[H2C_DST_LEN + 1] = "QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_";
  uint32_t zeros[16] = {0};
  sha256_init(p->mid);
  sha256_block(p->mid, zeros);
  for (int i = 0; i < 48; i++) p->m[i] = 0;
  for (int i = 0; i < 24; i++) p->tail[i] = 0;
  size_t at = 0;
  for (size_t i = 0; i < msg_len; i++) h2c_put_byte(p->m, at++, msg[i]);
  if (keyed) at += 33;
  p->keyed = keyed ? 1u : 0u;
  h2c_put_byte(p->m, at++, 0);
  h2c_put_byte(p->m, at++, 96);                               // len_in_bytes = 96, two bytes
  h2c_put_byte(p->m, at++, 0);
  for (int i = 0; i < H2C_DST_LEN; i++) h2c_put_byte(p->m, at++, (uint8_t)dst[i]);
  h2c_put_byte(p->m, at++, H2C_DST_LEN);
  h2c_put_byte(p->m, at, 0x80);
  p->len = (uint32_t)msg_len;
  p->blocks = (uint32_t)((at + 9 + 63) / 64);
  p->m[16 * p->blocks - 1] = (uint32_t)((64 + at) * 8);
  at = 1;                                                     // behind the byte i, which is byte 32 of the message and byte 0 of the tail
  for (int i = 0; i < H2C_DST_LEN; i++) h2c_put_byte(p->tail, at++, (uint8_t)dst[i]);
  h2c_put_byte(p->tail, at++, H2C_DST_LEN);
  h2c_put_byte(p->tail, at, 0x80);
  p->tail[23] = (32 + 1 + H2C_DST_LEN + 1) * 8;
}

// b_i = SHA-256(x || i || DST'), two blocks
SK_HD void h2c_b(const h2c_prefix& pre, const uint32_t x[8], uint32_t i, uint32_t out[8]) {
  uint32_t m[32];
#pragma unroll
  for (int k = 0; k < 8; k++) m[k] = x[k];
#pragma unroll
  for (int k = 0; k < 24; k++) m[8 + k] = pre.tail[k];
  m[8] |= i << 24;
  sha256_init(out);
  sha256_block(out, m);
  sha256_block(out, m + 16);
}

// twelve big-endian words (48 bytes) -> the integer mod p
SK_HD sk_fe h2c_os2ip_mod_p(const uint32_t* hi8, const uint32_t* lo4, bool hi_first) {
  uint32_t be[12], t[16];
#pragma unroll
  for (int k = 0; k < 12; k++) be[k] = hi_first ? (k < 8 ? hi8[k] : lo4[k - 8]) : (k < 4 ? lo4[k] : hi8[k - 4]);
#pragma unroll
  for (int k = 0; k < 16; k++) t[k] = k < 12 ? be[11 - k] : 0u;
  return sk_reduce512(t);
}

// the two field elements of hash_to_field(msg || compress(pk), 2)
SK_HD void h2c_hash_to_field(const h2c_prefix& pre, const sk_aff& pk, sk_fe& u0, sk_fe& u1) {
  uint32_t c[9], s[10];
  sk_compress(pk, c);
  const uint32_t r = 8u * (pre.len & 3u), q = pre.len >> 2;   // uniform over the batch
#pragma unroll
  for (int j = 0; j < 10; j++) {
    const uint32_t cur = j < 9 ? c[j] : 0u, prev = j > 0 ? c[j - 1] : 0u;
    s[j] = !pre.keyed ? 0u : r ? (cur >> r) | (prev << (32u - r)) : cur;
  }
  uint32_t m[48];
#pragma unroll
  for (int w = 0; w < 48; w++) {
    uint32_t v = 0;
    if (w < H2C_MAX_MSG / 4 + 10) {                           // q <= 16: the key reaches no later word
#pragma unroll
      for (int j = 0; j < 10; j++)
        if (w - j >= 0) v = ((uint32_t)(w - j) == q) ? s[j] : v;
    }
    m[w] = pre.m[w] | v;
  }
  uint32_t b0[8], b[8], x[8], uni[24];
#pragma unroll
  for (int k = 0; k < 24; k++) uni[k] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) b0[k] = pre.mid[k];
  sha256_block(b0, m);
  if (pre.blocks >= 2) sha256_block(b0, m + 16);
  if (pre.blocks == 3) sha256_block(b0, m + 32);
#pragma unroll
  for (int k = 0; k < 8; k++) b[k] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t i = 1; i <= 3; i++) {
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = b0[k] ^ b[k];          // b_1 hashes b_0 itself: b starts as zeros
    h2c_b(pre, x, i, b);
#pragma unroll
    for (int k = 0; k < 8; k++) {                             // uni[8 (i - 1) + k] = b[k] without an index that runs
      uni[k] = i == 1 ? b[k] : uni[k];
      uni[8 + k] = i == 2 ? b[k] : uni[8 + k];
      uni[16 + k] = i == 3 ? b[k] : uni[16 + k];
    }
  }
  u0 = h2c_os2ip_mod_p(uni, uni + 8, true);                   // bytes 0 .. 47: b_1, half of b_2
  u1 = h2c_os2ip_mod_p(uni + 16, uni + 12, false);            // bytes 48 .. 95: the other half, b_3
}

// E': y^2 = x^3 + A' x + B', Z = -11
SK_HD sk_fe h2c_iso_a() { return sk_const(0x3f8731abdd661adcull, 0xa08a5558f0f5d272ull, 0xe953d363cb6f0e5dull, 0x405447c01a444533ull); }
SK_HD sk_fe h2c_g(const sk_fe& x) { return sk_add(sk_mul(sk_add(sk_sqr(x), h2c_iso_a()), x), sk_small(1771)); }

// simplified SWU: u -> (x', y') on E'
SK_HD sk_aff h2c_sswu(const sk_fe& u) {
  const sk_fe c1 = sk_const(0x0bc56cee718538b2ull, 0xa00c4df5d3e87b0cull, 0x6df4ff98e82d74fdull, 0xaa01d58e8d2345c3ull);   // -B' / A'
  const sk_fe b_za = sk_const(0xbb407e4438dd90caull, 0x6ba4071659152275ull, 0x7e5c173c7232ad8bull, 0x6c8bcd97de490391ull);  // B' / (Z A')
  const sk_fe zu2 = sk_neg(sk_mul_small(sk_sqr(u), 11));      // Z u^2
  const sk_fe tv1 = sk_add(sk_sqr(zu2), zu2);                 // Z^2 u^4 + Z u^2
  const sk_fe x1 = sk_sel(sk_is_zero(tv1), b_za, sk_mul(c1, sk_add(sk_small(1), sk_inv(tv1))));
  const sk_fe gx1 = h2c_g(x1);
  sk_aff r;
  r.x = x1;
  r.y = sk_sqrt(gx1);
  if (!sk_eq(sk_sqr(r.y), gx1)) {                             // gx1 is no square: then gx2 is one
    r.x = sk_mul(zu2, x1);
    r.y = sk_sqrt(h2c_g(r.x));
  }
  if (sk_is_odd(u) != sk_is_odd(r.y)) r.y = sk_neg(r.y);      // sgn0(y) = sgn0(u)
  return r;
}

// the 3-isogeny E' -> secp256k1 (RFC 9380 appendix E.1), projective
SK_HD sk_pt h2c_iso(const sk_aff& a) {
  const sk_fe& x = a.x;
  sk_fe xn = sk_const(0x8e38e38e38e38e38ull, 0xe38e38e38e38e38eull, 0x38e38e38e38e38e3ull, 0x8e38e38daaaaa88cull);
  xn = sk_add(sk_mul(xn, x), sk_const(0x534c328d23f234e6ull, 0xe2a413deca25caecull, 0xe4506144037c4031ull, 0x4ecbd0b53d9dd262ull));
  xn = sk_add(sk_mul(xn, x), sk_const(0x07d3d4c80bc321d5ull, 0xb9f315cea7fd44c5ull, 0xd595d2fc0bf63b92ull, 0xdfff1044f17c6581ull));
  xn = sk_add(sk_mul(xn, x), sk_const(0x8e38e38e38e38e38ull, 0xe38e38e38e38e38eull, 0x38e38e38e38e38e3ull, 0x8e38e38daaaaa8c7ull));
  sk_fe xd = sk_add(x, sk_const(0xedadc6f64383dc1dull, 0xf7c4b2d51b542254ull, 0x06d36b641f5e41bbull, 0xc52a56612a8c6d14ull));
  xd = sk_add(sk_mul(xd, x), sk_const(0xd35771193d94918aull, 0x9ca34ccbb7b640ddull, 0x86cd409542f8487dull, 0x9fe6b745781eb49bull));
  sk_fe yn = sk_const(0x2f684bda12f684bdull, 0xa12f684bda12f684ull, 0xbda12f684bda12f6ull, 0x84bda12f38e38d84ull);
  yn = sk_add(sk_mul(yn, x), sk_const(0x29a6194691f91a73ull, 0x715209ef6512e576ull, 0x722830a201be2018ull, 0xa765e85a9ecee931ull));
  yn = sk_add(sk_mul(yn, x), sk_const(0xc75e0c32d5cb7c0full, 0xa9d0a54b12a0a6d5ull, 0x647ab046d686da6full, 0xdffc90fc201d71a3ull));
  yn = sk_add(sk_mul(yn, x), sk_const(0x4bda12f684bda12full, 0x684bda12f684bda1ull, 0x2f684bda12f684bdull, 0xa12f684b8e38e23cull));
  sk_fe yd = sk_add(x, sk_const(0x6484aa716545ca2cull, 0xf3a70c3fa8fe337eull, 0x0a3d21162f0d6299ull, 0xa7bf8192bfd2a76full));
  yd = sk_add(sk_mul(yd, x), sk_const(0x7a06534bb8bdb49full, 0xd5e9e6632722c298ull, 0x9467c1bfc8e8d978ull, 0xdfb425d2685c2573ull));
  yd = sk_add(sk_mul(yd, x), sk_const(0xffffffffffffffffull, 0xffffffffffffffffull, 0xffffffffffffffffull, 0xfffffffefffff93bull));
  sk_pt r;
  r.Z = sk_mul(xd, yd);
  const bool id = sk_is_zero(r.Z);
  r.X = sk_sel(id, sk_small(0), sk_mul(xn, yd));
  r.Y = sk_sel(id, sk_small(1), sk_mul(sk_mul(a.y, yn), xd));
  return r;
}
SK_HD sk_pt h2c_map(const sk_fe& u) { return h2c_iso(h2c_sswu(u)); }

// H(msg, pk), affine
SK_HD sk_aff h2c_hash(const h2c_prefix& pre, const sk_aff& pk) {
  sk_fe u0, u1;
  h2c_hash_to_field(pre, pk, u0, u1);
  return sk_to_affine(sk_padd(h2c_map(u0), h2c_map(u1)));
}

// d = SHA-256(compress(G) || compress(pk) || compress(H) || compress(N) || compress(A) || compress(B)), eight big-endian words
SK_HD void plume_challenge(const sk_aff& pk, const sk_aff& h, const sk_aff& nullifier, const sk_aff& a, const sk_aff& b, uint32_t d[8]) {
  uint32_t m[64], piece[9];
#pragma unroll
  for (int k = 0; k < 64; k++) m[k] = 0;
  sk_compress(sk_generator(), piece); sha256_put33<0>(m, piece);
  sk_compress(pk, piece);             sha256_put33<33>(m, piece);
  sk_compress(h, piece);              sha256_put33<66>(m, piece);
  sk_compress(nullifier, piece);      sha256_put33<99>(m, piece);
  sk_compress(a, piece);              sha256_put33<132>(m, piece);
  sk_compress(b, piece);              sha256_put33<165>(m, piece);
  sha256_pad<198, 64>(m);
  sha256_init(d);
  sha256_block(d, m);
  sha256_block(d, m + 16);
  sha256_block(d, m + 32);
  sha256_block(d, m + 48);
}
// the digest read as a big-endian integer equals c
SK_HD bool plume_challenge_is(const sk_aff& pk, const sk_aff& h, const sk_aff& nullifier, const sk_aff& a, const sk_aff& b, const sk_fe& c) {
  uint32_t d[8], diff = 0;
  plume_challenge(pk, h, nullifier, a, b, d);
#pragma unroll
  for (int k = 0; k < 8; k++) diff |= d[k] ^ c.l[7 - k];
  return diff == 0;
}

constexpr uint32_t PLUME_OK = 0, PLUME_REFUSED = 1, PLUME_MALFORMED = 2;

SK_HD bool plume_well_formed(const sk_aff& pk, const sk_aff& nullifier, const sk_fe& s, const sk_fe& c) {
  return sk_on_curve(pk) && sk_on_curve(nullifier) && sk_scalar_ok(s) && sk_scalar_ok(c);
}

// `verify_nullifier` of one voter: A = s G - c pk, B = s H - c N, accept iff the challenge of (pk, H, N, A, B) is c.  h_out: H(msg, pk), or
// (0, 0) where pk is malformed.
SK_HD uint32_t plume_verdict(const h2c_prefix& pre, const sk_aff& pk, const sk_aff& nullifier, const sk_fe& s, const sk_fe& c, sk_aff* h_out) {
  const bool pk_ok = sk_on_curve(pk);
  if (!pk_ok) {
    if (h_out) h_out->x = h_out->y = sk_small(0);
    return PLUME_MALFORMED;
  }
  const sk_aff h = h2c_hash(pre, pk);
  if (h_out) *h_out = h;
  if (!plume_well_formed(pk, nullifier, s, c)) return PLUME_MALFORMED;
  const sk_aff a = sk_lincomb(s, sk_generator(), c, sk_neg_affine(pk));
  const sk_aff b = sk_lincomb(s, h, c, sk_neg_affine(nullifier));
  return plume_challenge_is(pk, h, nullifier, a, b, c) ? PLUME_OK : PLUME_REFUSED;
}

// what `gen_test_nullifier` returns, and H(msg, pk) beside it
struct plume_signature {
  sk_aff pk, nullifier, h;
  sk_fe s, c;
};
// sk, r in [1, n)
SK_HD bool plume_secret_ok(const sk_fe& k) { return !sk_is_zero(k) && sk_scalar_ok(k); }
// the last step, given the four ladder results: c = SHA-256(..) mod n, s = r + sk c mod n
SK_HD void plume_sign_finish(const sk_fe& sk, const sk_fe& r, const sk_aff& rg, const sk_aff& rh, plume_signature& o) {
  uint32_t d[8];
  plume_challenge(o.pk, o.h, o.nullifier, rg, rh, d);
  o.c = sk_scalar_from_digest(d);
  o.s = sk_scalar_muladd(sk, o.c, r);
}
// `gen_test_nullifier` of one voter in one thread, r in place of `Fq::random`; the kernel splits the same pieces over two lanes.  A malformed
// sk or r gives PLUME_MALFORMED and zeros.
SK_HD uint32_t plume_sign(const h2c_prefix& pre, const sk_fe& sk, const sk_fe& r, plume_signature* o) {
  if (!plume_secret_ok(sk) || !plume_secret_ok(r)) {
    o->pk.x = o->pk.y = o->nullifier.x = o->nullifier.y = o->h.x = o->h.y = o->s = o->c = sk_small(0);
    return PLUME_MALFORMED;
  }
  const sk_aff g = sk_generator();
  o->pk = sk_to_affine(sk_mul_proj(sk, g));
  o->h = h2c_hash(pre, o->pk);
  o->nullifier = sk_to_affine(sk_mul_proj(sk, o->h));
  plume_sign_finish(sk, r, sk_to_affine(sk_mul_proj(r, g)), sk_to_affine(sk_mul_proj(r, o->h)), *o);
  return PLUME_OK;
}

}  // namespace zkhip

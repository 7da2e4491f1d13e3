// The library's random Fr stream, one element per index (include/zkhip.h, "random field elements", is the contract).
//
// Element i of stream (seed, stream_id): one ChaCha20 block (20 rounds, the original layout with a 64-bit block counter) with
//   words 0..3 "expand 32-byte k" | words 4..11 the 32 seed bytes as little-endian u32 | words 12, 13 = i (low, high) |
//   words 14, 15 = stream_id (low, high);
// its 64 output bytes read as a little-endian 512-bit integer x; the element is x mod r, stored as 4 x u64 Montgomery-256, canonical.
// One block gives one element, so an element depends on (seed, stream_id, i) alone: any launch geometry, any split into calls, any
// device computes the same column.
//
// The reduction: x = lo + hi 2^256 with lo, hi < 2^256 unpacked as they are (fe_unpack<0>: limbs 0..7 < 2^29, limb 8 < 2^24), and ONE
// fe_mul_add gives (lo 2^517 + hi 2^773) 2^-261 = x 2^256 mod r, the stored form, directly.  Bounds (fp29.hpp): all four operands have
// limbs < 2^29, so a column holds at most 9 (2^58 + 2^58) + 9 2^58 = 27 2^58 < 2^64; lo 2^517' + hi 2^773' < 2 * 2^256 r, so the value is
// below r (2^257 / 2^261 + 1) < 1.07 r and one conditional subtraction makes it canonical.
#pragma once
#include "fp29.hpp"

namespace zkhip {

struct fr_random_key {   // the 32 seed bytes as the eight little-endian key words; passed to the kernels by value
  uint32_t w[8];
};

ZK_HD fr_random_key fr_random_key_from_seed(const uint8_t seed[32]) {
  fr_random_key k;
  for (int i = 0; i < 8; i++)
    k.w[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) | ((uint32_t)seed[4 * i + 3] << 24);
  return k;
}

ZK_HD uint32_t chacha_rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }

#define ZK_CHACHA_QR(a, b, c, d)                     \
  do {                                               \
    a += b; d ^= a; d = chacha_rotl(d, 16);          \
    c += d; b ^= c; b = chacha_rotl(b, 12);          \
    a += b; d ^= a; d = chacha_rotl(d, 8);           \
    c += d; b ^= c; b = chacha_rotl(b, 7);           \
  } while (0)

// the 16 output words of the block (key, counter, stream_id)
ZK_HD void chacha20_block(const fr_random_key& key, uint64_t counter, uint64_t stream_id, uint32_t (&out)[16]) {
  const uint32_t i0 = 0x61707865u, i1 = 0x3320646eu, i2 = 0x79622d32u, i3 = 0x6b206574u;   // "expand 32-byte k"
  const uint32_t i12 = (uint32_t)counter, i13 = (uint32_t)(counter >> 32), i14 = (uint32_t)stream_id, i15 = (uint32_t)(stream_id >> 32);
  uint32_t x0 = i0, x1 = i1, x2 = i2, x3 = i3;
  uint32_t x4 = key.w[0], x5 = key.w[1], x6 = key.w[2], x7 = key.w[3], x8 = key.w[4], x9 = key.w[5], x10 = key.w[6], x11 = key.w[7];
  uint32_t x12 = i12, x13 = i13, x14 = i14, x15 = i15;
#pragma unroll
  for (int r = 0; r < 10; r++) {   // ten double rounds: four column rounds, four diagonal rounds
    ZK_CHACHA_QR(x0, x4, x8, x12);
    ZK_CHACHA_QR(x1, x5, x9, x13);
    ZK_CHACHA_QR(x2, x6, x10, x14);
    ZK_CHACHA_QR(x3, x7, x11, x15);
    ZK_CHACHA_QR(x0, x5, x10, x15);
    ZK_CHACHA_QR(x1, x6, x11, x12);
    ZK_CHACHA_QR(x2, x7, x8, x13);
    ZK_CHACHA_QR(x3, x4, x9, x14);
  }
  out[0] = x0 + i0; out[1] = x1 + i1; out[2] = x2 + i2; out[3] = x3 + i3;
  out[4] = x4 + key.w[0]; out[5] = x5 + key.w[1]; out[6] = x6 + key.w[2]; out[7] = x7 + key.w[3];
  out[8] = x8 + key.w[4]; out[9] = x9 + key.w[5]; out[10] = x10 + key.w[6]; out[11] = x11 + key.w[7];
  out[12] = x12 + i12; out[13] = x13 + i13; out[14] = x14 + i14; out[15] = x15 + i15;
}
#undef ZK_CHACHA_QR

// element `index` of stream (key, stream_id) as the eight 32-bit words of its stored form
ZK_HD void fr_random_element(const fr_random_key& key, uint64_t stream_id, uint64_t index, uint32_t (&w)[8]) {
  uint32_t blk[16], lo[8], hi[8];
  chacha20_block(key, index, stream_id, blk);
#pragma unroll
  for (int i = 0; i < 8; i++) { lo[i] = blk[i]; hi[i] = blk[8 + i]; }
  const fe r = fe_mul_add<FrParams>(fe_unpack<0>(lo), fe_const<FrParams>(FrParams::RAND_LO), fe_unpack<0>(hi), fe_const<FrParams>(FrParams::RAND_HI));
  fe_pack(fe_canon_lt2p<FrParams>(r), w);
}

}  // namespace zkhip

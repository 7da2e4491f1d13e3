// SHA-256 (FIPS 180-4) over a byte string assembled in registers, for the PLUME check (plume.hip): the 198-byte challenge and the blocks of
// `expand_message_xmd`.  A message is an array of big-endian 32-bit words, sixteen per block, with the padding already in it; the caller places
// its pieces at offsets known when the code is compiled, so every index below is a constant once the loops are unrolled and nothing goes to
// scratch.  sha256_pad writes the 0x80 byte and the bit length.  The 33-byte pieces are compressed points (secp256k1.hpp sk_compress).
//
// Host and device code, plain g++ compiles it (tests/cpp/secp256k1_host_check.cpp, which also hashes byte strings of any length through
// sha256_bytes -- host only, it indexes at run time).
#pragma once
#include <cstdint>
#include <cstddef>

#if defined(__HIPCC__)
#define SHA_HD __host__ __device__ __forceinline__
#else
#define SHA_HD inline
#endif

namespace zkhip {

SHA_HD uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

SHA_HD void sha256_init(uint32_t h[8]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

// one block: sixteen big-endian words into the state.  The schedule rolls over sixteen registers.
SHA_HD void sha256_block(uint32_t h[8], const uint32_t* m) {
  const uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
      0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
      0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
      0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = m[i];
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      w[i & 15] += (sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10));
    }
    const uint32_t t1 = hh + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
    const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// the 0x80 byte behind BYTES bytes of message and the bit length of TOTAL bytes in the last two words of the WORDS-word buffer (TOTAL counts
// blocks hashed before this buffer too); the rest of the buffer is the caller's zeros
template <int BYTES, int WORDS, int TOTAL = BYTES>
SHA_HD void sha256_pad(uint32_t* m) {
  static_assert(WORDS % 16 == 0 && BYTES + 9 <= WORDS * 4, "the padding fits the last block");
  m[BYTES >> 2] |= 0x80u << (24 - 8 * (BYTES & 3));
  m[WORDS - 1] = (uint32_t)TOTAL * 8u;
}

// the 33 bytes of c (nine big-endian words, the last one byte) ORed into m at byte offset OFF, a constant
template <int OFF>
SHA_HD void sha256_put33(uint32_t* m, const uint32_t c[9]) {
  constexpr int q = OFF >> 2, r = 8 * (OFF & 3);
#pragma unroll
  for (int j = 0; j < 9; j++) {
    m[q + j] |= c[j] >> r;
    if (r != 0 && (j < 8 || r > 24)) m[q + j + 1] |= c[j] << ((32 - r) & 31);
  }
}

// host only: any byte string.  out: the digest as eight big-endian words.
inline void sha256_bytes(const uint8_t* data, size_t len, uint32_t out[8]) {
  sha256_init(out);
  const size_t blocks = (len + 9 + 63) / 64;
  for (size_t b = 0; b < blocks; b++) {
    uint32_t m[16] = {0};
    for (size_t k = 0; k < 64; k++) {
      const size_t at = b * 64 + k;
      const uint32_t byte = at < len ? data[at] : at == len ? 0x80u : 0u;
      m[k >> 2] |= byte << (24 - 8 * (k & 3));
    }
    if (b + 1 == blocks) {
      m[14] = (uint32_t)(((uint64_t)len * 8) >> 32);
      m[15] = (uint32_t)((uint64_t)len * 8);
    }
    sha256_block(out, m);
  }
}

}  // namespace zkhip

// Blake2b (RFC 7693), unkeyed, with a 16-byte personalisation: the hash under halo2's `Blake2bWrite` / `Blake2bRead` transcripts
// [DEP halo2-axiom transcript.rs: `Blake2bParams::new().hash_length(64).personal(b"Halo2-Transcript")`; the reference reaches it through
// `gen_proof`, /root/reference/aggregator/benches/wrapper_circuit.rs:140].  Host code only: the compression function is a serial chain of
// 128-byte blocks, and a proof absorbs on the order of 100 KB -- see DESIGN.md section 4b for why it is not a kernel.
//
// Streaming: `update` keeps the last (possibly full) block in the buffer, because the final block is compressed with the finalisation flag and
// a message that ends on a block boundary has a FULL final block.  `digest` finalises a copy, so a state can be squeezed and go on.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace zkhip {

struct blake2b {
  uint64_t h[8];
  uint64_t t[2];
  uint8_t buf[128];
  size_t buflen;

  static inline uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
  static inline uint64_t load64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
    return v;
  }

  // digest_len 1..64, no key, fanout = depth = 1, `person`: 16 bytes or null
  void init(unsigned digest_len, const uint8_t* person) {
    static const uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                   0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= 0x01010000ULL ^ (uint64_t)digest_len;          // parameter block bytes 0..3: digest length, key length 0, fanout 1, depth 1
    if (person) { h[6] ^= load64(person); h[7] ^= load64(person + 8); }   // parameter block bytes 48..63
    t[0] = t[1] = 0;
    buflen = 0;
    std::memset(buf, 0, sizeof(buf));
  }

  void compress(const uint8_t block[128], bool last) {
    static const uint8_t SIGMA[12][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
    static const uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                   0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    uint64_t m[16], v[16];
    for (int i = 0; i < 16; i++) m[i] = load64(block + 8 * i);
    for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = IV[i]; }
    v[12] ^= t[0];
    v[13] ^= t[1];
    if (last) v[14] = ~v[14];
#define ZK_B2B_G(a, b, c, d, x, y)                                   \
  do {                                                               \
    v[a] = v[a] + v[b] + (x); v[d] = rotr(v[d] ^ v[a], 32);          \
    v[c] = v[c] + v[d];       v[b] = rotr(v[b] ^ v[c], 24);          \
    v[a] = v[a] + v[b] + (y); v[d] = rotr(v[d] ^ v[a], 16);          \
    v[c] = v[c] + v[d];       v[b] = rotr(v[b] ^ v[c], 63);          \
  } while (0)
    for (int r = 0; r < 12; r++) {
      const uint8_t* s = SIGMA[r];
      ZK_B2B_G(0, 4, 8, 12, m[s[0]], m[s[1]]);
      ZK_B2B_G(1, 5, 9, 13, m[s[2]], m[s[3]]);
      ZK_B2B_G(2, 6, 10, 14, m[s[4]], m[s[5]]);
      ZK_B2B_G(3, 7, 11, 15, m[s[6]], m[s[7]]);
      ZK_B2B_G(0, 5, 10, 15, m[s[8]], m[s[9]]);
      ZK_B2B_G(1, 6, 11, 12, m[s[10]], m[s[11]]);
      ZK_B2B_G(2, 7, 8, 13, m[s[12]], m[s[13]]);
      ZK_B2B_G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
#undef ZK_B2B_G
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
  }

  void add_count(uint64_t n) {
    t[0] += n;
    if (t[0] < n) t[1]++;
  }

  void update(const uint8_t* in, size_t len) {
    while (len) {
      if (buflen == 128) {               // more input follows: the buffered block is not the last one
        add_count(128);
        compress(buf, false);
        buflen = 0;
      }
      const size_t take = len < 128 - buflen ? len : 128 - buflen;
      std::memcpy(buf + buflen, in, take);
      buflen += take;
      in += take;
      len -= take;
    }
  }

  // finalises a COPY: the state itself goes on absorbing
  void digest(uint8_t* out, unsigned digest_len) const {
    blake2b c = *this;
    c.add_count(c.buflen);
    std::memset(c.buf + c.buflen, 0, 128 - c.buflen);
    c.compress(c.buf, true);
    for (unsigned i = 0; i < digest_len; i++) out[i] = (uint8_t)(c.h[i >> 3] >> (8 * (i & 7)));
  }
};

}  // namespace zkhip

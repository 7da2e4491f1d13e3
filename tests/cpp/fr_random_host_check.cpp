// Host build of csrc/fr_random.hpp (the per-element function the device kernels call), run under ASan + UBSan by tests/test_fr_random_host.py.
// stdin: one request per line, "<seed: 64 hex digits> <stream_id hex> <first hex> <n decimal>".
// stdout: first "C <2^517 mod r> <2^773 mod r>" as the header's limb arrays spell them (hex integers), then for every request its n elements,
// one per line, as the 256-bit number the four stored u64 words make (64 hex digits, most significant first).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fr_random.hpp"

using namespace zkhip;

static void print_limbs(const uint32_t (&l)[NL]) {   // 9 x 29-bit limbs -> hex integer (261 bits: 66 digits)
  unsigned __int128 acc = 0;
  int bits = 0;
  char digits[80];
  int nd = 0;
  for (int i = 0; i < NL; i++) {
    acc |= (unsigned __int128)l[i] << bits;
    bits += LB;
    while (bits >= 4) { digits[nd++] = "0123456789abcdef"[(unsigned)(acc & 15)]; acc >>= 4; bits -= 4; }
  }
  if (bits) digits[nd++] = "0123456789abcdef"[(unsigned)(acc & 15)];
  for (int i = nd - 1; i >= 0; i--) putchar(digits[i]);
}

int main() {
  printf("C ");
  print_limbs(FrParams::RAND_LO);
  putchar(' ');
  print_limbs(FrParams::RAND_HI);
  putchar('\n');
  char seed_hex[128];
  uint64_t stream_id, first;
  unsigned long n;
  while (scanf("%64s %" SCNx64 " %" SCNx64 " %lu", seed_hex, &stream_id, &first, &n) == 4) {
    if (strlen(seed_hex) != 64) { fprintf(stderr, "bad seed\n"); return 2; }
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) {
      unsigned v;
      if (sscanf(seed_hex + 2 * i, "%2x", &v) != 1) { fprintf(stderr, "bad seed\n"); return 2; }
      seed[i] = (uint8_t)v;
    }
    const fr_random_key key = fr_random_key_from_seed(seed);
    for (unsigned long j = 0; j < n; j++) {
      uint32_t w[8];
      fr_random_element(key, stream_id, first + j, w);
      for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
      putchar('\n');
    }
  }
  return 0;
}

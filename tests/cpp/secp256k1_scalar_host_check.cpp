// The scalars mod n of csrc/secp256k1.hpp compiled for the host (tests/test_secp256k1_scalar_host.py builds this under ASan + UBSan): one command
// per line of standard input, values in hex, one line of results each; the test compares every value with Python's `%`.
//   red T            -> T mod n                                    (T any integer below 2^512)
//   ops a b c        -> a b + c, a b, a + b, a mod n, all mod n    (any 256-bit a, b, c)
//   dig D            -> the digest D (64 hex digits, as SHA-256 prints it) read big-endian, mod n
//   sign MSGHEX|- sk r -> status, pk, N, s, c, H                   (plume_sign, the host form of the kernel)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "secp256k1_h2c.hpp"

using namespace zkhip;

// up to `words` 32-bit words from a hex string, little-endian
static void parse(const std::string& hex, uint32_t* out, int words) {
  for (int i = 0; i < words; i++) out[i] = 0;
  int nib = 0;
  for (size_t i = hex.size(); i-- > 0 && nib < 8 * words; nib++) {
    const char ch = hex[i];
    const uint32_t v = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    out[nib / 8] |= v << (4 * (nib % 8));
  }
}
static sk_fe parse(const std::string& hex) {
  sk_fe r;
  parse(hex, r.l, 8);
  return r;
}
static void put(const sk_fe& a) {
  for (int i = 7; i >= 0; i--) std::printf("%08x", a.l[i]);
  std::printf(" ");
}

int main() {
  std::string line;
  size_t done = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    std::vector<std::string> w;
    in >> op;
    for (std::string t; in >> t;) w.push_back(t);
    if (op == "red") {
      uint32_t t[16];
      parse(w.at(0), t, 16);
      put(sk_scalar_reduce512(t));
    } else if (op == "ops") {
      const sk_fe a = parse(w.at(0)), b = parse(w.at(1)), c = parse(w.at(2));
      put(sk_scalar_muladd(a, b, c)); put(sk_scalar_mul(a, b)); put(sk_scalar_add(a, b)); put(sk_scalar_reduce(a));
    } else if (op == "dig") {
      uint32_t le[8], d[8];
      parse(w.at(0), le, 8);
      for (int i = 0; i < 8; i++) d[i] = le[7 - i];           // word 0 of a digest is its most significant
      put(sk_scalar_from_digest(d));
    } else if (op == "sign") {
      std::vector<uint8_t> msg;
      if (w.at(0) != "-")
        for (size_t i = 0; i + 1 < w[0].size(); i += 2) msg.push_back((uint8_t)std::stoul(w[0].substr(i, 2), nullptr, 16));
      h2c_prefix pre;
      h2c_prefix_build(msg.data(), msg.size(), &pre);
      plume_signature sig;
      const uint32_t status = plume_sign(pre, parse(w.at(1)), parse(w.at(2)), &sig);
      std::printf("%u ", status);
      put(sig.pk.x); put(sig.pk.y); put(sig.nullifier.x); put(sig.nullifier.y); put(sig.s); put(sig.c); put(sig.h.x); put(sig.h.y);
    } else {
      std::printf("unknown command");
    }
    std::printf("\n");
    done++;
  }
  std::printf("secp256k1 scalar host check done: %zu lines\n", done);
  return 0;
}

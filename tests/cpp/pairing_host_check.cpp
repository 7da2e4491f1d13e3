// Host driver of tests/test_pairing_host.py: csrc/pairing.hpp through its single-lane policy, built with the host compiler under ASan + UBSan.
// stdin, one request per line (hex = the little-endian bytes of the Montgomery-256 words):
//   O <op> <a: 384 bytes> <b: 384 bytes>      -> one tower operation (pairing_test_op), prints 384 bytes
//   V <n> <g1: n * 64 bytes | -> <g2: n * 128 bytes | ->   -> the verdict of the whole check, prints 0 or 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "pairing.hpp"

static std::vector<uint32_t> words(const std::string& hex) {
  if (hex == "-") return {};
  if (hex.size() % 8) { std::fprintf(stderr, "bad hex length\n"); std::exit(2); }
  std::vector<uint32_t> w(hex.size() / 8);
  for (size_t i = 0; i < w.size(); i++) {
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) v |= (uint32_t)std::stoul(hex.substr(8 * i + 2 * b, 2), nullptr, 16) << (8 * b);
    w[i] = v;
  }
  return w;
}

int main() {
  std::string kind;
  const zkhip::f2_single m;
  while (std::cin >> kind) {
    if (kind == "O") {
      int op;
      std::string ha, hb;
      std::cin >> op >> ha >> hb;
      const std::vector<uint32_t> a = words(ha), b = words(hb);
      if (a.size() != 96 || b.size() != 96 || op < 0 || op >= zkhip::PAIRING_TEST_OPS) { std::fprintf(stderr, "bad request\n"); return 2; }
      std::vector<uint32_t> out(96);
      zkhip::pairing_test_op(op, a.data(), b.data(), out.data(), m);
      for (uint32_t v : out) std::printf("%02x%02x%02x%02x", v & 255, (v >> 8) & 255, (v >> 16) & 255, v >> 24);
      std::printf("\n");
    } else if (kind == "V") {
      size_t n;
      std::string h1, h2;
      std::cin >> n >> h1 >> h2;
      const std::vector<uint32_t> g1 = words(h1), g2 = words(h2);
      if (g1.size() != 16 * n || g2.size() != 32 * n) { std::fprintf(stderr, "bad request\n"); return 2; }
      std::printf("%d\n", zkhip::pairing_check_serial(g1.data(), g2.data(), n, m) ? 1 : 0);
    } else {
      std::fprintf(stderr, "unknown request\n");
      return 2;
    }
  }
  return 0;
}

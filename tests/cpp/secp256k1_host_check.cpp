// csrc/secp256k1.hpp, sha256.hpp and secp256k1_h2c.hpp compiled for the host (tests/test_secp256k1_host.py builds this under ASan + UBSan): one
// command per line of standard input, values in hex, one line of results each; the test compares every value with Python integers and hashlib.
//   mul a b                          -> a b, a^2, 21 a, a mod p                         (any 256-bit a, b)
//   add a b                          -> a + b, a - b, -a                                (canonical a, b)
//   inv a                            -> a^(p - 2), a^((p + 1) / 4)
//   padd x1 y1 x2 y2                 -> P1 + P2 by the complete addition, 2 P1 by the complete doubling, both affine; on_curve(P1)
//   lin a x1 y1 b x2 y2              -> a P1 + b P2
//   sha HEX|-                        -> SHA-256 of the bytes
//   sswu u                           -> (x', y') on E', then its image under the isogeny
//   h2c MSGHEX|- x y                 -> H(msg, pk)
//   h2craw MSGHEX|-                  -> hash_to_curve(msg) of RFC 9380 itself: no key behind the message (the published vectors)
//   chal x y (pk, H, N, A, B)        -> the challenge digest
//   verify MSGHEX|- pkx pky nx ny s c -> verdict, H
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "secp256k1_h2c.hpp"

using namespace zkhip;

static sk_fe parse(const std::string& hex) {
  sk_fe r = sk_small(0);
  int nib = 0;
  for (size_t i = hex.size(); i-- > 0 && nib < 64; nib++) {
    const char ch = hex[i];
    const uint32_t v = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    r.l[nib / 8] |= v << (4 * (nib % 8));
  }
  return r;
}
static std::vector<uint8_t> bytes(const std::string& hex) {
  std::vector<uint8_t> out;
  if (hex == "-") return out;
  for (size_t i = 0; i + 1 < hex.size(); i += 2) out.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
  return out;
}
static void put(const sk_fe& a) {
  for (int i = 7; i >= 0; i--) std::printf("%08x", a.l[i]);
  std::printf(" ");
}
static void put(const sk_aff& a) { put(a.x); put(a.y); }
static void put_digest(const uint32_t d[8]) {
  for (int i = 0; i < 8; i++) std::printf("%08x", d[i]);
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
    auto fe = [&](size_t i) { return parse(w.at(i)); };
    auto pt = [&](size_t i) { sk_aff a; a.x = fe(i); a.y = fe(i + 1); return a; };
    if (op == "mul") {
      put(sk_mul(fe(0), fe(1))); put(sk_sqr(fe(0))); put(sk_mul_small(fe(0), 21)); put(sk_reduce(fe(0)));
    } else if (op == "add") {
      put(sk_add(fe(0), fe(1))); put(sk_sub(fe(0), fe(1))); put(sk_neg(fe(0)));
    } else if (op == "inv") {
      put(sk_inv(fe(0))); put(sk_sqrt(fe(0)));
    } else if (op == "padd") {
      put(sk_to_affine(sk_padd(sk_from_affine(pt(0)), sk_from_affine(pt(2))))); put(sk_to_affine(sk_pdbl(sk_from_affine(pt(0)))));
      std::printf("%d", sk_on_curve(pt(0)) ? 1 : 0);
    } else if (op == "lin") {
      put(sk_lincomb(fe(0), pt(1), fe(3), pt(4)));
    } else if (op == "sha") {
      const std::vector<uint8_t> data = bytes(w.at(0));
      uint32_t d[8];
      sha256_bytes(data.data(), data.size(), d);
      put_digest(d);
    } else if (op == "sswu") {
      const sk_aff e = h2c_sswu(fe(0));
      put(e); put(sk_to_affine(h2c_iso(e)));
    } else if (op == "h2c") {
      const std::vector<uint8_t> msg = bytes(w.at(0));
      h2c_prefix pre;
      h2c_prefix_build(msg.data(), msg.size(), &pre);
      put(h2c_hash(pre, pt(1)));
    } else if (op == "h2craw") {
      const std::vector<uint8_t> msg = bytes(w.at(0));
      h2c_prefix pre;
      h2c_prefix_build(msg.data(), msg.size(), &pre, false);
      put(h2c_hash(pre, sk_generator()));
    } else if (op == "chal") {
      uint32_t d[8];
      plume_challenge(pt(0), pt(2), pt(4), pt(6), pt(8), d);
      put_digest(d);
    } else if (op == "verify") {
      const std::vector<uint8_t> msg = bytes(w.at(0));
      h2c_prefix pre;
      h2c_prefix_build(msg.data(), msg.size(), &pre);
      sk_aff h;
      const uint32_t v = plume_verdict(pre, pt(1), pt(3), fe(5), fe(6), &h);
      std::printf("%u ", v);
      put(h);
    } else {
      std::printf("unknown command");
    }
    std::printf("\n");
    done++;
  }
  std::printf("secp256k1 host check done: %zu lines\n", done);
  return 0;
}

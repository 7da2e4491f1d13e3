// Host check of csrc/kzg_limbs.hpp and csrc/row_msm.hpp (tests/test_kzg_limbs_host.py builds this under ASan + UBSan and compares every line
// with Python integers).  Commands on stdin, one per line; 256-bit values are hexadecimal, the words the library reads or writes:
//   enc X Y              the affine point's Montgomery words            -> its six Fr values
//   dec L0 .. L5         six Fr values (Montgomery words)               -> status X Y
//   plan ROWS COLS       a row MSM's shape                              -> valid chunks stages units grid1 grid2 partial_bytes
//   pins                                                                 -> the header's pins: limbs of (1, 2) and of the coordinate q - 1, as integers
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "kzg_limbs.hpp"
#include "row_msm.hpp"

using namespace zkhip;

static void parse256(const std::string& hex, uint64_t out[4]) {
  std::string s = std::string(64 > hex.size() ? 64 - hex.size() : 0, '0') + hex;
  for (int i = 0; i < 4; i++) out[3 - i] = std::stoull(s.substr(16 * i, 16), nullptr, 16);
}
static void print256(const uint64_t v[4]) { std::printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64, v[3], v[2], v[1], v[0]); }

int main() {
  std::string line;
  size_t cases = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    if (cmd == "enc") {
      uint64_t pt[8], limbs[24];
      for (int c = 0; c < 2; c++) { in >> tok; parse256(tok, pt + 4 * c); }
      kzg_limbs::encode_point(pt, limbs);
      for (int i = 0; i < 6; i++) { print256(limbs + 4 * i); std::printf(i == 5 ? "\n" : " "); }
    } else if (cmd == "dec") {
      uint64_t pt[8], limbs[24];
      for (int i = 0; i < 6; i++) { in >> tok; parse256(tok, limbs + 4 * i); }
      std::memset(pt, 0xff, sizeof(pt));
      const uint32_t st = kzg_limbs::decode_point(limbs, pt);
      std::printf("%u ", st);
      print256(pt); std::printf(" "); print256(pt + 4); std::printf("\n");
    } else if (cmd == "plan") {
      uint64_t rows = 0, cols = 0;
      in >> rows >> cols;
      row_msm_plan p;
      const bool ok = row_msm_make_plan(rows, cols, &p);
      std::printf("%d %u %u %" PRIu64 " %u %u %zu\n", ok ? 1 : 0, p.chunks, p.stages, p.units, p.grid1, p.grid2, p.partial_bytes);
    } else if (cmd == "pins") {
      // (1, 2) and (q - 1, q - 1) through encode, the limbs brought back to integers
      const uint64_t one[4] = {1, 0, 0, 0}, two[4] = {2, 0, 0, 0};
      uint64_t qm1[4];
      for (int i = 0; i < 4; i++) qm1[i] = kzg_limbs::fq().p[i];
      qm1[0] -= 1;
      uint64_t pt[8], limbs[24], v[4];
      kzg_limbs::to_mont(kzg_limbs::fq(), one, pt); kzg_limbs::to_mont(kzg_limbs::fq(), two, pt + 4);
      kzg_limbs::encode_point(pt, limbs);
      for (int i = 0; i < 6; i++) { kzg_limbs::from_mont(kzg_limbs::fr(), limbs + 4 * i, v); print256(v); std::printf(" "); }
      kzg_limbs::to_mont(kzg_limbs::fq(), qm1, pt);
      kzg_limbs::encode_coordinate(pt, limbs);
      for (int i = 0; i < 3; i++) { kzg_limbs::from_mont(kzg_limbs::fr(), limbs + 4 * i, v); print256(v); std::printf(i == 2 ? "\n" : " "); }
    } else {
      std::printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
    cases++;
  }
  std::printf("kzg limbs host check done: %zu cases\n", cases);
  return 0;
}

// csrc/instance_evals.hpp on the host (tests/test_instance_host.py builds this with ASan + UBSan and supplies the vectors): one (query, proof)
// pair per case, computed the way a lane group of G lanes computes it on the device -- lane g's running fraction over the terms g, g + G, ...,
// then log2 G rounds in which lane g joins its fraction with lane g ^ d's -- and printed as a hexadecimal integer for the test to compare with
// Python's defining sum.  Every field element comes in as the device sees it: the 256-bit external Montgomery word (a 2^256 mod r), unpacked
// lazily (below 32 r), so the products run at the magnitudes of the kernel.
//
// stdin, one case per line:  G  k  rot  len  omega  omega^G  1/n  x  v_0 ... v_(len-1)     (decimal, decimal, decimal, decimal, then hexadecimal)
// stdout per case, one line: the evaluation as a plain integer, hexadecimal
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "instance_evals.hpp"

using namespace zkhip;
using Fr = FrParams;

struct words { uint32_t w[8]; };

static bool read_hex(words& out) {
  char s[80];
  if (scanf("%70s", s) != 1) return false;
  for (int i = 0; i < 8; i++) out.w[i] = 0;
  const size_t len = strlen(s);
  if (len == 0 || len > 64) return false;
  for (size_t k = 0; k < len; k++) {
    const char ch = s[len - 1 - k];
    uint32_t d;
    if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
    else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
    else return false;
    out.w[k / 8] |= d << (4 * (k % 8));
  }
  return true;
}

static std::string to_hex(const fe& internal) {
  uint32_t w[8];
  fe_pack(fe_canon_lt2p<Fr>(fe_mul<Fr>(internal, fe_const<Fr>(Fr::RAW_ONE))), w);
  char buf[16];
  std::string s;
  for (int i = 7; i >= 0; i--) {
    snprintf(buf, sizeof buf, "%08x", w[i]);
    s += buf;
  }
  return s;
}
static bool canonical(const fe& a) {        // N form and below r
  for (int i = 0; i < NL - 1; i++) if (a.l[i] > LMASK) return false;
  for (int i = NL - 1; i >= 0; i--) {
    if (a.l[i] < Fr::P[i]) return true;
    if (a.l[i] > Fr::P[i]) return false;
  }
  return false;
}
static bool same(const fe& a, const fe& b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }

int main() {
  unsigned G, k, rot, len;
  int cases = 0;
  while (scanf("%u %u %u %u", &G, &k, &rot, &len) == 4) {
    words omega, omega_g, n_inv, x;
    if ((G != 1 && G != 4 && G != 16) || k > 28 || rot >= (1u << k) || len > (1u << k) || !read_hex(omega) || !read_hex(omega_g) || !read_hex(n_inv) || !read_hex(x)) {
      fprintf(stderr, "bad input line %d\n", cases);
      return 2;
    }
    std::vector<words> values(len);                                // exactly len elements: ASan sees a read of v_len
    for (unsigned i = 0; i < len; i++)
      if (!read_hex(values[i])) { fprintf(stderr, "case %d: value %u\n", cases, i); return 2; }
    const fe xv = fe_from_ext_lazy(x.w);
    std::vector<ie_fraction> lane(G);
    for (unsigned g = 0; g < G; g++)
      lane[g] = ie_lane<Fr>(xv, k, fe_from_ext_lazy(omega.w), fe_from_ext_lazy(omega_g.w), rot, len, g, G, [&](uint32_t i) { return fe_from_ext_lazy(values.at(i).w); });
    for (unsigned d = 1; d < G; d <<= 1) {                         // what __shfl_xor at distance d does, every lane at once
      std::vector<ie_fraction> next(G);
      for (unsigned g = 0; g < G; g++) next[g] = ie_join<Fr>(lane[g], lane[g ^ d]);
      lane = next;
    }
    for (unsigned g = 1; g < G; g++)                               // the joins are symmetric: every lane of the group ends with the group's fraction
      if (!same(lane[g].num, lane[0].num) || !same(lane[g].den, lane[0].den)) { fprintf(stderr, "case %d: lane %u differs from lane 0\n", cases, g); return 3; }
    const fe e = ie_finish<Fr>(lane[0], xv, k, fe_from_ext_lazy(n_inv.w));
    if (!canonical(e)) { fprintf(stderr, "case %d: the output is not canonical\n", cases); return 3; }
    printf("%s\n", to_hex(e).c_str());
    cases++;
  }
  printf("instance host check done: %d cases\n", cases);
  return 0;
}

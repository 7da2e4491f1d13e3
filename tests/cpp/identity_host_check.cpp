// csrc/identity_points.hpp on the host (tests/test_identity_host.py builds this with ASan + UBSan and supplies the vectors): the domain values a
// verifier needs at its point x, printed as hexadecimal integers for the test to compare with Python's.
//
// stdin, one case per line:  k  u  omega  n_inv  x      (k, u decimal; the three field elements hexadecimal integers below r)
// stdout per case, one line:  x^n  l_0  l_last  l_active  in_domain      (plain integers, hexadecimal; in_domain 0 or 1)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "identity_points.hpp"

using namespace zkhip;
using Fr = FrParams;

static bool parse_hex(const char* s, uint32_t (&w)[8]) {
  for (int i = 0; i < 8; i++) w[i] = 0;
  const size_t len = strlen(s);
  if (len == 0 || len > 64) return false;
  for (size_t k = 0; k < len; k++) {
    const char ch = s[len - 1 - k];
    uint32_t d;
    if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
    else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
    else return false;
    w[k / 8] |= d << (4 * (k % 8));
  }
  return true;
}

// plain integer < r  ->  internal form (times 2^261), and back to canonical plain words
static fe to_internal(const uint32_t (&w)[8]) { return fe_mul<Fr>(fe_unpack<0>(w), fe_const<Fr>(Fr::R2)); }
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

int main() {
  unsigned k, u;
  char so[80], sn[80], sx[80];
  int cases = 0;
  while (scanf("%u %u %70s %70s %70s", &k, &u, so, sn, sx) == 5) {
    uint32_t wo[8], wn[8], wx[8];
    if (!parse_hex(so, wo) || !parse_hex(sn, wn) || !parse_hex(sx, wx) || k > 28 || u < 1 || u >= (1u << k) || (1u << k) - u > IDENTITY_MAX_TAIL) {
      fprintf(stderr, "bad input line %d\n", cases);
      return 2;
    }
    identity_points r;
    memset(&r, 0xA5, sizeof r);
    r = identity_points_at<Fr>(to_internal(wx), k, u, to_internal(wo), to_internal(wn));
    if (!canonical(r.xn) || !canonical(r.l0) || !canonical(r.l_last) || !canonical(r.l_active)) { fprintf(stderr, "case %d: an output is not canonical\n", cases); return 3; }
    printf("%s %s %s %s %d\n", to_hex(r.xn).c_str(), to_hex(r.l0).c_str(), to_hex(r.l_last).c_str(), to_hex(r.l_active).c_str(), r.in_domain ? 1 : 0);
    cases++;
  }
  printf("identity host check done: %d cases\n", cases);
  return 0;
}

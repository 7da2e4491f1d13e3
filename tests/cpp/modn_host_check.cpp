// csrc/modn.hpp on the host (tests/test_modn_host.py builds this with ASan + UBSan and supplies the vectors): the context builder and the four
// operations the Paillier kernels run, printed as hexadecimal integers for the test to compare with Python's.
//
// stdin, one case per line, four hexadecimal integers:  n  A  B  E      (n < 2^192; A, B < 2^384; E < 2^256)
// stdout per case, one line:  N  ninv  R mod N  R^2 mod N  A R  A R^-1  A B  A B R  A^E      (all mod N = n^2), or "refused" for an N the builder declines
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "modn.hpp"

using namespace zkhip;

static bool parse_hex(const char* s, uint32_t* out, int limbs) {
  for (int i = 0; i < limbs; i++) out[i] = 0;
  const size_t len = strlen(s);
  if (len == 0 || len > (size_t)limbs * 8) return false;
  for (size_t k = 0; k < len; k++) {
    const char ch = s[len - 1 - k];
    uint32_t d;
    if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
    else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
    else return false;
    out[k / 8] |= d << (4 * (k % 8));
  }
  return true;
}

static std::string hex(const uint32_t* l, int limbs) {
  char buf[16];
  std::string s;
  for (int i = limbs - 1; i >= 0; i--) {
    snprintf(buf, sizeof buf, "%08x", l[i]);
    s += buf;
  }
  return s;
}

int main() {
  char sn[128], sa[128], sb[128], se[128];
  int cases = 0;
  while (scanf("%100s %100s %100s %100s", sn, sa, sb, se) == 4) {
    uint32_t n32[6], e[8];
    modn A, B;
    if (!parse_hex(sn, n32, 6) || !parse_hex(sa, A.l, MODN_L) || !parse_hex(sb, B.l, MODN_L) || !parse_hex(se, e, 8)) {
      fprintf(stderr, "bad input line %d\n", cases);
      return 2;
    }
    uint64_t n64[3];
    for (int i = 0; i < 3; i++) n64[i] = (uint64_t)n32[2 * i] | ((uint64_t)n32[2 * i + 1] << 32);
    uint32_t N[MODN_L];
    modn_square_words(n64, 3, N);
    modn_ctx c;
    memset(&c, 0xA5, sizeof c);
    if (!modn_ctx_build(N, &c)) {
      printf("refused\n");
      cases++;
      continue;
    }
    // the 64-bit word forms round-trip
    uint64_t w[6];
    modn_to_words(A, w);
    const modn A2 = modn_from_words(w);
    if (memcmp(A.l, A2.l, sizeof A.l) != 0) { fprintf(stderr, "word round trip failed\n"); return 3; }
    const modn am = modn_to_mont(A, c), bm = modn_to_mont(B, c);
    const modn back = modn_from_mont(A, c);
    const modn ab = modn_mul(A, bm, c);           // A unreduced, bm < N
    const modn abr = modn_mul(am, bm, c);
    const modn p = modn_from_mont(modn_pow(am, e, 8, c), c);
    printf("%s %08x %s %s %s %s %s %s %s\n", hex(N, MODN_L).c_str(), c.ninv, hex(c.one, MODN_L).c_str(), hex(c.r2, MODN_L).c_str(), hex(am.l, MODN_L).c_str(),
           hex(back.l, MODN_L).c_str(), hex(ab.l, MODN_L).c_str(), hex(abr.l, MODN_L).c_str(), hex(p.l, MODN_L).c_str());
    cases++;
  }
  printf("modn host check done: %d cases\n", cases);
  return 0;
}

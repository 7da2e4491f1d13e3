// csrc/gwc_fold.hpp on the host (tests/test_gwc_fold_host.py builds this with ASan + UBSan and supplies the vectors): a proof's GWC rows and a
// column's fold, computed the way a workgroup of T lanes computes them on the device -- the v and u tables entry by entry, one lane per column,
// lane t's partial sum over the items t, t + T, ..., then the pairwise joins that the kernel makes through LDS -- and printed as hexadecimal
// integers for the test to compare with Python's sums.  Every field element comes in as the device sees it: the 256-bit external Montgomery
// word (a 2^256 mod r), unpacked lazily, so the products run at the magnitudes of the kernel.
//
// stdin, one case after another (decimal counts, hexadecimal elements):
//   gwc T n_sets n_slots n_evals  x v u  w_0 .. w_(n_sets-1)  then per query: set pos slot eval          (w_i = omega^rot_i)
//   fold T count negate  then per row: r a
//   join T count negate  then count canonical partial sums
//   scale negate r a
// stdout: gwc: n_sets + n_slots + 1 lines (the A row) and n_sets lines (the C row), plain integers; fold / join / scale: one line, the
// external word of the result (the value times 2^256 mod r), as the kernels store it
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gwc_fold.hpp"

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

static void print_words(const uint32_t (&w)[8]) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
  printf("\n");
}
static void print_internal(const fe& internal) {                 // a 2^261 -> a
  uint32_t w[8];
  fe_pack(fe_canon_lt2p<Fr>(fe_mul<Fr>(internal, fe_const<Fr>(Fr::RAW_ONE))), w);
  print_words(w);
}
static void print_packed(const fe& canonical) {
  uint32_t w[8];
  fe_pack(canonical, w);
  print_words(w);
}
static bool canonical(const fe& a) {                             // N form and below r
  for (int i = 0; i < NL - 1; i++) if (a.l[i] > LMASK) return false;
  for (int i = NL - 1; i >= 0; i--) {
    if (a.l[i] < Fr::P[i]) return true;
    if (a.l[i] > Fr::P[i]) return false;
  }
  return false;
}
static bool power_of_two(unsigned T) { return T && !(T & (T - 1)); }

// gf_join_block of the kernels: part[t] joins part[t + d] for d = T / 2, T / 4, ..., 1
static bool join_block(std::vector<fe>& part) {
  for (size_t d = part.size() >> 1; d; d >>= 1)
    for (size_t t = 0; t < d; t++) {
      if (!canonical(part.at(t)) || !canonical(part.at(t + d))) return false;
      part.at(t) = gf_join<Fr>(part.at(t), part.at(t + d));
    }
  return canonical(part.at(0));
}

static int gwc_case(int cases) {
  unsigned T, n_sets, n_slots, n_evals;
  words x, v, u;
  if (scanf("%u %u %u %u", &T, &n_sets, &n_slots, &n_evals) != 4 || !power_of_two(T) || T > GWC_THREADS || n_sets < 1 || n_sets > GWC_MAX_SETS || n_slots < 1 ||
      n_evals < 1 || n_evals > GWC_MAX_EVALS || !read_hex(x) || !read_hex(v) || !read_hex(u)) { fprintf(stderr, "case %d: bad gwc head\n", cases); return 2; }
  std::vector<words> set_omega(n_sets), evals(n_evals);
  std::vector<uint32_t> word(n_evals), slot(n_evals);
  for (auto& w : set_omega) if (!read_hex(w)) return 2;
  for (unsigned q = 0; q < n_evals; q++) {
    unsigned s, pos;
    if (scanf("%u %u %u", &s, &pos, &slot[q]) != 3 || s >= n_sets || pos >= n_evals || slot[q] >= n_slots || !read_hex(evals[q])) { fprintf(stderr, "case %d: query %u\n", cases, q); return 2; }
    word[q] = gf_query_word(s, pos);
  }
  // the plan's CSR list, as gwc_fold.hip builds it (exactly n_evals entries: ASan sees a read behind them)
  std::vector<uint32_t> slot_start(n_slots + 1, 0), slot_query(n_evals);
  for (unsigned q = 0; q < n_evals; q++) slot_start[slot[q] + 1]++;
  for (unsigned s = 0; s < n_slots; s++) slot_start[s + 1] += slot_start[s];
  std::vector<uint32_t> fill(slot_start.begin(), slot_start.end() - 1);
  for (unsigned q = 0; q < n_evals; q++) slot_query.at(fill[slot[q]]++) = q;
  std::vector<fe> vtab(GWC_V_BITS), upow(n_sets);                // exactly n_sets entries of the u table
  for (unsigned b = 0; b < GWC_V_BITS; b++) vtab[b] = gf_v_entry<Fr>(gf_reduce<Fr>(fe_from_ext_lazy(v.w)), b);
  for (unsigned i = 0; i < n_sets; i++) upow[i] = ip_pow<Fr>(gf_reduce<Fr>(fe_from_ext_lazy(u.w)), i);
  for (unsigned c = 0; c < n_sets; c++) print_internal(gf_witness_column<Fr>(upow[c], gf_reduce<Fr>(fe_from_ext_lazy(x.w)), fe_from_ext_lazy(set_omega[c].w)));
  for (unsigned s = 0; s < n_slots; s++)
    print_internal(gf_slot_column<Fr>(upow.data(), vtab.data(), slot_start[s], slot_start[s + 1], [&](uint32_t i) { return word.at(slot_query.at(i)); }));
  std::vector<fe> part(T);
  for (unsigned t = 0; t < T; t++)
    part[t] = gf_g_lane<Fr>(upow.data(), vtab.data(), n_evals, t, T, [&](uint32_t q) { return word.at(q); }, [&](uint32_t q) { return fe_from_ext_lazy(evals.at(q).w); });
  if (!join_block(part)) { fprintf(stderr, "case %d: a partial sum is not canonical\n", cases); return 3; }
  const fe g = gf_neg<Fr>(part[0]);
  if (!canonical(g)) { fprintf(stderr, "case %d: -G is not canonical\n", cases); return 3; }
  print_internal(g);
  for (unsigned i = 0; i < n_sets; i++) print_internal(upow[i]);
  return 0;
}

static int fold_case(int cases, bool second_level) {
  unsigned T, count, negate;
  if (scanf("%u %u %u", &T, &count, &negate) != 3 || !power_of_two(T) || T > FOLD_THREADS || count > FOLD_SPAN || negate > 1) { fprintf(stderr, "case %d: bad fold head\n", cases); return 2; }
  std::vector<words> r(second_level ? 0 : count), a(count);
  for (unsigned i = 0; i < count; i++)
    if ((!second_level && !read_hex(r[i])) || !read_hex(a[i])) { fprintf(stderr, "case %d: row %u\n", cases, i); return 2; }
  std::vector<fe> part(T);
  for (unsigned t = 0; t < T; t++)
    part[t] = second_level ? gf_join_lane<Fr>(count, t, T, [&](uint32_t i) { return fe_unpack<0>(a.at(i).w); })
                           : gf_fold_lane<Fr>(count, t, T, [&](uint32_t i) { return fe_from_ext_lazy(r.at(i).w); }, [&](uint32_t i) { return fe_unpack<0>(a.at(i).w); });
  if (!join_block(part)) { fprintf(stderr, "case %d: a partial sum is not canonical\n", cases); return 3; }
  const fe out = negate ? gf_neg<Fr>(part[0]) : part[0];
  if (!canonical(out)) { fprintf(stderr, "case %d: the output is not canonical\n", cases); return 3; }
  print_packed(out);
  return 0;
}

int main() {
  char mode[16];
  int cases = 0;
  while (scanf("%15s", mode) == 1) {
    int rc;
    if (!strcmp(mode, "gwc")) rc = gwc_case(cases);
    else if (!strcmp(mode, "fold")) rc = fold_case(cases, false);
    else if (!strcmp(mode, "join")) rc = fold_case(cases, true);
    else if (!strcmp(mode, "scale")) {
      unsigned negate;
      words r, a;
      if (scanf("%u", &negate) != 1 || negate > 1 || !read_hex(r) || !read_hex(a)) { fprintf(stderr, "case %d: bad scale\n", cases); return 2; }
      const fe out = gf_scale<Fr>(fe_from_ext_lazy(r.w), fe_unpack<0>(a.w), negate != 0);
      if (!canonical(out)) { fprintf(stderr, "case %d: the output is not canonical\n", cases); return 3; }
      print_packed(out);
      rc = 0;
    } else { fprintf(stderr, "case %d: mode %s\n", cases, mode); return 2; }
    if (rc) return rc;
    cases++;
  }
  printf("gwc fold host check done: %d cases\n", cases);
  return 0;
}

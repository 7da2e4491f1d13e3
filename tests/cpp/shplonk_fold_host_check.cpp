// csrc/shplonk_fold.hpp on the host (tests/test_shplonk_fold_host.py builds this with ASan + UBSan and supplies the vectors): a proof's SHPLONK
// rows computed the way a workgroup of T lanes computes them on the device -- the point differences and the y and v tables entry by entry, one
// task per set and per (set, point) pair, one lane's inversion, the weights, one lane per column, lane t's partial sum of G over the queries
// t, t + T, ..., then the pairwise joins that the kernel makes through LDS -- and printed as hexadecimal integers for the test to compare with
// multiopen.shplonk_accumulate.  Every field element comes in as the device sees it: the 256-bit external Montgomery word (a 2^256 mod r),
// unpacked lazily, so the products run at the magnitudes of the kernel.  The tables are vectors of exactly the plan's sizes: a read or a write
// behind one is ASan's to report.
//
// stdin, one case after another (decimal counts, hexadecimal elements):
//   shplonk T n_points n_sets n_slots n_evals  x y v u  w_0 .. w_(n_points-1)  set_start[0 .. n_sets]  set_point[0 .. pairs-1]
//           then per slot: set pos      then per query: slot point eval                                   (w_t = omega^rot_t)
// stdout per case: the status (0 or 1), then 2 + n_slots + 1 lines (the A row) and 1 line (the C row), plain integers
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "shplonk_fold.hpp"

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

static void print_internal(const fe& internal) {                 // a 2^261 -> a
  uint32_t w[8];
  fe_pack(fe_canon_lt2p<Fr>(fe_mul<Fr>(internal, fe_const<Fr>(Fr::RAW_ONE))), w);
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
  printf("\n");
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

static int shplonk_case(int cases) {
  unsigned T, n_points, n_sets, n_slots, n_evals;
  words x, y, v, u;
  if (scanf("%u %u %u %u %u", &T, &n_points, &n_sets, &n_slots, &n_evals) != 5 || !power_of_two(T) || T > SHPLONK_THREADS || n_points < 1 || n_points > SHPLONK_MAX_POINTS ||
      n_sets < 1 || n_sets > SHPLONK_MAX_SETS || n_slots < 1 || n_evals < 1 || n_evals > GWC_MAX_EVALS || !read_hex(x) || !read_hex(y) || !read_hex(v) || !read_hex(u)) {
    fprintf(stderr, "case %d: bad head\n", cases);
    return 2;
  }
  std::vector<words> point_omega(n_points), evals(n_evals);
  for (auto& w : point_omega) if (!read_hex(w)) return 2;
  std::vector<uint32_t> set_start(n_sets + 1);
  for (auto& s : set_start) if (scanf("%u", &s) != 1) return 2;
  if (set_start[0] != 0) return 2;
  for (unsigned i = 0; i < n_sets; i++) if (set_start[i + 1] <= set_start[i] || set_start[i + 1] > SHPLONK_MAX_PAIRS) { fprintf(stderr, "case %d: set %u\n", cases, i); return 2; }
  const unsigned n_pairs = set_start[n_sets];
  std::vector<uint32_t> set_point(n_pairs), pair_word(n_pairs), slot_word(n_slots), slot_set(n_slots), slot_pos(n_slots), query_word(n_evals);
  for (auto& pt : set_point) if (scanf("%u", &pt) != 1 || pt >= n_points) return 2;
  unsigned longest = 0;
  for (unsigned i = 0; i < n_sets; i++) {
    for (unsigned j = set_start[i]; j < set_start[i + 1]; j++) pair_word[j] = set_point[j] | (i << 16);
    if (set_start[i + 1] - set_start[i] > longest) longest = set_start[i + 1] - set_start[i];
  }
  for (unsigned s = 0; s < n_slots; s++) {
    if (scanf("%u %u", &slot_set[s], &slot_pos[s]) != 2 || slot_set[s] >= n_sets || slot_pos[s] >= (1u << GWC_V_BITS)) { fprintf(stderr, "case %d: slot %u\n", cases, s); return 2; }
    slot_word[s] = gf_query_word(slot_set[s], slot_pos[s]);
  }
  for (unsigned q = 0; q < n_evals; q++) {
    unsigned s, pt;
    if (scanf("%u %u", &s, &pt) != 2 || s >= n_slots || pt >= n_points || !read_hex(evals[q])) { fprintf(stderr, "case %d: query %u\n", cases, q); return 2; }
    unsigned j = set_start[slot_set[s]];
    while (j < set_start[slot_set[s] + 1] && set_point[j] != pt) j++;
    if (j == set_start[slot_set[s] + 1]) { fprintf(stderr, "case %d: query %u: its point is not in its slot's set\n", cases, q); return 2; }
    query_word[q] = gf_query_word(j, slot_pos[s]);
  }
  auto pair = [&](uint32_t j) { return pair_word.at(j); };
  // the host's share of the plan: c per pair, through the external form as the upload carries it
  std::vector<fe> omega_pow(n_points);
  for (unsigned t = 0; t < n_points; t++) omega_pow[t] = gf_reduce<Fr>(fe_from_ext_lazy(point_omega[t].w));
  std::vector<words> pair_coeff(n_pairs);
  for (unsigned i = 0; i < n_sets; i++)
    for (unsigned j = set_start[i]; j < set_start[i + 1]; j++)
      fe_to_ext<Fr>(sf_pair_coefficient<Fr>(set_point.data(), set_start[i], set_start[i + 1], j, [&](uint32_t pt) { return omega_pow.at(pt); }), pair_coeff[j].w);
  // 1. points
  const fe xr = gf_reduce<Fr>(fe_from_ext_lazy(x.w)), ur = gf_reduce<Fr>(fe_from_ext_lazy(u.w));
  std::vector<fe> diff(n_points), ytab(GWC_V_BITS), vpow(n_sets), zset(n_sets), wset(n_sets), lag(n_pairs), xpow(longest), part(T);
  for (unsigned t = 0; t < n_points; t++) diff[t] = sf_diff<Fr>(ur, xr, fe_from_ext_lazy(point_omega[t].w));
  for (unsigned i = 0; i < n_sets; i++) vpow[i] = ip_pow<Fr>(gf_reduce<Fr>(fe_from_ext_lazy(v.w)), i);
  for (unsigned b = 0; b < GWC_V_BITS; b++) ytab[b] = gf_v_entry<Fr>(gf_reduce<Fr>(fe_from_ext_lazy(y.w)), b);
  // 2. sets
  const fe zt = sf_outside<Fr>(diff.data(), n_points, 0);
  for (unsigned i = 0; i < n_sets; i++) zset[i] = sf_outside<Fr>(diff.data(), n_points, sf_set_mask(set_start[i], set_start[i + 1], pair));
  for (unsigned j = 0; j < n_pairs; j++) {
    const unsigned i = pair_word[j] >> 16;
    lag[j] = sf_numerator<Fr>(diff.data(), set_start[i], set_start[i + 1], j, pair);
  }
  // 3. the inversion
  const sf_inverse inv = sf_invert<Fr>(xr, zset[0]);
  sf_xinv_powers<Fr>(xpow.data(), longest, inv.xinv);
  printf("%d\n", inv.bad ? 1 : 0);
  const unsigned n_cols = 2 + n_slots + 1;
  if (inv.bad) {
    for (unsigned c = 0; c < n_cols + 1; c++) print_internal(fe_zero());
    return 0;
  }
  // 4. weights
  for (unsigned i = 0; i < n_sets; i++) wset[i] = sf_weight<Fr>(vpow[i], zset[i], inv.norm);
  for (unsigned j = 0; j < n_pairs; j++) {
    const unsigned i = pair_word[j] >> 16;
    lag[j] = sf_lagrange<Fr>(sf_weight<Fr>(vpow[i], zset[i], inv.norm), lag[j], xpow.at(set_start[i + 1] - set_start[i] - 1), fe_from_ext_lazy(pair_coeff[j].w));
  }
  // 5. columns
  print_internal(ur);
  const fe h = sf_h_column<Fr>(zt, inv.norm);
  if (!canonical(h)) { fprintf(stderr, "case %d: the H column is not canonical\n", cases); return 3; }
  print_internal(h);
  for (unsigned s = 0; s < n_slots; s++) {
    if ((slot_word[s] >> 16) >= n_sets) return 3;
    print_internal(gf_coeff<Fr>(wset.data(), ytab.data(), slot_word[s]));
  }
  for (unsigned q = 0; q < n_evals; q++) if ((query_word[q] >> 16) >= n_pairs) return 3;                 // the L table has n_pairs entries
  for (unsigned t = 0; t < T; t++)
    part[t] = gf_g_lane<Fr>(lag.data(), ytab.data(), n_evals, t, T, [&](uint32_t q) { return query_word.at(q); }, [&](uint32_t q) { return fe_from_ext_lazy(evals.at(q).w); });
  if (!join_block(part)) { fprintf(stderr, "case %d: a partial sum is not canonical\n", cases); return 3; }
  const fe g = gf_neg<Fr>(part[0]);
  if (!canonical(g)) { fprintf(stderr, "case %d: -G is not canonical\n", cases); return 3; }
  print_internal(g);
  print_internal(fe_one<Fr>());
  return 0;
}

int main() {
  char mode[16];
  int cases = 0;
  while (scanf("%15s", mode) == 1) {
    if (strcmp(mode, "shplonk")) { fprintf(stderr, "case %d: mode %s\n", cases, mode); return 2; }
    const int rc = shplonk_case(cases);
    if (rc) return rc;
    cases++;
  }
  printf("shplonk fold host check done: %d cases\n", cases);
  return 0;
}

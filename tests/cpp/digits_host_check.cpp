// Host check of csrc/msm_digits.hpp (compiled under ASan + UBSan by tests/test_digits_host.py): the conversion of a caller's Montgomery-256
// scalar word into the canonical integer by the Montgomery reduction alone (fr_ext_to_canon), and the signed recoding specialised on the
// (20, 13, 4) window layout (recode_fixed), against the big integers of bigint_ref.hpp and against the generic recoding (recode_window on
// the packed words, as the generic kernels run it).  For every scalar a < r:
//   conversion   fr_ext_to_canon(a 2^256 mod r) has limbs below 2^29 and the value a, and equals the product form it replaces
//   sum          sum_w d_w 2^(off_w) = a, and no carry leaves the top window
//   size         |d_w| <= 2^(cw - 1)
//   same digits  recode_fixed = recode_window, digit for digit (also for three other layouts of the template)
#include "bigint_ref.hpp"
#include "msm_digits.hpp"

static big R, R256, R256_INV;      // r, 2^256 mod r and its inverse
static long n_scalars = 0;

static big big_shl(uint64_t v, int bits) {      // v 2^bits for v < 2^32, bits <= 256
  big r = big_zero();
  r.w[bits >> 6] = v << (bits & 63);
  if ((bits & 63) > 32 && (bits >> 6) + 1 < 5) r.w[(bits >> 6) + 1] = v >> (64 - (bits & 63));
  return r;
}
static big pow2(int k) { return big_shl(1, k); }
static void words_of(const big& x, uint32_t (&w)[8]) { for (int j = 0; j < 8; j++) w[j] = (uint32_t)(x.w[j >> 1] >> (32 * (j & 1))); }

template <int C, int W, int NARROW>
static void check_layout(const fe& s, const big& a) {
  constexpr win_layout lay{C, W, NARROW};
  static_assert(win_off(lay, W - 1) + win_bits(lay, W - 1) >= 256, "the windows cover 256 bits");
  int32_t d[W], g[W];
  recode_fixed<C, W, NARROW>(s, d);
  uint32_t pw[8];
  fe_pack(s, pw);
  uint32_t carry = 0;
  for (int w = 0; w < W; w++) g[w] = recode_window(pw, lay, w, carry);
  CHECK(carry == 0, "a carry leaves the top window");
  big pos = big_zero(), neg = big_zero();
  for (int w = 0; w < W; w++) {
    const int cw = win_bits(lay, w), off = win_off(lay, w);
    CHECK(d[w] == g[w], "fixed and generic digits differ");
    CHECK(d[w] >= -(1 << (cw - 1)) && d[w] <= (1 << (cw - 1)), "|digit| above 2^(cw-1)");
    if (d[w] >= 0) pos = big_add(pos, big_shl((uint64_t)d[w], off)); else neg = big_add(neg, big_shl((uint64_t)(-(int64_t)d[w]), off));
  }
  CHECK(big_cmp(pos, big_add(a, neg)) == 0, "sum of d_w 2^off_w is not the scalar");
}

static fe convert_by_product(const uint32_t (&w)[8]) {      // the form fr_ext_to_canon replaces: mont261(x, 2^5)
  return fe_canon_lt2p<FrParams>(fe_mul<FrParams>(fe_const<FrParams>(FrParams::FROM_EXT_CANON), fe_unpack<0>(w)));
}

static void check_scalar(const big& a) {
  n_scalars++;
  CHECK(big_cmp(a, R) < 0, "test scalar not below r");
  uint32_t w[8];
  words_of(mulmod(a, R256, R), w);
  const fe s = fr_ext_to_canon(w), old = convert_by_product(w);
  bool canon = true, same = true;
  for (int i = 0; i < NL; i++) { canon = canon && s.l[i] <= LMASK; same = same && s.l[i] == old.l[i]; }
  CHECK(canon, "limb above 2^29");
  CHECK(same, "reduction alone and product form differ");
  CHECK(big_cmp(fe_value(s), a) == 0, "fr_ext_to_canon(a 2^256) is not a");
  check_layout<20, 13, 4>(s, a);       // the layout the wide tables ship with
  check_layout<19, 14, 10>(s, a);
  check_layout<18, 15, 14>(s, a);
  check_layout<16, 16, 0>(s, a);
}

// any 256-bit word is a valid input of the conversion (the bound at its call site): x -> x 2^-256 mod r
static void check_word(const big& x) {
  uint32_t w[8];
  words_of(x, w);
  const fe s = fr_ext_to_canon(w);
  CHECK(is_N(s) && s.l[NL - 1] <= LMASK, "limb above 2^29");
  CHECK(big_cmp(fe_value(s), mulmod(big_mod(x, R), R256_INV, R)) == 0, "fr_ext_to_canon(x) is not x 2^-256");
}

int main() {
  R = modulus<FrParams>();
  R256 = big_mod(pow2(256), R);
  R256_INV = invmod(R256, R);
  constexpr win_layout lay{20, 13, 4};
  const uint64_t top_max = R.w[3] >> (237 - 192);          // the top window (bits 237 .. 255) of r: a scalar's is at most this
  const big one = big_small(1);

  check_scalar(big_zero());
  check_scalar(one);
  check_scalar(big_sub(R, one));
  { big h = big_sub(R, one); for (int i = 0; i < 5; i++) h.w[i] = (h.w[i] >> 1) | (i < 4 ? h.w[i + 1] << 63 : 0); check_scalar(h); }   // (r - 1) / 2
  for (int w = 1; w < lay.W; w++) {                         // 2^k and 2^k - 1 at every window boundary (k = 0: the scalars 1 and 0 above)
    const int k = win_off(lay, w);
    check_scalar(pow2(k));
    check_scalar(big_sub(pow2(k), one));
    check_scalar(pow2(k - 1));                              // the half of the window below: the first value that carries
    check_scalar(big_add(pow2(k), one));
  }
  for (int k = 238; k <= 253; k++) { check_scalar(pow2(k)); check_scalar(big_sub(pow2(k), one)); }     // inside the top window, below r
  // every window 2^(cw-1) - 1 (the largest value that does not carry) and 2^(cw-1) (the smallest that does: the carry runs through all
  // windows); the top window holds what a scalar below r can: 0, 1, top_max - 1
  for (int delta = -1; delta <= 0; delta++)
    for (uint64_t top : {(uint64_t)0, (uint64_t)1, top_max - 1}) {
      big a = big_shl(top, win_off(lay, lay.W - 1));
      for (int w = 0; w < lay.W - 1; w++) a = big_add(a, big_shl((1u << (win_bits(lay, w) - 1)) + delta, win_off(lay, w)));
      check_scalar(a);
    }
  // the top window carries: all bits below it set (every window carries into the next, and the top digit is its bits plus one)
  for (uint64_t top : {(uint64_t)0, top_max - 1}) check_scalar(big_add(big_shl(top, win_off(lay, lay.W - 1)), big_sub(pow2(win_off(lay, lay.W - 1)), one)));
  // ... and with only the window below the top at its half
  check_scalar(big_add(big_shl(top_max - 1, win_off(lay, lay.W - 1)), pow2(win_off(lay, lay.W - 1) - 1)));
  for (int i = 0; i < 4000; i++) check_scalar(rnd_below(R));

  // words that are not reduced: r, r + 1, 2^256 - 1, 2^255, and random 256-bit words
  check_word(R);
  check_word(big_add(R, one));
  check_word(big_sub(pow2(256), one));
  check_word(pow2(255));
  for (int i = 0; i < 1000; i++) { big x = big_zero(); for (int j = 0; j < 4; j++) x.w[j] = rnd(); check_word(x); }

  if (fails) { printf("digits host check: %d FAILURES\n", fails); return 1; }
  printf("digits host check done: %ld scalars\n", n_scalars);
  return 0;
}

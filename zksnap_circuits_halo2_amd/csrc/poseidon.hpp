// Poseidon over BN254's Fr with T = 3, RATE = 2, R_F = 8, R_P = 57 (include/zkhip.h, "Poseidon"): the hash of the reference's membership Merkle
// trees (/root/reference/voter/src/merkletree/native.rs:30-49) and of the `PoseidonTranscript` its `gen_snark` proves under
// (/root/reference/aggregator/src/wrapper.rs:111-158).  Restated from the Poseidon paper: no Poseidon source was at hand.
//
//   poseidon_grain        the paper's Grain LFSR for (field 1, sbox 0, n 254, t 3, R_F 8, R_P 57): the 195 round constants and the 6 values
//                         the Cauchy matrix is made of come out of it; nothing is pasted.
//   poseidon_permute<F>   ONE body of the 65 rounds over a field policy F: the kernels (poseidon.hip) run it over the 9 x 29-bit Fr of
//                         fp29.hpp, the host calls over the 4 x 64 Montgomery Fr of include/zkhip.hpp.  The round loop stays rolled.
//   poseidon_hash<F>      a fresh sponge over w elements, one body as well.
//   poseidon_host_*       the host form: constants made once per process, no HIP call anywhere.
//
// The plain form (a dense 3 x 3 product every round) is the definition and is what runs: the form with sparse partial-round matrices is not
// built.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>
#include "../../include/zkhip.hpp"
#include "fp29.hpp"

namespace zkhip {

constexpr int POSEIDON_T = 3;
constexpr int POSEIDON_RATE = 2;
constexpr int POSEIDON_RF = 8;
constexpr int POSEIDON_RP = 57;
constexpr int POSEIDON_ROUNDS = POSEIDON_RF + POSEIDON_RP;
constexpr int POSEIDON_N_RC = POSEIDON_ROUNDS * POSEIDON_T;          // 195
constexpr int POSEIDON_N_MDS = POSEIDON_T * POSEIDON_T;              // 9
// the table both forms read: round constants (round-major), the matrix (row-major), then 2^64 (word 0 of a fresh sponge) and 1 (the padding)
constexpr int POSEIDON_TAB_MDS = POSEIDON_N_RC;
constexpr int POSEIDON_TAB_INIT = POSEIDON_TAB_MDS + POSEIDON_N_MDS;
constexpr int POSEIDON_TAB_ONE = POSEIDON_TAB_INIT + 1;
constexpr int POSEIDON_TAB_LEN = POSEIDON_TAB_ONE + 1;               // 206

// ---- the permutation and the sponge, over a field policy -----------------------------------------------------------------------------------
// F::E the element; F::add_c(a, c) = a + c with c a table entry or an input; F::pow5(x); F::dot3(m, a, b, c) = m[0] a + m[1] b + m[2] c.
// `tab` is read at indices that depend on the round counter alone: wave-uniform on the device, so the entries arrive by scalar loads.
// ONE rolled loop over the 65 rounds, the full rounds told from the partial ones by a branch on the round counter (wave-uniform as well):
// the first four, the 57 partial and the last four rounds share one body, a third of the code of three loops, and every word of the
// state is named so that nothing is indexed at run time (no scratch memory on the device).
template <class F>
ZK_HD void poseidon_permute(typename F::E (&s)[3], const typename F::E* __restrict__ tab) {
  typedef typename F::E E;
  const E* m = tab + POSEIDON_TAB_MDS;
#pragma unroll 1
  for (int r = 0; r < POSEIDON_ROUNDS; r++) {
    const E* rc = tab + r * POSEIDON_T;
    E x0 = F::pow5(F::add_c(s[0], rc[0]));
    E x1 = F::add_c(s[1], rc[1]);
    E x2 = F::add_c(s[2], rc[2]);
    if (r < POSEIDON_RF / 2 || r >= POSEIDON_RF / 2 + POSEIDON_RP) {
      x1 = F::pow5(x1);
      x2 = F::pow5(x2);
    }
    s[0] = F::dot3(m, x0, x1, x2);
    s[1] = F::dot3(m + 3, x0, x1, x2);
    s[2] = F::dot3(m + 6, x0, x1, x2);
  }
}

// a fresh sponge over w elements, `load(i)` the i-th: every full chunk of 2 into words 1 and 2, then the rest with a single 1 behind it;
// word 1 of the last state.  One permutation site, w / 2 + 1 turns of a rolled loop.
template <class F, class Load>
ZK_HD typename F::E poseidon_hash(uint32_t w, const typename F::E* __restrict__ tab, Load load) {
  typename F::E s[3] = {tab[POSEIDON_TAB_INIT], F::zero(), F::zero()};
  const uint32_t full = w / POSEIDON_RATE;
#pragma unroll 1
  for (uint32_t c = 0; c <= full; c++) {
    if (c < full) {
      s[1] = F::add_c(s[1], load(2 * c));
      s[2] = F::add_c(s[2], load(2 * c + 1));
    } else if (w & 1) {
      s[1] = F::add_c(s[1], load(w - 1));
      s[2] = F::add_c(s[2], tab[POSEIDON_TAB_ONE]);
    } else {
      s[1] = F::add_c(s[1], tab[POSEIDON_TAB_ONE]);
    }
    poseidon_permute<F>(s, tab);
  }
  return s[1];
}

// ---- host policy: canonical 4 x 64 Montgomery Fr ---------------------------------------------------------------------------------------------
struct poseidon_host_field {
  using E = halo2::Fr;
  static E zero() { return E{{0, 0, 0, 0}}; }
  static E add_c(const E& a, const E& c) { return halo2::detail::add_fr(a, c); }
  static E pow5(const E& x) {
    const E x2 = halo2::detail::mul(x, x);
    return halo2::detail::mul(halo2::detail::mul(x2, x2), x);
  }
  static E dot3(const E* m, const E& a, const E& b, const E& c) {
    namespace hd = halo2::detail;
    return hd::add_fr(hd::add_fr(hd::mul(m[0], a), hd::mul(m[1], b)), hd::mul(m[2], c));
  }
};

// ---- Grain ----------------------------------------------------------------------------------------------------------------------------------
struct poseidon_grain {
  uint8_t b[80];
  int head = 0;                                            // b[(head + i) % 80] is bit i of the state
  poseidon_grain() {
    int at = 0;
    auto put = [&](uint32_t v, int width) { for (int i = width - 1; i >= 0; i--) b[at++] = (uint8_t)((v >> i) & 1); };
    put(1, 2);                                             // a prime field
    put(0, 4);                                             // the S-box x^alpha
    put(254, 12);
    put(POSEIDON_T, 12);
    put(POSEIDON_RF, 10);
    put(POSEIDON_RP, 10);
    while (at < 80) b[at++] = 1;
    for (int i = 0; i < 160; i++) (void)step();
  }
  int bit_at(int i) const { return b[(head + i) % 80]; }
  int step() {
    const int nb = bit_at(62) ^ bit_at(51) ^ bit_at(38) ^ bit_at(23) ^ bit_at(13) ^ bit_at(0);
    b[head] = (uint8_t)nb;                                 // bit 0 leaves, the new bit becomes bit 79
    head = (head + 1) % 80;
    return nb;
  }
  int out_bit() {
    for (;;) {
      const int first = step(), second = step();
      if (first) return second;
    }
  }
  // 254 output bits as a big-endian integer, 4 little-endian words
  void draw(uint64_t v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0;
    for (int i = 0; i < 254; i++) {
      v[3] = (v[3] << 1) | (v[2] >> 63);
      v[2] = (v[2] << 1) | (v[1] >> 63);
      v[1] = (v[1] << 1) | (v[0] >> 63);
      v[0] = (v[0] << 1) | (uint64_t)out_bit();
    }
  }
};

// the table in canonical integers (not Montgomery): 195 constants with rejection, the matrix from 6 values reduced mod r, 2^64, 1
inline void poseidon_make_table(uint64_t (*canon)[4]) {
  namespace hd = halo2::detail;
  poseidon_grain g;
  for (int i = 0; i < POSEIDON_N_RC; i++) {
    do g.draw(canon[i]); while (hd::geq(canon[i], hd::R_MOD));
  }
  halo2::Fr xy[2 * POSEIDON_T];
  for (auto& e : xy) {
    uint64_t v[4];
    g.draw(v);
    if (hd::geq(v, hd::R_MOD)) hd::sub(v, v, hd::R_MOD);   // 2^254 < 2 r
    e = hd::from_raw(v);
  }
  const uint64_t raw_one[4] = {1, 0, 0, 0};
  for (int i = 0; i < POSEIDON_T; i++)
    for (int j = 0; j < POSEIDON_T; j++) {
      const halo2::Fr inv = hd::invert(hd::add_fr(xy[i], xy[POSEIDON_T + j]));
      hd::mont_mul(canon[POSEIDON_TAB_MDS + 3 * i + j], inv.l, raw_one, hd::R_MOD, hd::R_INV);
    }
  const uint64_t two64[4] = {0, 1, 0, 0};
  std::memcpy(canon[POSEIDON_TAB_INIT], two64, 32);
  std::memcpy(canon[POSEIDON_TAB_ONE], raw_one, 32);
}

struct poseidon_tables {
  uint64_t canon[POSEIDON_TAB_LEN][4];
  halo2::Fr host[POSEIDON_TAB_LEN];                        // Montgomery radix 2^256
  uint32_t dev[POSEIDON_TAB_LEN][NL];                      // 9 x 29-bit limbs of v 2^261 mod r: what the kernels read
};

inline const poseidon_tables& poseidon_tab() {
  static poseidon_tables T;
  static std::once_flag once;
  std::call_once(once, [] {
    namespace hd = halo2::detail;
    poseidon_make_table(T.canon);
    for (int i = 0; i < POSEIDON_TAB_LEN; i++) {
      T.host[i] = hd::from_raw(T.canon[i]);
      halo2::Fr m = T.host[i];                             // the integer v 2^256 mod r; five doublings make v 2^261 mod r
      for (int d = 0; d < 5; d++) m = hd::add_fr(m, m);
      for (int l = 0; l < NL; l++) {
        const int bit = LB * l, w = bit >> 6, sh = bit & 63;
        uint64_t v = m.l[w] >> sh;
        if (sh + LB > 64 && w < 3) v |= m.l[w + 1] << (64 - sh);
        T.dev[i][l] = (uint32_t)v & LMASK;
      }
    }
  });
  return T;
}

inline void poseidon_host_permute(halo2::Fr (&s)[3]) { poseidon_permute<poseidon_host_field>(s, poseidon_tab().host); }
inline halo2::Fr poseidon_host_hash(const halo2::Fr* in, size_t n) {
  return poseidon_hash<poseidon_host_field>((uint32_t)n, poseidon_tab().host, [&](uint32_t i) { return in[i]; });
}

// The sponge with its buffer (`pse_poseidon::Poseidon` as include/zkhip.h words it): the state carries on after a squeeze.
struct poseidon_sponge {
  halo2::Fr s[3];
  std::vector<halo2::Fr> buf;
  poseidon_sponge() { reset(); }
  void reset() {
    s[0] = poseidon_tab().host[POSEIDON_TAB_INIT];
    s[1] = s[2] = poseidon_host_field::zero();
    buf.clear();
  }
  void update(const halo2::Fr& v) { buf.push_back(v); }
  halo2::Fr squeeze() {
    namespace hd = halo2::detail;
    const halo2::Fr one = poseidon_tab().host[POSEIDON_TAB_ONE];
    size_t i = 0;
    for (; i + POSEIDON_RATE <= buf.size(); i += POSEIDON_RATE) {
      s[1] = hd::add_fr(s[1], buf[i]);
      s[2] = hd::add_fr(s[2], buf[i + 1]);
      poseidon_host_permute(s);
    }
    if (i < buf.size()) { s[1] = hd::add_fr(s[1], buf[i]); s[2] = hd::add_fr(s[2], one); }
    else s[1] = hd::add_fr(s[1], one);
    poseidon_host_permute(s);
    buf.clear();
    return s[1];
  }
};

#if defined(__HIPCC__)
// ---- device policy: fp29.hpp's Fr, Montgomery radix 2^261 ------------------------------------------------------------------------------------
// Magnitudes.  Table entries and inputs are N-form values < 1.2 r.  dot3 returns the limb-wise sum of two multiply outputs: value < 2.2 r,
// limbs < 2^30.  add_c adds an N-form value to that and carries: N form, value < 3.4 r (4.6 r where an input is absorbed), which fe_sqr takes
// (limbs < 2^30.3) and whose products stay far below 169 r^2, so every multiply output is < 2 r.
struct poseidon_dev_field {
  using E = fe;
  static ZK_D E zero() { return fe_zero(); }
  static ZK_D E add_c(const E& a, const E& c) { return fe_norm(fe_add(a, c)); }
  static ZK_D E pow5(const E& x) {
    const E x2 = fe_sqr<FrParams>(x);
    return fe_mul<FrParams>(fe_sqr<FrParams>(x2), x);
  }
  static ZK_D E dot3(const E* m, const E& a, const E& b, const E& c) {
    return fe_add(fe_mul_add<FrParams>(m[0], a, m[1], b), fe_mul<FrParams>(m[2], c));
  }
};
#endif

}  // namespace zkhip

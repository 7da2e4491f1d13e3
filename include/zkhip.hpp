// C++ host-side mirror of the reference's prover interface for the MSM / NTT path, header-only over the C ABI (zkhip.h).
//
// The reference is Rust and reaches this path through the un-vendored halo2-axiom crate [DEP]
// (`halo2_base::halo2_proofs`, /root/reference/aggregator/src/wrapper.rs:3-24).  This header gives a C++ host the same
// names, argument meaning and error behaviour:
//     halo2_proofs::arithmetic::{best_multiexp, best_fft, eval_polynomial, kate_division}
//     halo2_proofs::poly::EvaluationDomain::{new, lagrange_to_coeff, coeff_to_extended, extended_to_coeff,
//                                           divide_by_vanishing_poly, extended_len, get_omega, ...}
//     halo2_proofs::poly::kzg::commitment::ParamsKZG::{commit, commit_lagrange, get_g, k, n}
//     ff::BatchInvert, the grand products, plonk::lookup::prover::permute_expression_pair, and row programs (plonk::evaluation)
//     over device-resident columns (DeviceVec, RowProgram)
// Types are the Rust memory layouts (Montgomery limbs), so buffers can be shared with a Rust host unchanged.
// The reference's functions are infallible (`assert!` / `unwrap()`): here a failing call throws std::runtime_error with
// zkhip_last_error(), and length mismatches throw std::invalid_argument (the `assert_eq!` of best_multiexp / best_fft).
// Only scalar constants are computed on the host (what `EvaluationDomain::new` does); every vector operation runs in
// libzkhip.so on the GPU.  There is no CPU fallback.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <functional>
#include <istream>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "zkhip.h"

namespace zkhip {
namespace halo2 {

struct Fr {
  uint64_t l[4];  // Montgomery form, little-endian limbs (= halo2curves bn256::Fr)
  bool operator==(const Fr& o) const { return std::memcmp(l, o.l, 32) == 0; }
};
struct G1Affine {
  uint64_t x[4], y[4];  // identity = all zero
};
struct G1 {
  uint64_t x[4], y[4], z[4];  // Jacobian, identity z = 0
};
static_assert(sizeof(Fr) == 32 && sizeof(G1Affine) == 64 && sizeof(G1) == 96, "layouts must match the Rust types");

inline void check(int rc, const char* what) {
  if (rc != ZKHIP_OK) throw std::runtime_error(std::string(what) + ": " + zkhip_last_error());
}

// ---- scalar Fr arithmetic for domain constants (host; 4 x 64-bit Montgomery like the reference's Fr) ---------------
namespace detail {
typedef unsigned __int128 u128;
constexpr uint64_t R_MOD[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
constexpr uint64_t R_INV = 0xc2e1f593efffffffULL;  // -r^-1 mod 2^64
constexpr uint64_t R_ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
constexpr uint64_t R_R2[4] = {0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL, 0x0216d0b17f4e44a5ULL};

inline bool geq(const uint64_t a[4], const uint64_t b[4]) {
  for (int i = 3; i >= 0; i--) {
    if (a[i] != b[i]) return a[i] > b[i];
  }
  return true;
}
inline void sub(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
  uint64_t borrow = 0;
  for (int i = 0; i < 4; i++) {
    u128 d = (u128)a[i] - b[i] - borrow;
    r[i] = (uint64_t)d;
    borrow = (uint64_t)(d >> 64) & 1;
  }
}
// Montgomery product a b 2^-256 mod `mod` (CIOS, 4 x 64), for either BN254 field
inline void mont_mul(uint64_t r[4], const uint64_t a[4], const uint64_t b[4], const uint64_t mod[4], uint64_t inv) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    uint64_t carry = 0;
    for (int j = 0; j < 4; j++) {
      u128 s = (u128)a[j] * b[i] + t[j] + carry;
      t[j] = (uint64_t)s;
      carry = (uint64_t)(s >> 64);
    }
    u128 s = (u128)t[4] + carry;
    t[4] = (uint64_t)s;
    t[5] = (uint64_t)(s >> 64);
    const uint64_t m = t[0] * inv;
    s = (u128)m * mod[0] + t[0];
    carry = (uint64_t)(s >> 64);
    for (int j = 1; j < 4; j++) {
      s = (u128)m * mod[j] + t[j] + carry;
      t[j - 1] = (uint64_t)s;
      carry = (uint64_t)(s >> 64);
    }
    s = (u128)t[4] + carry;
    t[3] = (uint64_t)s;
    t[4] = t[5] + (uint64_t)(s >> 64);
  }
  if (t[4] || geq(t, mod)) sub(r, t, mod); else std::memcpy(r, t, 32);
}
inline Fr mul(const Fr& a, const Fr& b) {
  Fr r;
  mont_mul(r.l, a.l, b.l, R_MOD, R_INV);
  return r;
}
inline Fr one() { Fr r; std::memcpy(r.l, R_ONE, 32); return r; }
inline Fr from_u64(uint64_t v) { Fr raw{{v, 0, 0, 0}}, r2; std::memcpy(r2.l, R_R2, 32); return mul(raw, r2); }
inline Fr from_raw(const uint64_t v[4]) { Fr raw, r2; std::memcpy(raw.l, v, 32); std::memcpy(r2.l, R_R2, 32); return mul(raw, r2); }
inline Fr sub_fr(const Fr& a, const Fr& b) {
  Fr r;
  if (geq(a.l, b.l)) sub(r.l, a.l, b.l);
  else { uint64_t t[4]; sub(t, b.l, a.l); sub(r.l, R_MOD, t); }
  return r;
}
inline Fr add_fr(const Fr& a, const Fr& b) {
  Fr r;
  uint64_t carry = 0, t[4];
  for (int i = 0; i < 4; i++) {
    const u128 sum = (u128)a.l[i] + b.l[i] + carry;
    t[i] = (uint64_t)sum;
    carry = (uint64_t)(sum >> 64);
  }
  if (carry || geq(t, R_MOD)) sub(r.l, t, R_MOD); else std::memcpy(r.l, t, 32);
  return r;
}
inline Fr neg_fr(const Fr& a) { return sub_fr(Fr{}, a); }
inline Fr pow(Fr base, const uint64_t e[4]) {
  Fr acc = one();
  for (int i = 0; i < 256; i++) {
    if ((e[i >> 6] >> (i & 63)) & 1) acc = mul(acc, base);
    base = mul(base, base);
  }
  return acc;
}
inline Fr pow_u64(const Fr& base, uint64_t e) { const uint64_t ee[4] = {e, 0, 0, 0}; return pow(base, ee); }
inline Fr invert(const Fr& a) {
  uint64_t e[4];
  const uint64_t two[4] = {2, 0, 0, 0};
  sub(e, R_MOD, two);
  return pow(a, e);
}
}  // namespace detail

// `Fr::S`, `Fr::ROOT_OF_UNITY` (= 7^((r-1)/2^28)), `Fr::ZETA` of halo2curves bn256 [DEP]
constexpr uint32_t FR_S = 28;
inline Fr fr_root_of_unity() {
  const uint64_t raw[4] = {0xd34f1ed960c37c9cULL, 0x3215cf6dd39329c8ULL, 0x98865ea93dd31f74ULL, 0x03ddb9f5166d18b7ULL};
  return detail::from_raw(raw);
}
inline Fr fr_zeta() {
  const uint64_t raw[4] = {0xb8ca0b2d36636f23ULL, 0xcc37a73fec2bc5e9ULL, 0x048b6e193fd84104ULL, 0x30644e72e131a029ULL};
  return detail::from_raw(raw);
}

// ---- base field Fq and Fq2 on the host: only for the two G2 points of a `SerdeFormat::Processed` parameter file ----------------------
namespace detail {
constexpr uint64_t Q_MOD[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
constexpr uint64_t Q_INV = 0x87d20782e4866389ULL;  // -q^-1 mod 2^64
constexpr uint64_t Q_ONE[4] = {0xd35d438dc58f0d9dULL, 0x0a78eb28f5c70b3dULL, 0x666ea36f7879462cULL, 0x0e0a77c19a07df2fULL};
constexpr uint64_t Q_R2[4] = {0xf32cfc5b538afa89ULL, 0xb5e71911d44501fbULL, 0x47ab1eff0a417ff6ULL, 0x06d89f71cab8351fULL};
struct Fq {
  uint64_t l[4];   // Montgomery form
  bool operator==(const Fq& o) const { return std::memcmp(l, o.l, 32) == 0; }
  bool is_zero() const { return !(l[0] | l[1] | l[2] | l[3]); }
};
inline Fq fq_mul(const Fq& a, const Fq& b) { Fq r; mont_mul(r.l, a.l, b.l, Q_MOD, Q_INV); return r; }
inline Fq fq_add(const Fq& a, const Fq& b) {
  Fq r;
  uint64_t carry = 0, t[4];
  for (int i = 0; i < 4; i++) { const u128 sum = (u128)a.l[i] + b.l[i] + carry; t[i] = (uint64_t)sum; carry = (uint64_t)(sum >> 64); }
  if (carry || geq(t, Q_MOD)) sub(r.l, t, Q_MOD); else std::memcpy(r.l, t, 32);
  return r;
}
inline Fq fq_sub(const Fq& a, const Fq& b) {
  Fq r;
  if (geq(a.l, b.l)) sub(r.l, a.l, b.l);
  else { uint64_t t[4]; sub(t, b.l, a.l); sub(r.l, Q_MOD, t); }
  return r;
}
inline Fq fq_neg(const Fq& a) { return fq_sub(Fq{}, a); }
inline Fq fq_one() { Fq r; std::memcpy(r.l, Q_ONE, 32); return r; }
inline Fq fq_from_canonical(const uint64_t v[4]) { Fq raw, r2; std::memcpy(raw.l, v, 32); std::memcpy(r2.l, Q_R2, 32); return fq_mul(raw, r2); }
inline void fq_to_canonical(const Fq& a, uint64_t out[4]) { const Fq one_raw{{1, 0, 0, 0}}; const Fq c = fq_mul(a, one_raw); std::memcpy(out, c.l, 32); }
inline Fq fq_from_u64(uint64_t v) { const uint64_t raw[4] = {v, 0, 0, 0}; return fq_from_canonical(raw); }
inline Fq fq_pow(Fq base, const uint64_t e[4]) {
  Fq acc = fq_one();
  for (int i = 0; i < 256; i++) {
    if ((e[i >> 6] >> (i & 63)) & 1) acc = fq_mul(acc, base);
    base = fq_mul(base, base);
  }
  return acc;
}
inline Fq fq_invert(const Fq& a) { uint64_t e[4]; const uint64_t two[4] = {2, 0, 0, 0}; sub(e, Q_MOD, two); return fq_pow(a, e); }
// a root of a (q = 3 mod 4: a^((q+1)/4)); false when a is not a square
inline bool fq_sqrt(const Fq& a, Fq* root) {
  const uint64_t e[4] = {0x4f082305b61f3f52ULL, 0x65e05aa45a1c72a3ULL, 0x6e14116da0605617ULL, 0x0c19139cb84c680aULL};   // (q + 1) / 4
  *root = fq_pow(a, e);
  return fq_mul(*root, *root) == a;
}
struct Fq2 { Fq c0, c1; bool operator==(const Fq2& o) const { return c0 == o.c0 && c1 == o.c1; } };   // c0 + c1 u, u^2 = -1
inline Fq2 f2_mul(const Fq2& a, const Fq2& b) { return {fq_sub(fq_mul(a.c0, b.c0), fq_mul(a.c1, b.c1)), fq_add(fq_mul(a.c0, b.c1), fq_mul(a.c1, b.c0))}; }
inline Fq2 f2_add(const Fq2& a, const Fq2& b) { return {fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)}; }
inline Fq2 f2_invert(const Fq2& a) {
  const Fq d = fq_invert(fq_add(fq_mul(a.c0, a.c0), fq_mul(a.c1, a.c1)));
  return {fq_mul(a.c0, d), fq_neg(fq_mul(a.c1, d))};
}
// with s^2 = a0^2 + a1^2: x0^2 = (a0 +- s) / 2, x1 = a1 / (2 x0)
inline bool f2_sqrt(const Fq2& a, Fq2* root) {
  Fq r;
  if (a.c1.is_zero()) {
    if (fq_sqrt(a.c0, &r)) { *root = {r, Fq{}}; return true; }
    if (fq_sqrt(fq_neg(a.c0), &r)) { *root = {Fq{}, r}; return true; }     // a0 = -(r^2) = (r u)^2
    return false;
  }
  Fq s;
  if (!fq_sqrt(fq_add(fq_mul(a.c0, a.c0), fq_mul(a.c1, a.c1)), &s)) return false;
  const Fq half = fq_invert(fq_from_u64(2));
  const Fq cand[2] = {fq_mul(fq_add(a.c0, s), half), fq_mul(fq_sub(a.c0, s), half)};
  for (const Fq& t : cand) {
    Fq x0;
    if (!fq_sqrt(t, &x0) || x0.is_zero()) continue;
    const Fq2 x{x0, fq_mul(a.c1, fq_invert(fq_add(x0, x0)))};
    if (f2_mul(x, x) == a) { *root = x; return true; }
  }
  return false;
}
// `G2Affine::{to_bytes, from_bytes}`: 64 bytes, x.c0 || x.c1 canonical little-endian, flags in the last byte; the sign is the lsb of the
// first byte of y's encoding, i.e. of canonical y.c0.  `g2` = the memory of a G2Affine (16 Montgomery limbs); flag layouts as in zkhip.h
inline std::array<unsigned char, 64> g2_compress(const std::array<uint64_t, 16>& g2, int flag_layout) {
  std::array<unsigned char, 64> out{};
  bool zero = true;
  for (uint64_t w : g2) zero = zero && w == 0;
  if (zero) { if (flag_layout == 0) out[63] = 0x80; return out; }
  Fq c[3];
  for (int i = 0; i < 3; i++) std::memcpy(c[i].l, g2.data() + 4 * i, 32);
  uint64_t x0[4], x1[4], y0[4];
  fq_to_canonical(c[0], x0); fq_to_canonical(c[1], x1); fq_to_canonical(c[2], y0);
  std::memcpy(out.data(), x0, 32);
  std::memcpy(out.data() + 32, x1, 32);
  out[63] |= (unsigned char)((y0[0] & 1) << (flag_layout == 0 ? 6 : 7));
  return out;
}
inline std::array<uint64_t, 16> g2_decompress(const unsigned char in[64], int flag_layout) {
  unsigned char b[64];
  std::memcpy(b, in, 64);
  bool is_inf, sign;
  if (flag_layout == 0) { is_inf = (b[63] >> 7) != 0; sign = ((b[63] >> 6) & 1) != 0; b[63] &= 0x3f; }
  else { sign = (b[63] >> 7) != 0; b[63] &= 0x7f; is_inf = !sign; for (int i = 0; i < 64; i++) is_inf = is_inf && b[i] == 0; }
  std::array<uint64_t, 16> out{};
  bool any = false;
  for (int i = 0; i < 64; i++) any = any || b[i] != 0;
  if (is_inf) {
    if (any || sign) throw std::runtime_error("G2: identity flag on a non-zero encoding");
    return out;
  }
  uint64_t x0[4], x1[4];
  std::memcpy(x0, b, 32); std::memcpy(x1, b + 32, 32);
  if (geq(x0, Q_MOD) || geq(x1, Q_MOD)) throw std::runtime_error("G2: x is not canonical");
  const Fq2 x{fq_from_canonical(x0), fq_from_canonical(x1)};
  const Fq2 twist_b = f2_mul(Fq2{fq_from_u64(3), Fq{}}, f2_invert(Fq2{fq_from_u64(9), fq_one()}));     // 3 / (9 + u)
  Fq2 y;
  if (!f2_sqrt(f2_add(f2_mul(f2_mul(x, x), x), twist_b), &y)) throw std::runtime_error("G2: x is not the abscissa of a point of the twist");
  uint64_t y0[4];
  fq_to_canonical(y.c0, y0);
  if (((y0[0] & 1) != 0) != sign) y = {fq_neg(y.c0), fq_neg(y.c1)};
  std::memcpy(out.data(), x.c0.l, 32); std::memcpy(out.data() + 4, x.c1.l, 32);
  std::memcpy(out.data() + 8, y.c0.l, 32); std::memcpy(out.data() + 12, y.c1.l, 32);
  return out;
}
// `G2Affine::read_raw`'s validity check for the two G2 points of a RawBytes parameter file: canonical Montgomery residues and (0, 0) or
// y^2 = x^3 + 3 / (9 + u) on the twist (what srs.py's reader checks in the Python mirror)
inline bool g2_is_valid(const std::array<uint64_t, 16>& g2) {
  bool zero = true;
  for (uint64_t w : g2) zero = zero && w == 0;
  if (zero) return true;
  Fq c[4];
  for (int i = 0; i < 4; i++) {
    if (geq(g2.data() + 4 * i, Q_MOD)) return false;
    std::memcpy(c[i].l, g2.data() + 4 * i, 32);
  }
  const Fq2 x{c[0], c[1]}, y{c[2], c[3]};
  const Fq2 twist_b = f2_mul(Fq2{fq_from_u64(3), Fq{}}, f2_invert(Fq2{fq_from_u64(9), fq_one()}));
  return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), twist_b);
}
}  // namespace detail

// ---- halo2_proofs::arithmetic ----------------------------------------------------------------------------------
inline G1 best_multiexp(const Fr* coeffs, size_t coeffs_len, const G1Affine* bases, size_t bases_len) {
  if (coeffs_len != bases_len) throw std::invalid_argument("best_multiexp: coeffs.len() != bases.len()");
  G1 out;
  check(zkhip_msm_g1(coeffs->l, bases->x, coeffs_len, out.x), "best_multiexp");
  return out;
}
inline G1 best_multiexp(const std::vector<Fr>& coeffs, const std::vector<G1Affine>& bases) {
  static const Fr dummy_s{};
  static const G1Affine dummy_b{};
  return best_multiexp(coeffs.empty() ? &dummy_s : coeffs.data(), coeffs.size(), bases.empty() ? &dummy_b : bases.data(), bases.size());
}
// `best_multiexp::<G2Affine>`: the same function over the twist group (halo2curves bn256::{G2Affine, G2} memory: Fq2 = c0 || c1)
struct G2Affine {
  uint64_t x[8], y[8];   // identity = all zero
};
struct G2 {
  uint64_t x[8], y[8], z[8];   // Jacobian, identity z = 0
};
static_assert(sizeof(G2Affine) == 128 && sizeof(G2) == 192, "layouts must match the Rust types");
inline G2 best_multiexp(const std::vector<Fr>& coeffs, const std::vector<G2Affine>& bases) {
  if (coeffs.size() != bases.size()) throw std::invalid_argument("best_multiexp: coeffs.len() != bases.len()");
  static const Fr dummy_s{};
  static const G2Affine dummy_b{};
  G2 out;
  check(zkhip_msm_g2(coeffs.empty() ? dummy_s.l : coeffs.data()->l, bases.empty() ? dummy_b.x : bases.data()->x, coeffs.size(), out.x), "best_multiexp::<G2Affine>");
  return out;
}

// The devices this process drives (one `create_proof` process, several GPUs: /root/reference/aggregator/src/wrapper.rs:129).  devices[0]
// is the primary device; an SRS registered afterwards (ParamsKZG below) is cut into one point range per device and every commit is
// fanned out, gathered and folded by the library.  `set_msm_shards` cuts into more ranges than devices (round robin).
inline void init(const std::vector<int>& devices) { check(zkhip_init(devices.empty() ? nullptr : devices.data(), (int)devices.size()), "zkhip_init"); }
inline int device_count() { return zkhip_device_count(); }
inline void set_msm_shards(int shards) { check(zkhip_set_msm_shards(shards), "zkhip_set_msm_shards"); }
inline int msm_shards() { return zkhip_msm_shards(); }

inline void best_fft(std::vector<Fr>& a, const Fr& omega, uint32_t log_n) {
  if (a.size() != ((size_t)1 << log_n)) throw std::invalid_argument("best_fft: a.len() != 1 << log_n");
  check(zkhip_ntt_fr(a.data()->l, omega.l, log_n), "best_fft");
}
inline Fr eval_polynomial(const std::vector<Fr>& poly, const Fr& point) {
  Fr out;
  static const Fr dummy{};
  check(zkhip_fr_eval_polynomial(poly.empty() ? dummy.l : poly.data()->l, poly.size(), point.l, out.l), "eval_polynomial");
  return out;
}
inline std::vector<Fr> kate_division(const std::vector<Fr>& a, const Fr& b) {
  std::vector<Fr> q(a.empty() ? 0 : a.size() - 1);
  if (a.size() > 1) check(zkhip_fr_kate_division(a.data()->l, a.size(), b.l, q.data()->l), "kate_division");
  return q;
}
// `div_by_vanishing`: quotient of a(X) by prod_i (X - roots[i]) (1 .. ZKHIP_MAX_ROOTS distinct roots), remainder dropped; a.len() elements, the top
// roots.len() of them zero.  evals (optional) receives a(roots[i]).
inline std::vector<Fr> divide_by_roots(const std::vector<Fr>& a, const std::vector<Fr>& roots, std::vector<Fr>* evals = nullptr) {
  std::vector<Fr> q(a.size());
  if (evals) evals->assign(roots.size(), Fr{});
  static const Fr dummy{};
  check(zkhip_fr_divide_by_roots(a.empty() ? dummy.l : a.data()->l, a.size(), roots.empty() ? nullptr : roots.data()->l, (uint32_t)roots.size(),
                                 a.empty() ? nullptr : q.data()->l, evals && !roots.empty() ? evals->data()->l : nullptr), "divide_by_roots");
  return q;
}

// ---- the prover's other Fr-vector steps ---------------------------
// ff::BatchInvert: in place, zeros stay zero
inline void batch_invert(std::vector<Fr>& a) {
  if (!a.empty()) check(zkhip_fr_batch_invert(a.data()->l, a.size()), "batch_invert");
}
// the z column of the permutation / lookup arguments: z[0] = 1, z[i+1] = z[i] * num[i] / den[i]
inline std::vector<Fr> grand_product(const std::vector<Fr>& num, const std::vector<Fr>& den) {
  if (num.size() != den.size()) throw std::invalid_argument("grand_product: num.len() != den.len()");
  std::vector<Fr> z(num.size());
  if (!num.empty()) check(zkhip_fr_grand_product(num.data()->l, den.data()->l, num.size(), z.data()->l), "grand_product");
  return z;
}
// plonk::permutation::prover `Argument::commit`: the product column of every set of `chunk_len` permutation columns in one call, chained
// through z[usable_rows]; `values[c]` / `sigmas[c]` are the Lagrange values of permutation column c and of its sigma polynomial.  The
// rows after usable_rows repeat z[usable_rows]: the caller writes its blinding scalars there, as the reference does.
inline std::vector<std::vector<Fr>> permutation_products(const std::vector<std::vector<Fr>>& values, const std::vector<std::vector<Fr>>& sigmas, uint32_t chunk_len,
                                                         uint32_t log_n, size_t usable_rows, const Fr& beta, const Fr& gamma, const Fr& delta, const Fr& omega) {
  if (values.size() != sigmas.size() || chunk_len == 0) throw std::invalid_argument("permutation_products: values / sigmas / chunk_len");
  const size_t n = size_t(1) << log_n, sets = (values.size() + chunk_len - 1) / chunk_len;
  std::vector<const uint64_t*> vp(values.size()), sp(values.size());
  for (size_t c = 0; c < values.size(); c++) {
    if (values[c].size() != n || sigmas[c].size() != n) throw std::invalid_argument("permutation_products: a column is not 2^log_n rows long");
    vp[c] = values[c].data()->l;
    sp[c] = sigmas[c].data()->l;
  }
  std::vector<Fr> flat(sets * n);
  if (!values.empty())
    check(zkhip_permutation_products(vp.data(), sp.data(), (uint32_t)values.size(), chunk_len, log_n, usable_rows, beta.l, gamma.l, delta.l, omega.l, flat.data()->l),
          "permutation_products");
  std::vector<std::vector<Fr>> z(sets);
  for (size_t s = 0; s < sets; s++) z[s].assign(flat.begin() + s * n, flat.begin() + (s + 1) * n);
  return z;
}
// plonk::lookup::prover::permute_expression_pair on the usable rows; throws (like the reference's ConstraintSystemFailure) when an
// input value is missing from the table
inline std::pair<std::vector<Fr>, std::vector<Fr>> permute_expression_pair(const std::vector<Fr>& input, const std::vector<Fr>& table,
                                                                            size_t usable_rows) {
  if (input.size() < usable_rows || table.size() < usable_rows) throw std::invalid_argument("permute_expression_pair: usable_rows > len");
  std::vector<Fr> pi(usable_rows), pt(usable_rows);
  if (usable_rows) check(zkhip_lookup_permute(input.data()->l, table.data()->l, usable_rows, pi.data()->l, pt.data()->l), "permute_expression_pair");
  return {std::move(pi), std::move(pt)};
}
// elements first .. first + n - 1 of the library's random stream (zkhip.h, "random field elements"), brought to the host: what a verifier of
// the stream, or a host without device-resident columns, compares against
inline std::vector<Fr> random_fr(const std::array<uint8_t, 32>& seed, size_t n, uint64_t first = 0, uint64_t stream_id = 0) {
  std::vector<Fr> out(n);
  if (n) check(zkhip_fr_random(seed.data(), stream_id, first, n, out.data()->l), "random_fr");
  return out;
}

// A polynomial / column that lives in HBM between calls (zkhip_alloc / upload / download): what a host passes to the `_device`
// entry points so that iNTT -> commit -> extended NTT -> quotient never cross PCIe.
class DeviceVec {
 public:
  explicit DeviceVec(size_t len) : len_(len) { check(zkhip_alloc(len * sizeof(Fr), &p_), "DeviceVec"); }
  explicit DeviceVec(const std::vector<Fr>& host) : DeviceVec(host.size()) {
    if (len_) check(zkhip_upload(p_, host.data(), len_ * sizeof(Fr)), "DeviceVec upload");
  }
  DeviceVec(const DeviceVec&) = delete;
  DeviceVec& operator=(const DeviceVec&) = delete;
  DeviceVec(DeviceVec&& o) noexcept : p_(o.p_), len_(o.len_), owned_(o.owned_) { o.p_ = nullptr; o.len_ = 0; }
  ~DeviceVec() { if (owned_) (void)zkhip_free(p_); }
  // a view of `len` elements of device memory somebody else owns (a host that keeps its polynomials as handles of its own: the C entry
  // points zkhip_multiopen_* wrap their callers' addresses this way); never freed here
  static DeviceVec borrow(const void* p, size_t len) {
    DeviceVec v;
    v.p_ = const_cast<void*>(p); v.len_ = len; v.owned_ = false;
    return v;
  }
  void* data() const { return p_; }
  size_t size() const { return len_; }
  std::vector<Fr> to_host() const {
    std::vector<Fr> h(len_);
    if (len_) check(zkhip_download(h.data(), p_, len_ * sizeof(Fr)), "DeviceVec download");
    return h;
  }

 private:
  DeviceVec() = default;
  void* p_ = nullptr;
  size_t len_ = 0;
  bool owned_ = true;
};

// Poseidon over Fr, T = 3, RATE = 2, R_F = 8, R_P = 57 (zkhip.h, "Poseidon"): `pse_poseidon::Poseidon` as far as the reference uses it -- `update`,
// `squeeze_and_reset` (host, no GPU) -- and the trees of `MerkleTree::new` over leaves that lie in HBM.
struct Poseidon {
  std::vector<Fr> buf;
  void update(const std::vector<Fr>& values) { buf.insert(buf.end(), values.begin(), values.end()); }
  Fr squeeze_and_reset() {
    Fr out;
    check(zkhip_poseidon_hash(buf.empty() ? nullptr : buf[0].l, buf.size(), out.l), "Poseidon::squeeze_and_reset");
    buf.clear();
    return out;
  }
  static Fr hash(const std::vector<Fr>& values) { Poseidon p; p.update(values); return p.squeeze_and_reset(); }
  static void permute(Fr (&state)[3]) { check(zkhip_poseidon_permute(state[0].l, 1), "Poseidon::permute"); }
  // n messages of `width` elements at d_in -> n digests at d_out; one launch on `stream`
  static void hash_many_device(const void* d_in, size_t n, uint32_t width, void* d_out, void* stream = nullptr) {
    check(zkhip_poseidon_hash_many_device(d_in, n, width, d_out, stream), "Poseidon::hash_many_device");
  }
  // n secp256k1 points (8 canonical words each) packed and hashed in HBM: layout 0 the nullifier tree's values, 1 the members tree's leaves
  static void hash_points_device(const void* d_points, size_t n, uint32_t layout, void* d_out, void* stream = nullptr) {
    check(zkhip_poseidon_hash_points_device(d_points, n, layout, d_out, stream), "Poseidon::hash_points_device");
  }
  // the n_leaves - 1 inner nodes, level 1 first, the root last; no host wait
  static void merkle_device(const void* d_leaves, size_t n_leaves, void* d_nodes, void* stream = nullptr) {
    check(zkhip_poseidon_merkle_device(d_leaves, n_leaves, d_nodes, stream), "Poseidon::merkle_device");
  }
};

// `paillier_add_native` / `paillier_enc_native` over arrays in HBM (zkhip.h, "Paillier tally"): ciphertexts are ZKHIP_PAILLIER_WORDS canonical
// little-endian words, n is three words on the host and odd; every call is asynchronous on `stream`.
struct Paillier {
  uint64_t n[3];
  // d_out[i] = d_a[i] d_b[i] mod n^2; d_out may be d_a or d_b
  void mul_device(const void* d_a, const void* d_b, size_t count, void* d_out, void* stream = nullptr) const {
    check(zkhip_paillier_mul_device(n, d_a, d_b, count, d_out, stream), "Paillier::mul_device");
  }
  // d_running[n_ballots + 1][n_cols]: row i the prev_vote of round i, the last row the tally; d_init null: every column starts from 1
  void tally_device(const void* d_ballots, size_t n_ballots, uint32_t n_cols, const void* d_init, void* d_running, void* stream = nullptr) const {
    check(zkhip_paillier_tally_device(n, d_ballots, n_ballots, n_cols, d_init, d_running, stream), "Paillier::tally_device");
  }
  // d_out[i] = g^m[i] r[i]^n mod n^2; m: 4 words each, r: 3 words each
  void encrypt_device(const uint64_t g[6], const void* d_m, const void* d_r, size_t count, void* d_out, void* stream = nullptr) const {
    check(zkhip_paillier_encrypt_device(n, g, d_m, d_r, count, d_out, stream), "Paillier::encrypt_device");
  }
};

// The PLUME nullifier check, and signing, over arrays in HBM (zkhip.h, "PLUME nullifiers on secp256k1"): points are 8 and scalars 4 canonical little-endian
// words; `msg` is on the host and shared by the batch; every `_device` call is asynchronous on `stream`.
struct Plume {
  // d_out[i] = a[i] P[i] + b[i] Q[i]; d_status[i] = 2 and (0, 0) for a malformed point
  static void lincomb_device(const void* d_a, const void* d_p, const void* d_b, const void* d_q, size_t count, void* d_out, void* d_status, void* stream = nullptr) {
    check(zkhip_secp256k1_lincomb_device(d_a, d_p, d_b, d_q, count, d_out, d_status, stream), "Plume::lincomb_device");
  }
  // d_out[i] = H(msg, pk[i])
  static void hash_to_curve_device(const uint8_t* msg, size_t msg_len, const void* d_pk, size_t count, void* d_out, void* d_status, void* stream = nullptr) {
    check(zkhip_secp256k1_hash_to_curve_device(msg, msg_len, d_pk, count, d_out, d_status, stream), "Plume::hash_to_curve_device");
  }
  // d_status[i]: 0 accepted, 1 refused, 2 malformed; d_report: one zkhip_check_report; d_h_out null or count points
  static void verify_device(const uint8_t* msg, size_t msg_len, const void* d_pk, const void* d_nullifier, const void* d_s, const void* d_c, size_t count, void* d_status,
                            void* d_report, void* d_h_out = nullptr, void* stream = nullptr) {
    check(zkhip_plume_verify_device(msg, msg_len, d_pk, d_nullifier, d_s, d_c, count, d_status, d_report, d_h_out, stream), "Plume::verify_device");
  }
  // `gen_test_nullifier` of every voter from d_sk, d_r; d_status[i]: 0, or 2 and zeros for sk or r outside [1, n); d_h_out null or count points
  static void sign_device(const uint8_t* msg, size_t msg_len, const void* d_sk, const void* d_r, size_t count, void* d_pk, void* d_nullifier, void* d_s, void* d_c,
                          void* d_status, void* d_h_out = nullptr, void* stream = nullptr) {
    check(zkhip_plume_sign_device(msg, msg_len, d_sk, d_r, count, d_pk, d_nullifier, d_s, d_c, d_status, d_h_out, stream), "Plume::sign_device");
  }
  // one voter on the host
  static uint32_t sign(const uint8_t* msg, size_t msg_len, const uint64_t sk[4], const uint64_t r[4], uint64_t pk[8], uint64_t nullifier[8], uint64_t s[4],
                       uint64_t c[4], uint64_t h_out[8] = nullptr) {
    uint32_t status = 0;
    check(zkhip_plume_sign(msg, msg_len, sk, r, pk, nullifier, s, c, &status, h_out), "Plume::sign");
    return status;
  }
  static uint32_t hash_to_curve(const uint8_t* msg, size_t msg_len, const uint64_t pk[8], uint64_t out[8]) {
    uint32_t status = 0;
    check(zkhip_secp256k1_hash_to_curve(msg, msg_len, pk, out, &status), "Plume::hash_to_curve");
    return status;
  }
  static uint32_t verify(const uint8_t* msg, size_t msg_len, const uint64_t pk[8], const uint64_t nullifier[8], const uint64_t s[4], const uint64_t c[4],
                         uint64_t h_out[8] = nullptr) {
    uint32_t verdict = 0;
    check(zkhip_plume_verify(msg, msg_len, pk, nullifier, s, c, &verdict, h_out), "Plume::verify");
    return verdict;
  }
};

// `Blake2bWrite` / `Blake2bRead` with `Challenge255` [DEP transcript.rs] over zkhip_transcript_* (zkhip.h, "transcript"): the hash and the framing
// run on the host inside the library, the `_device` forms take commitments / evaluations where they lie in HBM.  One thread at a time per object.
class Transcript {
 public:
  static Transcript writer(int flag_layout = 0) { return Transcript(zkhip_transcript_new(flag_layout)); }                       // Blake2bWrite::init(vec![])
  static Transcript reader(const std::vector<uint8_t>& proof, int flag_layout = 0) {                                              // Blake2bRead::init(proof)
    return Transcript(zkhip_transcript_new_reader(proof.data(), proof.size(), flag_layout));
  }
  // the same object over the Poseidon sponge (zkhip.h, "Poseidon"): snark-verifier's `PoseidonTranscript` with the native loader
  static Transcript poseidon_writer(int flag_layout = 0) { return Transcript(zkhip_transcript_new_poseidon(flag_layout)); }
  static Transcript poseidon_reader(const std::vector<uint8_t>& proof, int flag_layout = 0) {
    return Transcript(zkhip_transcript_new_poseidon_reader(proof.data(), proof.size(), flag_layout));
  }
  Transcript(const Transcript&) = delete;
  Transcript& operator=(const Transcript&) = delete;
  Transcript(Transcript&& o) noexcept : t_(o.t_) { o.t_ = nullptr; }
  ~Transcript() { zkhip_transcript_free(t_); }
  void common_scalar(const Fr& s) { check(zkhip_transcript_common_scalars(t_, s.l, 1), "Transcript::common_scalar"); }
  void common_point(const G1Affine& p) { check(zkhip_transcript_common_points(t_, p.x, 1), "Transcript::common_point"); }
  Fr squeeze_challenge() {
    Fr c;
    check(zkhip_transcript_squeeze(t_, c.l), "Transcript::squeeze_challenge");
    return c;
  }
  void write_scalars(const std::vector<Fr>& s) { if (!s.empty()) check(zkhip_transcript_write_scalars(t_, s[0].l, s.size()), "Transcript::write_scalars"); }
  void write_scalars(const DeviceVec& s, void* stream = nullptr) { check(zkhip_transcript_write_scalars_device(t_, s.data(), s.size(), stream), "Transcript::write_scalars"); }
  void write_points(const std::vector<G1>& p) { if (!p.empty()) check(zkhip_transcript_write_points(t_, p[0].x, p.size()), "Transcript::write_points"); }
  // n Jacobian commitments (96 bytes each) in device memory, e.g. the output of zkhip_msm_g1_registered_batch_device
  void write_points_device(const void* d_points_xyz, size_t n, void* stream = nullptr) {
    check(zkhip_transcript_write_points_device(t_, d_points_xyz, n, stream), "Transcript::write_points_device");
  }
  std::vector<Fr> read_scalars(size_t n) {
    std::vector<Fr> out(n);
    if (n) check(zkhip_transcript_read_scalars(t_, n, out[0].l), "Transcript::read_scalars");
    return out;
  }
  std::vector<G1Affine> read_points(size_t n) {
    std::vector<G1Affine> out(n);
    if (n) check(zkhip_transcript_read_points(t_, n, out[0].x), "Transcript::read_points");
    return out;
  }
  // n affine points (64 bytes each) left at d_affine for the verifier's MSMs
  void read_points_device(size_t n, void* d_affine, void* stream = nullptr) {
    check(zkhip_transcript_read_points_device(t_, n, d_affine, stream), "Transcript::read_points_device");
  }
  std::vector<uint8_t> finalize() const {                                                                                         // the proof written (or given) so far
    size_t len = 0;
    check(zkhip_transcript_proof(t_, nullptr, 0, &len), "Transcript::finalize");
    std::vector<uint8_t> out(len);
    if (len) check(zkhip_transcript_proof(t_, out.data(), len, &len), "Transcript::finalize");
    return out;
  }

 private:
  explicit Transcript(zkhip_transcript* t) : t_(t) { if (!t_) throw std::runtime_error(std::string("Transcript: ") + zkhip_last_error()); }
  zkhip_transcript* t_;
};

// A row program (plonk::evaluation::GraphEvaluator lowered to include/zkhip.h's instruction set) over device-resident columns.
struct RowProgram {
  std::vector<zkhip_vm_insn> insns;
  std::vector<Fr> constants;
  std::vector<int32_t> rotations;
  int32_t rot_scale = 1;
  uint32_t result_reg = 0;
  bool uses_omega = false;
  Fr omega{};

  static zkhip_vm_operand constant(uint16_t i) { return zkhip_vm_operand{ZKHIP_SRC_CONST, 0, i}; }
  static zkhip_vm_operand reg(uint16_t i) { return zkhip_vm_operand{ZKHIP_SRC_REG, 0, i}; }
  static zkhip_vm_operand column(uint16_t col, uint8_t rot_slot) { return zkhip_vm_operand{ZKHIP_SRC_COLUMN, rot_slot, col}; }
  void emit(uint8_t op, uint8_t dst, zkhip_vm_operand a, zkhip_vm_operand b = {}, zkhip_vm_operand c = {}) {
    insns.push_back(zkhip_vm_insn{op, dst, 0, a, b, c});
  }
  // out[row] = program(row) for 2^log_rows rows; `accumulate`: ZKHIP_SRC_PREV reads out[row]
  void run(const std::vector<const DeviceVec*>& columns, uint32_t log_rows, DeviceVec& out, bool accumulate = false) const {
    std::vector<const void*> ptrs;
    for (const DeviceVec* c : columns) {
      if (c->size() < ((size_t)1 << log_rows)) throw std::invalid_argument("RowProgram: column shorter than 2^log_rows");
      ptrs.push_back(c->data());
    }
    if (out.size() < ((size_t)1 << log_rows)) throw std::invalid_argument("RowProgram: output shorter than 2^log_rows");
    zkhip_vm_program p{};
    p.insns = insns.data(); p.n_insns = (uint32_t)insns.size();
    p.constants = constants.empty() ? nullptr : constants.data()->l; p.n_constants = (uint32_t)constants.size();
    p.rotations = rotations.data(); p.n_rotations = (uint32_t)rotations.size();
    p.rot_scale = rot_scale; p.result_reg = result_reg;
    p.omega = uses_omega ? omega.l : nullptr;
    check(zkhip_fr_eval_rows_device(&p, ptrs.data(), (uint32_t)ptrs.size(), log_rows, accumulate ? 1 : 0, out.data(), nullptr), "RowProgram::run");
  }
};

// ---- halo2_proofs::poly::EvaluationDomain -----------------------------------------------------------------------
class EvaluationDomain {
 public:
  // `EvaluationDomain::new(j, k)`: j = degree of the constraint system, n = 2^k
  EvaluationDomain(uint32_t j, uint32_t k) : k_(k), n_((uint64_t)1 << k), quotient_poly_degree_(j - 1) {
    extended_k_ = k;
    while (((uint64_t)1 << extended_k_) < n_ * quotient_poly_degree_) extended_k_++;
    if (extended_k_ > FR_S) throw std::invalid_argument("EvaluationDomain: extended_k exceeds the field's 2-adicity");
    extended_omega_ = fr_root_of_unity();
    for (uint32_t i = extended_k_; i < FR_S; i++) extended_omega_ = detail::mul(extended_omega_, extended_omega_);
    omega_ = extended_omega_;
    for (uint32_t i = k; i < extended_k_; i++) omega_ = detail::mul(omega_, omega_);
    omega_inv_ = detail::invert(omega_);
    extended_omega_inv_ = detail::invert(extended_omega_);
    g_coset_ = fr_zeta();
    g_coset_inv_ = detail::mul(g_coset_, g_coset_);
    ifft_divisor_ = detail::invert(detail::from_u64(n_));
    extended_ifft_divisor_ = detail::invert(detail::from_u64((uint64_t)1 << extended_k_));
    // t(X) = X^n - 1 on the coset zeta * <extended_omega>, period 2^(extended_k - k); stored inverted
    const Fr orig = detail::pow_u64(g_coset_, n_), step = detail::pow_u64(extended_omega_, n_);
    Fr cur = orig;
    do {
      t_evaluations_.push_back(detail::invert(detail::sub_fr(cur, detail::one())));
      cur = detail::mul(cur, step);
    } while (!(cur == orig));
  }

  uint32_t k() const { return k_; }
  uint32_t extended_k() const { return extended_k_; }
  size_t extended_len() const { return (size_t)1 << extended_k_; }
  uint64_t get_quotient_poly_degree() const { return quotient_poly_degree_; }
  const Fr& get_omega() const { return omega_; }
  const Fr& get_omega_inv() const { return omega_inv_; }
  const Fr& get_extended_omega() const { return extended_omega_; }

  // Lagrange (evaluations over <omega>) -> coefficients: ifft(omega_inv) then * 1/n
  std::vector<Fr> lagrange_to_coeff(std::vector<Fr> a) const {
    if (a.size() != n_) throw std::invalid_argument("lagrange_to_coeff: wrong length");
    check(zkhip_ifft_scaled(a.data()->l, omega_inv_.l, k_, ifft_divisor_.l), "lagrange_to_coeff");
    return a;
  }
  std::vector<Fr> coeff_to_extended(const std::vector<Fr>& a) const {
    if (a.size() != n_) throw std::invalid_argument("coeff_to_extended: wrong length");
    std::vector<Fr> out(extended_len());
    check(zkhip_coeff_to_extended(a.data()->l, k_, out.data()->l, extended_k_, extended_omega_.l, g_coset_.l), "coeff_to_extended");
    return out;
  }
  std::vector<Fr> extended_to_coeff(std::vector<Fr> a) const {
    if (a.size() != extended_len()) throw std::invalid_argument("extended_to_coeff: wrong length");
    std::vector<Fr> out((size_t)(n_ * quotient_poly_degree_));
    check(zkhip_extended_to_coeff(a.data()->l, extended_k_, extended_omega_inv_.l, extended_ifft_divisor_.l, g_coset_.l,
                                  out.data()->l, out.size()), "extended_to_coeff");
    return out;
  }
  std::vector<Fr> divide_by_vanishing_poly(std::vector<Fr> a) const {
    if (a.size() != extended_len()) throw std::invalid_argument("divide_by_vanishing_poly: wrong length");
    check(zkhip_mul_periodic(a.data()->l, a.size(), t_evaluations_.data()->l, (uint32_t)t_evaluations_.size()), "divide_by_vanishing_poly");
    return a;
  }

 private:
  uint32_t k_, extended_k_;
  uint64_t n_, quotient_poly_degree_;
  Fr omega_, omega_inv_, extended_omega_, extended_omega_inv_, g_coset_, g_coset_inv_, ifft_divisor_, extended_ifft_divisor_;
  std::vector<Fr> t_evaluations_;
};

// ---- halo2_proofs::poly::kzg::commitment::ParamsKZG (commit surface) ----------------------------------------------
// `g_to_lagrange(g, k)` [DEP poly/kzg/commitment.rs]: the Lagrange-basis SRS of a monomial-basis SRS with unknown trapdoor -- an inverse
// FFT over the G1 points on the device (zkhip_g_to_lagrange_device)
inline std::vector<G1Affine> g_to_lagrange(const std::vector<G1Affine>& g, uint32_t k) {
  const uint64_t n = (uint64_t)1 << k;
  if (g.size() != n) throw std::invalid_argument("g_to_lagrange: length != 2^k");
  void *d_in = nullptr, *d_out = nullptr;
  check(zkhip_alloc(n * sizeof(G1Affine), &d_in), "g_to_lagrange alloc");
  int rc = zkhip_alloc(n * sizeof(G1Affine), &d_out);
  std::vector<G1Affine> out(n);
  if (rc == ZKHIP_OK) rc = zkhip_upload(d_in, g.data(), n * sizeof(G1Affine));
  if (rc == ZKHIP_OK) rc = zkhip_g_to_lagrange_device(d_in, k, d_out, nullptr);
  if (rc == ZKHIP_OK) rc = zkhip_download(out.data(), d_out, n * sizeof(G1Affine));
  (void)zkhip_free(d_in);
  if (d_out) (void)zkhip_free(d_out);
  check(rc, "g_to_lagrange");
  return out;
}

// `SerdeFormat` [DEP halo2-axiom helpers.rs]: Processed = compressed points and canonical scalars; RawBytes = the in-memory Montgomery
// limbs, checked on read; RawBytesUnchecked = the same without the checks (what the reference writes its proving keys with)
enum class SerdeFormat { Processed, RawBytes, RawBytesUnchecked };

class ParamsKZG {
 public:
  // takes ownership of the SRS arrays and pins them in HBM (prepared fixed-base tables)
  ParamsKZG(uint32_t k, std::vector<G1Affine> g, std::vector<G1Affine> g_lagrange = {})
      : k_(k), n_((uint64_t)1 << k), g_(std::move(g)), g_lagrange_(std::move(g_lagrange)) {
    if (g_.size() != n_ || (!g_lagrange_.empty() && g_lagrange_.size() != n_)) throw std::invalid_argument("ParamsKZG: SRS length != 2^k");
    check(zkhip_register_bases(g_.data()->x, g_.size()), "ParamsKZG::register g");
    if (!g_lagrange_.empty()) {
      // a constructor that throws runs no destructor: g_ must not stay registered over memory that is about to be freed
      const int rc = zkhip_register_bases(g_lagrange_.data()->x, g_lagrange_.size());
      if (rc != ZKHIP_OK) {
        const std::string why = zkhip_last_error();
        (void)zkhip_unregister_bases(g_.data()->x);
        throw std::runtime_error("ParamsKZG::register g_lagrange: " + why);
      }
    }
  }
  ~ParamsKZG() {
    if (!g_.empty()) zkhip_unregister_bases(g_.data()->x);
    if (!g_lagrange_.empty()) zkhip_unregister_bases(g_lagrange_.data()->x);
  }
  ParamsKZG(const ParamsKZG&) = delete;
  ParamsKZG& operator=(const ParamsKZG&) = delete;

  // `ParamsKZG::setup(k, rng)` with the trapdoor given (tests / benches, as the reference's benches do with a seeded rng):
  // g[i] = [s^i] G, g_lagrange[i] = [(s^n - 1)/n * w^i / (s - w^i)] G.  The scalar vectors are O(n) host multiplications plus one
  // batch inversion on the device; the 2n fixed-base multiplications run on the device.
  static ParamsKZG setup(uint32_t k, const Fr& s) {
    const uint64_t n = (uint64_t)1 << k;
    Fr omega = fr_root_of_unity();
    for (uint32_t i = k; i < 28; i++) omega = detail::mul(omega, omega);
    std::vector<Fr> pw(n), den(n);
    Fr cur = detail::one(), wi = detail::one();
    for (uint64_t i = 0; i < n; i++) {
      pw[i] = cur;
      den[i] = detail::sub_fr(s, wi);
      cur = detail::mul(cur, s);
      wi = detail::mul(wi, omega);
    }
    const Fr s_n = cur;                                             // s^n
    if (std::memcmp(s_n.l, detail::one().l, 32) == 0) throw std::invalid_argument("ParamsKZG::setup: trapdoor lies in the domain");
    batch_invert(den);
    const Fr mult = detail::mul(detail::sub_fr(s_n, detail::one()), detail::invert(detail::from_u64(n)));
    wi = detail::one();
    for (uint64_t i = 0; i < n; i++) {
      den[i] = detail::mul(detail::mul(den[i], wi), mult);          // L_i(s)
      wi = detail::mul(wi, omega);
    }
    auto points = [n](const std::vector<Fr>& scalars) {
      DeviceVec d_sc(scalars);
      void* d_pts = nullptr;
      check(zkhip_alloc(n * sizeof(G1Affine), &d_pts), "setup alloc");
      std::vector<G1Affine> out(n);
      int rc = zkhip_g1_fixed_base_mul_device(d_sc.data(), n, d_pts, nullptr);
      if (rc == ZKHIP_OK) rc = zkhip_download(out.data(), d_pts, n * sizeof(G1Affine));
      (void)zkhip_free(d_pts);
      check(rc, "ParamsKZG::setup");
      return out;
    };
    std::vector<G1Affine> g = points(pw), gl = points(den);
    return ParamsKZG(k, std::move(g), std::move(gl));
  }
  ParamsKZG(ParamsKZG&& o) noexcept : k_(o.k_), n_(o.n_), g_(std::move(o.g_)), g_lagrange_(std::move(o.g_lagrange_)), g2_(o.g2_), s_g2_(o.s_g2_) {}   // the registered arrays keep their addresses

  // G2Affine memory (x.c0 || x.c1 || y.c0 || y.c1, Montgomery limbs): carried for the verifying key and the SRS file only -- no G2
  // arithmetic exists on this path (/root/reference/aggregator/src/wrapper.rs:1143-1144 only reads g2() / s_g2())
  using G2Bytes = std::array<uint64_t, 16>;
  void set_g2(const G2Bytes& g2, const G2Bytes& s_g2) { g2_ = g2; s_g2_ = s_g2; }
  const G2Bytes& g2() const { return g2_; }
  const G2Bytes& s_g2() const { return s_g2_; }

  // `ParamsKZG::write` / `read` [DEP halo2-axiom poly/kzg/commitment.rs, SerdeFormat::RawBytes], the format of the
  // `kzg_bn254_{k}.srs` files `gen_srs` keeps (/root/reference/aggregator/benches/wrapper_circuit.rs:35):
  //   k u32 LE | g: 2^k x 64 B | g_lagrange: 2^k x 64 B | g2 128 B | s_g2 128 B      (raw = the in-memory Montgomery limbs)
  // Restated from the published layout; no reference file pins it.  Little-endian hosts only.
  void write(std::ostream& out) const {
    if (g_lagrange_.size() != n_) throw std::invalid_argument("ParamsKZG::write: no Lagrange basis");
    out.write(reinterpret_cast<const char*>(&k_), 4);
    out.write(reinterpret_cast<const char*>(g_.data()), (std::streamsize)(n_ * sizeof(G1Affine)));
    out.write(reinterpret_cast<const char*>(g_lagrange_.data()), (std::streamsize)(n_ * sizeof(G1Affine)));
    out.write(reinterpret_cast<const char*>(g2_.data()), 128);
    out.write(reinterpret_cast<const char*>(s_g2_.data()), 128);
    if (!out) throw std::runtime_error("ParamsKZG::write: stream error");
  }
  // `verify_points` (default): every point of both tables is verified on the GPU (zkhip_g1_check_points), as the reference's
  // SerdeFormat::RawBytes reader does; false = RawBytesUnchecked
  static ParamsKZG read(std::istream& in, bool verify_points = true) {
    uint32_t k = 0;
    in.read(reinterpret_cast<char*>(&k), 4);
    if (!in || k > 28) throw std::runtime_error("ParamsKZG::read: not a RawBytes KZG parameter file");
    const uint64_t n = (uint64_t)1 << k;
    std::vector<G1Affine> g(n), gl(n);
    G2Bytes g2{}, s_g2{};
    in.read(reinterpret_cast<char*>(g.data()), (std::streamsize)(n * sizeof(G1Affine)));
    in.read(reinterpret_cast<char*>(gl.data()), (std::streamsize)(n * sizeof(G1Affine)));
    in.read(reinterpret_cast<char*>(g2.data()), 128);
    in.read(reinterpret_cast<char*>(s_g2.data()), 128);
    if (!in) throw std::runtime_error("ParamsKZG::read: truncated file");
    if (verify_points) {
      uint64_t bad = 0;
      halo2::check(zkhip_g1_check_points(reinterpret_cast<const uint64_t*>(g.data()), (size_t)n, &bad), "zkhip_g1_check_points");
      if (bad < n) throw std::runtime_error("ParamsKZG::read: g holds a point that is not on the curve");
      halo2::check(zkhip_g1_check_points(reinterpret_cast<const uint64_t*>(gl.data()), (size_t)n, &bad), "zkhip_g1_check_points");
      if (bad < n) throw std::runtime_error("ParamsKZG::read: g_lagrange holds a point that is not on the curve");
      if (!detail::g2_is_valid(g2) || !detail::g2_is_valid(s_g2)) throw std::runtime_error("ParamsKZG::read: g2 / s_g2 is not a point of the twist");
    }
    ParamsKZG p(k, std::move(g), std::move(gl));
    p.set_g2(g2, s_g2);
    return p;
  }

  // `ParamsKZG::{write_custom, read_custom}`: Processed = k u32 LE | g: 2^k x 32 B | g_lagrange: 2^k x 32 B | g2 64 B | s_g2 64 B, every
  // point compressed (the two tables on the GPU: zkhip_g1_compress / zkhip_g1_decompress, the G2 points on the host)
  void write_custom(std::ostream& out, SerdeFormat f, int flag_layout = 0) const {
    if (f != SerdeFormat::Processed) { write(out); return; }
    if (g_lagrange_.size() != n_) throw std::invalid_argument("ParamsKZG::write: no Lagrange basis");
    out.write(reinterpret_cast<const char*>(&k_), 4);
    std::vector<unsigned char> buf(n_ * 32);
    for (const std::vector<G1Affine>* tab : {&g_, &g_lagrange_}) {
      halo2::check(zkhip_g1_compress(tab->data()->x, (size_t)n_, buf.data(), flag_layout), "zkhip_g1_compress");
      out.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)buf.size());
    }
    for (const G2Bytes* pt : {&g2_, &s_g2_}) {
      const std::array<unsigned char, 64> c = detail::g2_compress(*pt, flag_layout);
      out.write(reinterpret_cast<const char*>(c.data()), 64);
    }
    if (!out) throw std::runtime_error("ParamsKZG::write: stream error");
  }
  static ParamsKZG read_custom(std::istream& in, SerdeFormat f, int flag_layout = 0) {
    if (f != SerdeFormat::Processed) return read(in, f == SerdeFormat::RawBytes);
    uint32_t k = 0;
    in.read(reinterpret_cast<char*>(&k), 4);
    if (!in || k > 28) throw std::runtime_error("ParamsKZG::read: not a KZG parameter file");
    const uint64_t n = (uint64_t)1 << k;
    std::vector<G1Affine> tabs[2] = {std::vector<G1Affine>(n), std::vector<G1Affine>(n)};
    std::vector<unsigned char> buf(n * 32);
    for (auto& tab : tabs) {
      in.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)buf.size());
      if (!in) throw std::runtime_error("ParamsKZG::read: truncated file");
      uint64_t bad = 0;
      halo2::check(zkhip_g1_decompress(buf.data(), (size_t)n, tab.data()->x, flag_layout, &bad), "zkhip_g1_decompress");
      if (bad < n) throw std::runtime_error("ParamsKZG::read: a point does not decode to a curve point");
    }
    unsigned char tail[128];
    in.read(reinterpret_cast<char*>(tail), 128);
    if (!in) throw std::runtime_error("ParamsKZG::read: truncated file");
    ParamsKZG p(k, std::move(tabs[0]), std::move(tabs[1]));
    p.set_g2(detail::g2_decompress(tail, flag_layout), detail::g2_decompress(tail + 64, flag_layout));
    return p;
  }

  uint32_t k() const { return k_; }
  uint64_t n() const { return n_; }
  const std::vector<G1Affine>& get_g() const { return g_; }
  const std::vector<G1Affine>& get_g_lagrange() const { return g_lagrange_; }
  // `ParamsKZG::from_parts` with the Lagrange basis derived from g
  static ParamsKZG from_parts(uint32_t k, std::vector<G1Affine> g) {
    std::vector<G1Affine> gl = g_to_lagrange(g, k);
    return ParamsKZG(k, std::move(g), std::move(gl));
  }
  // `ParamsKZG::downsize(k)`: the first 2^k points of g, Lagrange basis re-derived on the device
  ParamsKZG downsize(uint32_t new_k) const {
    if (new_k > k_) throw std::invalid_argument("downsize: new_k > k");
    std::vector<G1Affine> g(g_.begin(), g_.begin() + ((size_t)1 << new_k));
    std::vector<G1Affine> gl = g_to_lagrange(g, new_k);
    ParamsKZG p(new_k, std::move(g), std::move(gl));
    p.set_g2(g2_, s_g2_);
    return p;
  }
  // commit(poly) = best_multiexp(poly.coeffs, g[..len]); blinding is ignored for KZG, as in the reference
  G1 commit(const std::vector<Fr>& poly) const {
    if (poly.size() > n_) throw std::invalid_argument("commit: polynomial longer than the SRS");
    return best_multiexp(poly.data(), poly.size(), g_.data(), poly.size());
  }
  // the same for a polynomial that lives in HBM (the first poly.size() points of the registered table): result downloaded
  G1 commit_device(const DeviceVec& poly, bool lagrange = false) const {
    const std::vector<G1Affine>& b = lagrange ? g_lagrange_ : g_;
    if (b.empty() || poly.size() > n_) throw std::invalid_argument("commit_device: no such basis / polynomial longer than the SRS");
    DeviceVec d_out(3);
    G1 out;
    check(zkhip_msm_g1_registered_device(b.data()->x, poly.data(), poly.size(), d_out.data(), nullptr), "commit_device");
    check(zkhip_download(&out, d_out.data(), sizeof(G1)), "commit_device download");
    return out;
  }
  // multi-column commit (not in the reference API: its provers commit column by column): K polynomials of equal length,
  // stored back to back, in one launch set
  std::vector<G1> commit_many(const std::vector<Fr>& polys, size_t len, bool lagrange = false) const {
    if (len == 0 || len > n_ || polys.size() % len != 0) throw std::invalid_argument("commit_many: bad shape");
    const std::vector<G1Affine>& b = lagrange ? g_lagrange_ : g_;
    if (b.empty()) throw std::invalid_argument("commit_many: no such basis");
    std::vector<G1> out(polys.size() / len);
    check(zkhip_msm_g1_batch(polys.data()->l, b.data()->x, len, out.size(), out.data()->x), "commit_many");
    return out;
  }
  G1 commit_lagrange(const std::vector<Fr>& poly) const {
    if (g_lagrange_.empty()) throw std::invalid_argument("commit_lagrange: no Lagrange basis");
    if (poly.size() > n_) throw std::invalid_argument("commit_lagrange: polynomial longer than the SRS");
    return best_multiexp(poly.data(), poly.size(), g_lagrange_.data(), poly.size());
  }

 private:
  uint32_t k_;
  uint64_t n_;
  std::vector<G1Affine> g_, g_lagrange_;
  G2Bytes g2_{}, s_g2_{};
};

// ---- plonk::keygen, plonk::permutation::keygen, key files -----------------------------------------
// `keygen_vk` / `keygen_pk` and `VerifyingKey` / `ProvingKey::{write, read}` [DEP halo2-axiom plonk/keygen.rs, plonk/permutation/keygen.rs,
// plonk.rs], as the reference uses them: /root/reference/aggregator/src/wrapper.rs:106-109 (keygen), :967-989 (`pk.write(..,
// SerdeFormat::RawBytesUnchecked)` into build/*_pk.bin), :1007-1034 (`ProvingKey::read`).  The file layout is restated from the
// published crate and NOT pinned by a file written by the Rust prover (none exists in the reference tree):
//   VerifyingKey: k u32 BE | #fixed u32 BE | fixed commitments (G1Affine raw) | permutation commitments (one per permutation column)
//                 | selectors, ceil(n / 8) bytes each, row j of a group of eight in bit j
//   Polynomial:   #values u32 BE | values (Fr raw);     slices of polynomials: count u32 BE, then the polynomials
//   ProvingKey:   VerifyingKey | l0 | l_last | l_active_row | fixed_values | fixed_polys | fixed_cosets | permutations | polys | cosets
// "raw" = the in-memory Montgomery limbs (RawBytes and RawBytesUnchecked; the former checks every element / point on read).  Processed:
// the same sequence with commitments compressed (32 B) and scalars as canonical integers (`to_repr`), both converted on the GPU.

// the part of `ConstraintSystem` keygen and the key readers need (the mirror has no circuit synthesis: the host supplies the assigned
// fixed columns and the copy constraints)
struct CircuitShape {
  uint32_t num_fixed = 0, num_permutation_columns = 0, num_selectors = 0;
  uint32_t degree = 4;             // cs.degree(): the extended domain is 2^k * (degree - 1) rounded up
  uint32_t blinding_factors = 5;   // cs.blinding_factors()
};

// `permutation::keygen::Assembly`: mapping[col][row] = next cell of the copy-constraint cycle through (col, row)
class Assembly {
 public:
  Assembly(size_t n, size_t columns) : n_(n), cols_(columns), mapping_(columns * n), aux_(columns * n), sizes_(columns * n, 1) {
    for (size_t c = 0; c < columns; c++)
      for (size_t r = 0; r < n; r++) mapping_[c * n + r] = aux_[c * n + r] = {(uint32_t)c, (uint32_t)r};
  }
  // merge the cycles of the two cells exactly as the reference does: the smaller cycle takes the larger one's representative, then the
  // two mapping entries are swapped
  void copy(size_t left_column, size_t left_row, size_t right_column, size_t right_row) {
    if (left_column >= cols_ || right_column >= cols_) throw std::invalid_argument("Assembly::copy: column not in the permutation");
    if (left_row >= n_ || right_row >= n_) throw std::invalid_argument("Assembly::copy: row out of bounds");
    cell l = aux_[left_column * n_ + left_row], r = aux_[right_column * n_ + right_row];
    if (l == r) return;
    if (sizes_[idx(l)] < sizes_[idx(r)]) std::swap(l, r);
    sizes_[idx(l)] += sizes_[idx(r)];
    cell i = r;
    do {
      aux_[idx(i)] = l;
      i = mapping_[idx(i)];
    } while (!(i == r));
    std::swap(mapping_[left_column * n_ + left_row], mapping_[right_column * n_ + right_row]);
  }
  size_t columns() const { return cols_; }
  size_t rows() const { return n_; }
  // `build_pk`'s permutations: sigma_c[row] = delta^(mapping column) * omega^(mapping row), Lagrange basis.  omega^row is one row
  // program on the device (the running power), the products another.
  std::vector<std::vector<Fr>> sigma_columns(uint32_t k) const;

 private:
  struct cell {
    uint32_t c, r;
    bool operator==(const cell& o) const { return c == o.c && r == o.r; }
  };
  size_t idx(const cell& x) const { return (size_t)x.c * n_ + x.r; }
  size_t n_, cols_;
  std::vector<cell> mapping_, aux_;
  std::vector<uint64_t> sizes_;
};

// `Fr::DELTA` = 7^(2^28): generator of the cosets the permutation argument labels its columns with
inline Fr fr_delta() {
  Fr d = detail::from_u64(7);
  for (uint32_t i = 0; i < FR_S; i++) d = detail::mul(d, d);
  return d;
}

inline std::vector<std::vector<Fr>> Assembly::sigma_columns(uint32_t k) const {
  if (((size_t)1 << k) != n_) throw std::invalid_argument("Assembly::sigma_columns: n != 2^k");
  Fr omega = fr_root_of_unity();
  for (uint32_t i = k; i < FR_S; i++) omega = detail::mul(omega, omega);
  RowProgram powers;
  powers.uses_omega = true;
  powers.omega = omega;
  powers.emit(ZKHIP_OP_MOV, 0, zkhip_vm_operand{ZKHIP_SRC_ROWPOW, 0, 0});
  DeviceVec d_pow(n_);
  powers.run({}, k, d_pow);
  const std::vector<Fr> omega_pow = d_pow.to_host();
  std::vector<Fr> delta_pow(cols_);
  Fr dp = detail::one();
  const Fr delta = fr_delta();
  for (size_t c = 0; c < cols_; c++) { delta_pow[c] = dp; dp = detail::mul(dp, delta); }
  RowProgram mul;
  mul.rotations = {0};
  mul.emit(ZKHIP_OP_MUL, 0, RowProgram::column(0, 0), RowProgram::column(1, 0));
  std::vector<std::vector<Fr>> out;
  std::vector<Fr> a(n_), b(n_);
  for (size_t c = 0; c < cols_; c++) {
    for (size_t r = 0; r < n_; r++) {
      const cell m = mapping_[c * n_ + r];
      a[r] = omega_pow[m.r];
      b[r] = delta_pow[m.c];
    }
    DeviceVec da(a), db(b), dout(n_);
    mul.run({&da, &db}, k, dout);
    out.push_back(dout.to_host());
  }
  return out;
}

namespace detail {
inline void put_u32_be(std::ostream& out, uint32_t v) {
  const unsigned char b[4] = {(unsigned char)(v >> 24), (unsigned char)(v >> 16), (unsigned char)(v >> 8), (unsigned char)v};
  out.write(reinterpret_cast<const char*>(b), 4);
}
inline uint32_t get_u32_be(std::istream& in) {
  unsigned char b[4];
  in.read(reinterpret_cast<char*>(b), 4);
  if (!in) throw std::runtime_error("key file truncated");
  return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
}
inline void check_format(SerdeFormat) {}
// Montgomery words <-> canonical integers (`to_repr` / `from_repr`) as one row program: a Montgomery product with the constant whose
// words are 1 strips the factor R, one with the constant whose words are R^2 puts it back
inline std::vector<Fr> convert_repr(const std::vector<Fr>& p, bool to_repr) {
  if (p.empty()) return p;
  uint32_t log = 0;
  while (((size_t)1 << log) < p.size()) log++;
  std::vector<Fr> padded(p);
  padded.resize((size_t)1 << log, Fr{});
  Fr c{{1, 0, 0, 0}};
  if (!to_repr) std::memcpy(c.l, R_R2, 32);
  RowProgram prog;
  prog.rotations = {0};
  prog.constants = {c};
  prog.emit(ZKHIP_OP_MUL, 0, RowProgram::column(0, 0), RowProgram::constant(0));
  DeviceVec in(padded), out(padded.size());
  prog.run({&in}, log, out);
  std::vector<Fr> r = out.to_host();
  r.resize(p.size());
  return r;
}
inline void put_poly(std::ostream& out, const std::vector<Fr>& p, SerdeFormat f = SerdeFormat::RawBytes) {
  put_u32_be(out, (uint32_t)p.size());
  if (f == SerdeFormat::Processed) {
    const std::vector<Fr> repr = convert_repr(p, true);
    out.write(reinterpret_cast<const char*>(repr.data()), (std::streamsize)(repr.size() * sizeof(Fr)));
  } else {
    out.write(reinterpret_cast<const char*>(p.data()), (std::streamsize)(p.size() * sizeof(Fr)));
  }
}
inline std::vector<Fr> get_poly(std::istream& in, SerdeFormat f, size_t want) {
  const uint32_t m = get_u32_be(in);
  if (m != want) throw std::runtime_error("key file: polynomial of unexpected length");
  std::vector<Fr> p(m);
  in.read(reinterpret_cast<char*>(p.data()), (std::streamsize)(m * sizeof(Fr)));
  if (!in) throw std::runtime_error("key file truncated");
  if (f != SerdeFormat::RawBytesUnchecked)
    for (const Fr& v : p) if (geq(v.l, R_MOD)) throw std::runtime_error("key file: non-canonical field element");
  return f == SerdeFormat::Processed ? convert_repr(p, false) : p;
}
inline void put_slice(std::ostream& out, const std::vector<std::vector<Fr>>& s, SerdeFormat f = SerdeFormat::RawBytes) {
  put_u32_be(out, (uint32_t)s.size());
  for (const auto& p : s) put_poly(out, p, f);
}
inline void put_points(std::ostream& out, const std::vector<G1Affine>& pts, SerdeFormat f) {
  if (f != SerdeFormat::Processed) { out.write(reinterpret_cast<const char*>(pts.data()), (std::streamsize)(pts.size() * sizeof(G1Affine))); return; }
  if (pts.empty()) return;
  std::vector<unsigned char> buf(pts.size() * 32);
  check(zkhip_g1_compress(pts.data()->x, pts.size(), buf.data(), 0), "zkhip_g1_compress");
  out.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)buf.size());
}
inline std::vector<std::vector<Fr>> get_slice(std::istream& in, SerdeFormat f, size_t want_count, size_t want_len) {
  if (get_u32_be(in) != want_count) throw std::runtime_error("key file: unexpected number of polynomials");
  std::vector<std::vector<Fr>> s;
  for (size_t i = 0; i < want_count; i++) s.push_back(get_poly(in, f, want_len));
  return s;
}
inline std::vector<G1Affine> get_points(std::istream& in, SerdeFormat f, size_t count) {
  std::vector<G1Affine> p(count);
  if (f == SerdeFormat::Processed) {
    if (!count) return p;
    std::vector<unsigned char> buf(count * 32);
    in.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)buf.size());
    if (!in) throw std::runtime_error("key file truncated");
    uint64_t bad = 0;
    check(zkhip_g1_decompress(buf.data(), count, p.data()->x, 0, &bad), "zkhip_g1_decompress");
    if (bad < count) throw std::runtime_error("key file: a commitment does not decode to a curve point");
    return p;
  }
  in.read(reinterpret_cast<char*>(p.data()), (std::streamsize)(count * sizeof(G1Affine)));
  if (!in) throw std::runtime_error("key file truncated");
  if (f == SerdeFormat::RawBytes && count) {
    uint64_t bad = 0;
    check(zkhip_g1_check_points(p.data()->x, count, &bad), "zkhip_g1_check_points");
    if (bad < count) throw std::runtime_error("key file: point is not on the curve");
  }
  return p;
}
}  // namespace detail

struct VerifyingKey {
  uint32_t k = 0;
  std::vector<G1Affine> fixed_commitments, permutation_commitments;
  std::vector<std::vector<bool>> selectors;

  void write(std::ostream& out, SerdeFormat f = SerdeFormat::RawBytes) const {
    detail::check_format(f);
    detail::put_u32_be(out, k);
    detail::put_u32_be(out, (uint32_t)fixed_commitments.size());
    detail::put_points(out, fixed_commitments, f);
    detail::put_points(out, permutation_commitments, f);
    for (const auto& sel : selectors)
      for (size_t i = 0; i < sel.size(); i += 8) {
        unsigned char byte = 0;
        for (size_t j = 0; j < 8 && i + j < sel.size(); j++) byte |= (unsigned char)(sel[i + j] ? 1u << j : 0u);
        out.put((char)byte);
      }
  }
  // `VerifyingKey::read::<_, ConcreteCircuit>`: the shape comes from the circuit, the commitments from the file
  static VerifyingKey read(std::istream& in, SerdeFormat f, const CircuitShape& cs) {
    detail::check_format(f);
    VerifyingKey vk;
    vk.k = detail::get_u32_be(in);
    if (vk.k > 28) throw std::runtime_error("key file: k out of range");
    if (detail::get_u32_be(in) != cs.num_fixed) throw std::runtime_error("key file: number of fixed commitments does not match the circuit");
    vk.fixed_commitments = detail::get_points(in, f, cs.num_fixed);
    vk.permutation_commitments = detail::get_points(in, f, cs.num_permutation_columns);
    const size_t n = (size_t)1 << vk.k;
    for (uint32_t s_i = 0; s_i < cs.num_selectors; s_i++) {
      std::vector<bool> sel(n);
      for (size_t i = 0; i < n; i += 8) {
        const int byte = in.get();
        if (byte < 0) throw std::runtime_error("key file truncated");
        for (size_t j = 0; j < 8 && i + j < n; j++) sel[i + j] = (byte >> j) & 1;
      }
      vk.selectors.push_back(std::move(sel));
    }
    return vk;
  }
};

struct ProvingKey {
  VerifyingKey vk;
  std::vector<Fr> l0, l_last, l_active_row;                                            // extended coset
  std::vector<std::vector<Fr>> fixed_values, fixed_polys, fixed_cosets;                // Lagrange, coefficient, extended coset
  std::vector<std::vector<Fr>> permutations, permutation_polys, permutation_cosets;    // the sigma columns, likewise

  void write(std::ostream& out, SerdeFormat f = SerdeFormat::RawBytesUnchecked) const {
    vk.write(out, f);
    detail::put_poly(out, l0, f); detail::put_poly(out, l_last, f); detail::put_poly(out, l_active_row, f);
    detail::put_slice(out, fixed_values, f); detail::put_slice(out, fixed_polys, f); detail::put_slice(out, fixed_cosets, f);
    detail::put_slice(out, permutations, f); detail::put_slice(out, permutation_polys, f); detail::put_slice(out, permutation_cosets, f);
    if (!out) throw std::runtime_error("ProvingKey::write: stream error");
  }
  static ProvingKey read(std::istream& in, SerdeFormat f, const CircuitShape& cs) {
    ProvingKey pk;
    pk.vk = VerifyingKey::read(in, f, cs);
    const EvaluationDomain dom(cs.degree, pk.vk.k);
    const size_t n = (size_t)1 << pk.vk.k, en = dom.extended_len();
    pk.l0 = detail::get_poly(in, f, en); pk.l_last = detail::get_poly(in, f, en); pk.l_active_row = detail::get_poly(in, f, en);
    pk.fixed_values = detail::get_slice(in, f, cs.num_fixed, n);
    pk.fixed_polys = detail::get_slice(in, f, cs.num_fixed, n);
    pk.fixed_cosets = detail::get_slice(in, f, cs.num_fixed, en);
    pk.permutations = detail::get_slice(in, f, cs.num_permutation_columns, n);
    pk.permutation_polys = detail::get_slice(in, f, cs.num_permutation_columns, n);
    pk.permutation_cosets = detail::get_slice(in, f, cs.num_permutation_columns, en);
    return pk;
  }
};

namespace detail {
inline std::vector<G1Affine> commit_lagrange_affine(const ParamsKZG& params, const std::vector<std::vector<Fr>>& columns) {
  std::vector<G1> jac;
  for (const auto& c : columns) jac.push_back(params.commit_lagrange(c));
  std::vector<G1Affine> out(jac.size());
  if (!jac.empty()) check(zkhip_g1_batch_normalize(jac.data()->x, jac.size(), out.data()->x), "batch_normalize");   // `Curve::batch_normalize`
  return out;
}
}  // namespace detail

// `keygen_vk(params, circuit)`: commitments to the fixed columns and the sigma columns (Lagrange-basis MSMs against g_lagrange)
inline VerifyingKey keygen_vk(const ParamsKZG& params, const CircuitShape& cs, const std::vector<std::vector<Fr>>& fixed, const Assembly& assembly,
                              std::vector<std::vector<bool>> selectors = {}) {
  if (fixed.size() != cs.num_fixed || assembly.columns() != cs.num_permutation_columns || assembly.rows() != params.n())
    throw std::invalid_argument("keygen_vk: fixed columns / permutation assembly do not match the circuit shape");
  if (params.n() < cs.blinding_factors + 3) throw std::invalid_argument("keygen_vk: not enough rows available");
  VerifyingKey vk;
  vk.k = params.k();
  vk.fixed_commitments = detail::commit_lagrange_affine(params, fixed);
  vk.permutation_commitments = detail::commit_lagrange_affine(params, assembly.sigma_columns(params.k()));
  vk.selectors = std::move(selectors);
  return vk;
}

// `keygen_pk(params, vk, circuit)`: polys by lagrange_to_coeff, cosets by coeff_to_extended; l_active_row = 1 - (l_last + l_blind) on the
// extended coset is the coset of the indicator of the usable rows (the same polynomial of degree < n)
inline ProvingKey keygen_pk(const ParamsKZG& params, const VerifyingKey& vk, const CircuitShape& cs, const std::vector<std::vector<Fr>>& fixed,
                            const Assembly& assembly) {
  if (vk.k != params.k()) throw std::invalid_argument("keygen_pk: verifying key and params differ in k");
  const EvaluationDomain dom(cs.degree, params.k());
  const size_t n = (size_t)params.n(), u = n - (cs.blinding_factors + 1);
  ProvingKey pk;
  pk.vk = vk;
  auto transform = [&](const std::vector<Fr>& lagrange, std::vector<Fr>* poly, std::vector<Fr>* coset) {
    std::vector<Fr> c = dom.lagrange_to_coeff(lagrange);
    if (coset) *coset = dom.coeff_to_extended(c);
    if (poly) *poly = std::move(c);
  };
  std::vector<Fr> ind(n, Fr{});
  ind[0] = detail::one();
  transform(ind, nullptr, &pk.l0);
  ind[0] = Fr{}; ind[u] = detail::one();
  transform(ind, nullptr, &pk.l_last);
  for (size_t i = 0; i < n; i++) ind[i] = i < u ? detail::one() : Fr{};
  transform(ind, nullptr, &pk.l_active_row);
  pk.fixed_values = fixed;
  pk.fixed_polys.resize(fixed.size()); pk.fixed_cosets.resize(fixed.size());
  for (size_t i = 0; i < fixed.size(); i++) transform(fixed[i], &pk.fixed_polys[i], &pk.fixed_cosets[i]);
  pk.permutations = assembly.sigma_columns(params.k());
  pk.permutation_polys.resize(pk.permutations.size()); pk.permutation_cosets.resize(pk.permutations.size());
  for (size_t i = 0; i < pk.permutations.size(); i++) transform(pk.permutations[i], &pk.permutation_polys[i], &pk.permutation_cosets[i]);
  return pk;
}

// ---- poly::kzg::multiopen: ProverGWC (the gen_snark path) and ProverSHPLONK (the benches' gen_proof path) -------------------------
// [DEP halo2-axiom poly/kzg/multiopen/{gwc.rs, gwc/prover.rs, shplonk.rs, shplonk/prover.rs]; reached from
// /root/reference/aggregator/src/wrapper.rs:59-60, 127-137 (GWC) and /root/reference/aggregator/benches/wrapper_circuit.rs:140 (SHPLONK).
// Polynomials stay on the device: combinations are fused row programs, quotients zkhip_fr_kate_division_device (one point) or
// zkhip_fr_divide_by_roots_device (a rotation set), commitments a prepared MSM.
// The transcript is the host's: challenges come in as arguments, commitments go out.  Restated from the published algorithms (unpinned).

// the SRS pinned for device-resident commits (`params.commit(&poly)` on a polynomial that lives in HBM)
class DeviceCommitter {
 public:
  explicit DeviceCommitter(const std::vector<G1Affine>& g) : n_(g.size()) {
    check(zkhip_alloc(n_ * sizeof(G1Affine), &d_g_), "DeviceCommitter alloc");
    int rc = zkhip_upload(d_g_, g.data(), n_ * sizeof(G1Affine));
    if (rc == ZKHIP_OK) rc = zkhip_prepare_bases_device(d_g_, n_, &handle_);
    if (rc == ZKHIP_OK) rc = zkhip_alloc(sizeof(G1), &d_out_);
    if (rc != ZKHIP_OK) { (void)zkhip_free(d_g_); check(rc, "DeviceCommitter"); }
  }
  ~DeviceCommitter() {
    if (handle_) (void)zkhip_release_bases(handle_);
    (void)zkhip_free(d_g_);
    (void)zkhip_free(d_out_);
  }
  DeviceCommitter(const DeviceCommitter&) = delete;
  DeviceCommitter& operator=(const DeviceCommitter&) = delete;
  G1 commit(const void* d_coeffs) const {          // n coefficients
    G1 out;
    check(zkhip_msm_g1_prepared_device(handle_, 0, d_coeffs, n_, d_out_, nullptr), "commit");
    check(zkhip_download(&out, d_out_, sizeof(G1)), "commit download");
    return out;
  }
  size_t n() const { return n_; }

 private:
  size_t n_;
  void *d_g_ = nullptr, *d_out_ = nullptr;
  uint64_t handle_ = 0;
};

struct ProverQuery {
  Fr point;
  const DeviceVec* poly;   // 2^k coefficients
  Fr eval{};
  bool has_eval = false;
};

namespace detail {
// out[row] = sum_k coeffs[k] * column_k[row] (zkhip_fr_linear_combination_device: groups of columns side by side, two products per
// reduction -- the same sum as a row program is `coeffs.size()` dependent multiply-adds per row, which is what the Python mirror runs)
inline void linear_combination(const std::vector<Fr>& coeffs, const std::vector<const DeviceVec*>& cols, uint32_t k, DeviceVec& out) {
  if (coeffs.size() != cols.size()) throw std::invalid_argument("linear_combination: coeffs.len() != columns.len()");
  const size_t n = (size_t)1 << k;
  std::vector<const void*> ptrs;
  for (const DeviceVec* c : cols) {
    if (c->size() < n) throw std::invalid_argument("linear_combination: column shorter than 2^k");
    ptrs.push_back(c->data());
  }
  if (out.size() < n) throw std::invalid_argument("linear_combination: output shorter than 2^k");
  check(zkhip_fr_linear_combination_device(ptrs.data(), coeffs.empty() ? nullptr : coeffs.data()->l, coeffs.size(), n, out.data(), nullptr), "linear_combination");
}
// plonk::lookup::prover::permute_expression_pair of EVERY lookup of a circuit in one call: inputs[l] / tables[l] = the compressed input / table
// expression of lookup l in HBM (the same DeviceVec given as several lookups' table is sorted once); permuted_inputs / permuted_tables hold
// [lookups][2^k] elements, rows < usable_rows of every column are written, the blinding rows behind them are the caller's.  Throws (like the
// reference's ConstraintSystemFailure) when an input value is missing from its table; the message names the lowest such lookup.
inline void permute_expression_pairs_device(const std::vector<const DeviceVec*>& inputs, const std::vector<const DeviceVec*>& tables, uint32_t k, size_t usable_rows,
                                            DeviceVec& permuted_inputs, DeviceVec& permuted_tables) {
  if (inputs.size() != tables.size()) throw std::invalid_argument("permute_expression_pairs_device: inputs.len() != tables.len()");
  const size_t n = (size_t)1 << k;
  std::vector<const void*> in, tab;
  for (size_t l = 0; l < inputs.size(); l++) {
    if (inputs[l]->size() < usable_rows || tables[l]->size() < usable_rows) throw std::invalid_argument("permute_expression_pairs_device: usable_rows > len");
    in.push_back(inputs[l]->data());
    tab.push_back(tables[l]->data());
  }
  if (permuted_inputs.size() < inputs.size() * n || permuted_tables.size() < inputs.size() * n) throw std::invalid_argument("permute_expression_pairs_device: output too short");
  if (in.size() == 1 && usable_rows >= (size_t(1) << 20)) {   // one lookup over 2^20 rows or more: the single call's two sorts beat a search per row (same bytes)
    check(zkhip_lookup_permute_device(in[0], tab[0], usable_rows, permuted_inputs.data(), permuted_tables.data(), nullptr), "permute_expression_pairs_device");
    return;
  }
  check(zkhip_lookup_permute_many_device(in.data(), tab.data(), (uint32_t)in.size(), k, usable_rows, permuted_inputs.data(), permuted_tables.data(), nullptr),
        "permute_expression_pairs_device");
}
// plonk::lookup::prover::commit_product of every lookup in one call: z = [lookups][2^k], z[l][0] = 1, the rows after usable_rows repeat
// z[l][usable_rows] (the caller writes its blinding scalars there)
inline void lookup_products_device(const std::vector<const DeviceVec*>& inputs, const std::vector<const DeviceVec*>& tables, const DeviceVec& permuted_inputs,
                                   const DeviceVec& permuted_tables, uint32_t k, size_t usable_rows, const Fr& beta, const Fr& gamma, DeviceVec& z) {
  if (inputs.size() != tables.size()) throw std::invalid_argument("lookup_products_device: inputs.len() != tables.len()");
  const size_t n = (size_t)1 << k;
  std::vector<const void*> in, tab;
  for (size_t l = 0; l < inputs.size(); l++) {
    if (inputs[l]->size() < usable_rows || tables[l]->size() < usable_rows) throw std::invalid_argument("lookup_products_device: usable_rows > len");
    in.push_back(inputs[l]->data());
    tab.push_back(tables[l]->data());
  }
  if (permuted_inputs.size() < in.size() * n || permuted_tables.size() < in.size() * n || z.size() < in.size() * n) throw std::invalid_argument("lookup_products_device: column block too short");
  check(zkhip_lookup_products_device(in.data(), tab.data(), permuted_inputs.data(), permuted_tables.data(), (uint32_t)in.size(), k, usable_rows, beta.l, gamma.l, z.data(), nullptr),
        "lookup_products_device");
}
// The witness checks (zkhip.h, "witness checks"): MockProver's three questions over columns that are already in HBM.  Each returns the
// records read back: failures = the number of failing items, first = the lowest failing index (UINT64_MAX: none).  They throw only when the
// check could not run.
inline std::vector<zkhip_check_report> read_check_reports(const std::function<int(void*)>& enqueue, size_t count, const char* what) {
  std::vector<zkhip_check_report> out(count);
  if (count == 0) return out;
  void* d = nullptr;
  check(zkhip_alloc(count * sizeof(zkhip_check_report), &d), what);
  int rc = enqueue(d);
  if (rc == ZKHIP_OK) rc = zkhip_stream_sync(nullptr);
  if (rc == ZKHIP_OK) rc = zkhip_download(out.data(), d, count * sizeof(zkhip_check_report));
  (void)zkhip_free(d);
  check(rc, what);
  return out;
}
inline zkhip_vm_program vm_program_of(const RowProgram& r) {
  zkhip_vm_program p{};
  p.insns = r.insns.data(); p.n_insns = (uint32_t)r.insns.size();
  p.constants = r.constants.empty() ? nullptr : r.constants.data()->l; p.n_constants = (uint32_t)r.constants.size();
  p.rotations = r.rotations.data(); p.n_rotations = (uint32_t)r.rotations.size();
  p.rot_scale = r.rot_scale; p.result_reg = r.result_reg;
  p.omega = r.uses_omega ? r.omega.l : nullptr;
  return p;
}
// gates: one program per gate polynomial over whole-domain columns; report p counts the rows of [row0, row0 + count) where program p is not zero
inline std::vector<zkhip_check_report> check_rows_device(const std::vector<RowProgram>& gates, const std::vector<const DeviceVec*>& columns, uint32_t k, uint64_t row0,
                                                         uint64_t count) {
  std::vector<zkhip_vm_program> progs;
  for (const RowProgram& g : gates) progs.push_back(vm_program_of(g));
  std::vector<const void*> ptrs;
  for (const DeviceVec* c : columns) {
    if (c->size() < ((size_t)1 << k)) throw std::invalid_argument("check_rows_device: column shorter than 2^k");
    ptrs.push_back(c->data());
  }
  return read_check_reports([&](void* d) {
    return zkhip_check_rows_device(progs.data(), (uint32_t)progs.size(), ptrs.data(), (uint32_t)ptrs.size(), k, row0, count, d, nullptr); }, progs.size(), "check_rows_device");
}
// copy constraints: d_map_col / d_map_row are [columns][2^k] u32 in HBM (permutation::keygen::Assembly's mapping); item index = column 2^k + row
inline zkhip_check_report check_copies_device(const std::vector<const DeviceVec*>& columns, uint32_t k, const void* d_map_col, const void* d_map_row) {
  std::vector<const void*> ptrs;
  for (const DeviceVec* c : columns) {
    if (c->size() < ((size_t)1 << k)) throw std::invalid_argument("check_copies_device: column shorter than 2^k");
    ptrs.push_back(c->data());
  }
  return read_check_reports([&](void* d) {
    return zkhip_check_copies_device(ptrs.data(), (uint32_t)ptrs.size(), k, d_map_col, d_map_row, d, nullptr); }, 1, "check_copies_device")[0];
}
// lookup membership over the usable rows, arguments as permute_expression_pairs_device (compressed columns; a shared table is sorted once)
inline std::vector<zkhip_check_report> check_lookups_device(const std::vector<const DeviceVec*>& inputs, const std::vector<const DeviceVec*>& tables, uint32_t k,
                                                            size_t usable_rows) {
  if (inputs.size() != tables.size()) throw std::invalid_argument("check_lookups_device: inputs.len() != tables.len()");
  std::vector<const void*> in, tab;
  for (size_t l = 0; l < inputs.size(); l++) {
    if (inputs[l]->size() < usable_rows || tables[l]->size() < usable_rows) throw std::invalid_argument("check_lookups_device: usable_rows > len");
    in.push_back(inputs[l]->data());
    tab.push_back(tables[l]->data());
  }
  return read_check_reports([&](void* d) {
    return zkhip_check_lookups_device(in.data(), tab.data(), (uint32_t)in.size(), k, usable_rows, d, nullptr); }, in.size(), "check_lookups_device");
}
// The quotient identity at x (zkhip.h, "the quotient identity at x"): the scalar half of `verify_proof` for a batch of proofs of one circuit.
// x^n, l_0, l_last, l_active at every point of `x`: out = [4][x.size()]; a point of the domain gets four zeros
inline void domain_points_device(uint32_t k, uint32_t usable_rows, const Fr& omega, const DeviceVec& x, DeviceVec& out) {
  if (out.size() < 4 * x.size()) throw std::invalid_argument("domain_points_device: out shorter than 4 x points");
  check(zkhip_fr_domain_points_device(k, usable_rows, omega.l, x.data(), x.size(), out.data(), nullptr), "domain_points_device");
}
struct IdentityVerdicts {
  std::vector<int32_t> status;       // per proof: 0 the identity holds, 1 it does not, 2 x lies in the domain
  zkhip_check_report report;         // proofs with a status other than 0, the lowest such index
};
// evals = [n_proofs][n_evals] as the proofs' transcripts yield them, challenges = [n_proofs][5] = theta, beta, gamma, y, x; `identity` reads
// column j < n_evals as evaluation j, n_evals + 0 .. 4 as the challenges, n_evals + 5 .. 8 as x^n, l_0, l_last, l_active
inline IdentityVerdicts verify_identity_device(const RowProgram& identity, const DeviceVec& evals, uint32_t n_evals, const DeviceVec& challenges, uint32_t k,
                                               uint32_t usable_rows, const Fr& omega, size_t n_proofs) {
  if (evals.size() < n_proofs * n_evals || challenges.size() < n_proofs * 5) throw std::invalid_argument("verify_identity_device: records shorter than the batch");
  IdentityVerdicts out;
  out.status.assign(n_proofs, 0);
  const zkhip_vm_program prog = vm_program_of(identity);
  void* d_status = nullptr;
  check(zkhip_alloc(n_proofs * sizeof(int32_t) + 16, &d_status), "verify_identity_device");
  struct release { void* p; ~release() { (void)zkhip_free(p); } } held{d_status};
  out.report = read_check_reports([&](void* d) {
    return zkhip_verify_identity_device(&prog, evals.data(), n_evals, challenges.data(), k, usable_rows, omega.l, n_proofs, d_status, d, nullptr); }, 1, "verify_identity_device")[0];
  if (n_proofs) check(zkhip_download(out.status.data(), d_status, n_proofs * sizeof(int32_t)), "verify_identity_device");
  return out;
}
// Instance columns (public inputs): `instances` = [n_proofs][sum of column_lens], `queries` = (instance column, rotation mod 2^k) pairs.
// out = [queries][n_proofs]: e[q][p] = sum_i v[p][c][i] l_((i - rot) mod n)(x[p]); a point of the domain gets zeros
inline void instance_evals_device(uint32_t k, const Fr& omega, const DeviceVec& x, const DeviceVec& instances, const std::vector<uint32_t>& column_lens,
                                  const std::vector<std::pair<uint32_t, uint32_t>>& queries, DeviceVec& out) {
  size_t total = 0;
  for (uint32_t len : column_lens) total += len;
  if (instances.size() < total * x.size() || out.size() < queries.size() * x.size()) throw std::invalid_argument("instance_evals_device: arrays shorter than the batch");
  std::vector<uint32_t> cols, rots;
  for (const auto& q : queries) { cols.push_back(q.first); rots.push_back(q.second); }
  check(zkhip_fr_instance_evals_device(k, omega.l, x.data(), instances.data(), column_lens.data(), (uint32_t)column_lens.size(), cols.data(), rots.data(),
                                       (uint32_t)queries.size(), x.size(), out.data(), nullptr), "instance_evals_device");
}
// verify_identity_device for a circuit with instance columns: query q is column n_evals + 9 + q of `identity`
inline IdentityVerdicts verify_identity_device(const RowProgram& identity, const DeviceVec& evals, uint32_t n_evals, const DeviceVec& challenges, uint32_t k,
                                               uint32_t usable_rows, const Fr& omega, const DeviceVec& instances, const std::vector<uint32_t>& column_lens,
                                               const std::vector<std::pair<uint32_t, uint32_t>>& queries, size_t n_proofs) {
  size_t total = 0;
  for (uint32_t len : column_lens) total += len;
  if (evals.size() < n_proofs * n_evals || challenges.size() < n_proofs * 5 || instances.size() < n_proofs * total)
    throw std::invalid_argument("verify_identity_device: records shorter than the batch");
  std::vector<uint32_t> cols, rots;
  for (const auto& q : queries) { cols.push_back(q.first); rots.push_back(q.second); }
  IdentityVerdicts out;
  out.status.assign(n_proofs, 0);
  const zkhip_vm_program prog = vm_program_of(identity);
  void* d_status = nullptr;
  check(zkhip_alloc(n_proofs * sizeof(int32_t) + 16, &d_status), "verify_identity_device");
  struct release { void* p; ~release() { (void)zkhip_free(p); } } held{d_status};
  out.report = read_check_reports([&](void* d) {
    return zkhip_verify_identity_instances_device(&prog, evals.data(), n_evals, challenges.data(), k, usable_rows, omega.l, instances.data(), column_lens.data(),
                                                  (uint32_t)column_lens.size(), cols.data(), rots.data(), (uint32_t)queries.size(), n_proofs, d_status, d, nullptr); },
    1, "verify_identity_device")[0];
  if (n_proofs) check(zkhip_download(out.status.data(), d_status, n_proofs * sizeof(int32_t)), "verify_identity_device");
  return out;
}
// The batch verifier's scalar side (zkhip.h, "the batch verifier").  A key's opening plan as the GWC verifier groups it: query q is evaluation q of
// a record; its set (sets in order of first appearance, one rotation each), its position inside the set, the slot of its polynomial
struct GwcPlan {
  std::vector<uint32_t> set_rotation, query_set, query_pos, query_slot;
  uint32_t n_slots = 0;
};
// rows_a = [n_proofs][n_sets + n_slots + 1], rows_c = [n_proofs][n_sets]: the scalars of every proof's two accumulated points (layout: zkhip.h)
inline void gwc_scalars_device(const GwcPlan& plan, const DeviceVec& evals, const DeviceVec& points, uint32_t k, const Fr& omega, size_t n_proofs, DeviceVec& rows_a,
                               DeviceVec& rows_c) {
  const size_t n_evals = plan.query_set.size(), n_sets = plan.set_rotation.size();
  if (plan.query_pos.size() != n_evals || plan.query_slot.size() != n_evals) throw std::invalid_argument("gwc_scalars_device: the plan's query arrays differ in length");
  if (evals.size() < n_proofs * n_evals || points.size() < n_proofs * 3 || rows_a.size() < n_proofs * (n_sets + plan.n_slots + 1) || rows_c.size() < n_proofs * n_sets)
    throw std::invalid_argument("gwc_scalars_device: arrays shorter than the batch");
  zkhip_gwc_plan p{};
  p.n_evals = (uint32_t)n_evals;
  p.n_sets = (uint32_t)n_sets;
  p.n_slots = plan.n_slots;
  p.set_rotation = plan.set_rotation.data();
  p.query_set = plan.query_set.data();
  p.query_pos = plan.query_pos.data();
  p.query_slot = plan.query_slot.data();
  check(zkhip_gwc_scalars_device(&p, evals.data(), points.data(), k, omega.l, n_proofs, rows_a.data(), rows_c.data(), nullptr), "gwc_scalars_device");
}
// A key's opening plan as the SHPLONK verifier groups it: the distinct rotations (the super points), the rotation sets as a CSR list over them,
// per polynomial slot its set and its position inside it, per query (evaluation q of a record) its slot and its super point
struct ShplonkPlan {
  std::vector<uint32_t> point_rotation, set_start, set_point, slot_set, slot_pos, query_slot, query_point;
};
// rows_a = [n_proofs][2 + n_slots + 1] over [H', H | slots | G], rows_c = [n_proofs][1]: the scalars of every proof's two accumulated points
// (layout: zkhip.h).  -> the status of every proof: 1 where the proof has no such row (its rows are zeros: verify it one by one)
inline std::vector<uint32_t> shplonk_scalars_device(const ShplonkPlan& plan, const DeviceVec& evals, const DeviceVec& points, uint32_t k, const Fr& omega, size_t n_proofs,
                                                    DeviceVec& rows_a, DeviceVec& rows_c) {
  const size_t n_evals = plan.query_slot.size(), n_slots = plan.slot_set.size();
  if (plan.query_point.size() != n_evals || plan.slot_pos.size() != n_slots || plan.set_start.size() < 2 || plan.set_point.size() != plan.set_start.back())
    throw std::invalid_argument("shplonk_scalars_device: the plan's arrays differ in length");
  if (evals.size() < n_proofs * n_evals || points.size() < n_proofs * 4 || rows_a.size() < n_proofs * (n_slots + 3) || rows_c.size() < n_proofs)
    throw std::invalid_argument("shplonk_scalars_device: arrays shorter than the batch");
  zkhip_shplonk_plan p{};
  p.n_evals = (uint32_t)n_evals;
  p.n_sets = (uint32_t)plan.set_start.size() - 1;
  p.n_slots = (uint32_t)n_slots;
  p.n_points = (uint32_t)plan.point_rotation.size();
  p.point_rotation = plan.point_rotation.data();
  p.set_start = plan.set_start.data();
  p.set_point = plan.set_point.data();
  p.slot_set = plan.slot_set.data();
  p.slot_pos = plan.slot_pos.data();
  p.query_slot = plan.query_slot.data();
  p.query_point = plan.query_point.data();
  std::vector<uint32_t> status(n_proofs, 0);
  if (n_proofs == 0) return status;
  void* d_status = nullptr;
  check(zkhip_alloc(n_proofs * sizeof(uint32_t) + 16, &d_status), "shplonk_scalars_device");
  struct release { void* p; ~release() { (void)zkhip_free(p); } } held{d_status};
  check(zkhip_shplonk_scalars_device(&p, evals.data(), points.data(), k, omega.l, n_proofs, rows_a.data(), rows_c.data(), d_status, nullptr), "shplonk_scalars_device");
  check(zkhip_download(status.data(), d_status, n_proofs * sizeof(uint32_t)), "shplonk_scalars_device");
  return status;
}
// out_own[i][j] = +- r[i] rows[i][j] for j < n_own; out_shared[j] = +- sum_i r[i] rows[i][n_own + j]
inline void fold_rows_device(const DeviceVec& rows, uint32_t n_cols, uint32_t n_own, const DeviceVec& r, bool negate, size_t n_rows, DeviceVec& out_own,
                             DeviceVec& out_shared) {
  if (n_own > n_cols || rows.size() < n_rows * n_cols || r.size() < n_rows || out_own.size() < n_rows * n_own || out_shared.size() < n_cols - n_own)
    throw std::invalid_argument("fold_rows_device: arrays shorter than the batch");
  check(zkhip_fr_fold_rows_device(rows.data(), n_cols, n_own, r.data(), negate ? 1 : 0, n_rows, out_own.data(), out_shared.data(), nullptr), "fold_rows_device");
}
// KZG accumulators (zkhip.h, "KZG accumulators").  out[i] = sum_j rows[i][j] * (j < n_own ? own[i * own_stride + j] : shared[j - n_own]): Jacobian points
inline void g1_row_msm_device(const DeviceVec& rows, size_t n_cols, const void* d_own_points, size_t n_own, size_t own_stride, const void* d_shared_points,
                              size_t n_rows, void* d_out_xyz) {
  if (rows.size() < n_rows * n_cols) throw std::invalid_argument("g1_row_msm_device: rows shorter than the batch");
  check(zkhip_g1_row_msm_device(rows.data(), n_cols, d_own_points, n_own, own_stride, d_shared_points, n_rows, d_out_xyz, nullptr), "g1_row_msm_device");
}
// n affine points <-> n x 6 limbs in Fr (3 limbs of 88 bits per coordinate); the host forms need no device
inline std::vector<Fr> kzg_limbs_encode(const std::vector<G1>& points) {
  std::vector<Fr> out(points.size() * 2 * ZKHIP_KZG_LIMBS);
  check(zkhip_kzg_limbs_encode(reinterpret_cast<const uint64_t*>(points.data()), points.size(), reinterpret_cast<uint64_t*>(out.data())), "kzg_limbs_encode");
  return out;
}
inline std::vector<uint32_t> kzg_limbs_decode(const std::vector<Fr>& limbs, std::vector<G1>& points) {
  const size_t n = limbs.size() / (2 * ZKHIP_KZG_LIMBS);
  points.resize(n);
  std::vector<uint32_t> status(n, 0);
  check(zkhip_kzg_limbs_decode(reinterpret_cast<const uint64_t*>(limbs.data()), n, reinterpret_cast<uint64_t*>(points.data()), status.data()), "kzg_limbs_decode");
  return status;
}
inline void kzg_limbs_encode_device(const void* d_affine, size_t n, DeviceVec& fr_out) {
  if (fr_out.size() < n * 2 * ZKHIP_KZG_LIMBS) throw std::invalid_argument("kzg_limbs_encode_device: output shorter than 6 n");
  check(zkhip_kzg_limbs_encode_device(d_affine, n, fr_out.data(), nullptr), "kzg_limbs_encode_device");
}
inline void kzg_limbs_decode_device(const DeviceVec& fr_in, size_t n, void* d_affine, void* d_status) {
  if (fr_in.size() < n * 2 * ZKHIP_KZG_LIMBS) throw std::invalid_argument("kzg_limbs_decode_device: input shorter than 6 n");
  check(zkhip_kzg_limbs_decode_device(fr_in.data(), n, d_affine, d_status, nullptr), "kzg_limbs_decode_device");
}
// Random field elements drawn in HBM (zkhip.h, "random field elements": element i of stream (seed, stream_id) is one ChaCha20 block reduced mod r).
// The library holds no entropy: `seed` comes from the caller's generator, and a (seed, stream_id, index) triple is never reused across proofs.
// out[j] = element first + j for every j < out.size(): the vanishing argument's random polynomial, never on the host
inline void random_fr_device(const std::array<uint8_t, 32>& seed, uint64_t stream_id, uint64_t first, DeviceVec& out) {
  check(zkhip_fr_random_device(seed.data(), stream_id, first, out.size(), out.data(), nullptr), "random_fr_device");
}
// the blinding tails of all `columns` in one call: row row0 + j of column c = element first + c * count + j, j < count; no other row is touched
inline void blind_rows_device(const std::vector<DeviceVec*>& columns, size_t row0, size_t count, const std::array<uint8_t, 32>& seed, uint64_t stream_id = 0,
                              uint64_t first = 0) {
  std::vector<const void*> ptrs;
  for (DeviceVec* c : columns) {
    if (c->size() < row0 + count) throw std::invalid_argument("blind_rows_device: column shorter than row0 + count");
    ptrs.push_back(c->data());
  }
  check(zkhip_fr_random_rows_device(seed.data(), stream_id, first, ptrs.data(), (uint32_t)ptrs.size(), row0, count, nullptr), "blind_rows_device");
}
// d_poly[index] -= value / d_poly[index] = 0: one-row programs on the element itself (no host round trip)
inline void sub_const_at(DeviceVec& poly, size_t index, const Fr& value) {
  zkhip_vm_insn insn{ZKHIP_OP_SUB, 0, 0, RowProgram::column(0, 0), RowProgram::constant(0), zkhip_vm_operand{}};
  const int32_t rot0 = 0;
  zkhip_vm_program p{};
  p.insns = &insn; p.n_insns = 1; p.constants = value.l; p.n_constants = 1; p.rotations = &rot0; p.n_rotations = 1; p.rot_scale = 1;
  const void* col = static_cast<const char*>(poly.data()) + index * sizeof(Fr);
  check(zkhip_fr_eval_rows_device(&p, &col, 1, 0, 0, const_cast<void*>(col), nullptr), "sub_const_at");
}
inline void zero_at(DeviceVec& poly, size_t index) {
  const Fr zero{};
  zkhip_vm_insn insn{ZKHIP_OP_MOV, 0, 0, RowProgram::constant(0), zkhip_vm_operand{}, zkhip_vm_operand{}};
  zkhip_vm_program p{};
  p.insns = &insn; p.n_insns = 1; p.constants = zero.l; p.n_constants = 1; p.rot_scale = 1;
  check(zkhip_fr_eval_rows_device(&p, nullptr, 0, 0, 0, static_cast<char*>(poly.data()) + index * sizeof(Fr), nullptr), "zero_at");
}
// `kate_division` keeping n coefficients (the top one zero): out = in / (X - root)
inline void divide_by_root(const DeviceVec& in, const Fr& root, DeviceVec& out) {
  check(zkhip_fr_kate_division_device(in.data(), in.size(), root.l, out.data(), nullptr), "kate_division");
  zero_at(out, in.size() - 1);
}
// `div_by_vanishing` keeping n coefficients (the top points.size() zero): out = in / prod_i (X - points[i]), one pass whatever the number of points
inline void divide_by_roots(const DeviceVec& in, const std::vector<Fr>& points, DeviceVec& out) {
  if (out.size() < in.size()) throw std::invalid_argument("divide_by_roots: output shorter than input");
  if (points.size() > ZKHIP_MAX_ROOTS) {                  // larger than any rotation set of halo2: the fold, through a temporary
    DeviceVec tmp(in.size());
    const DeviceVec* src = &in;
    DeviceVec* dst = points.size() % 2 ? &out : &tmp;     // the last division lands in `out`
    for (const Fr& z : points) { divide_by_root(*src, z, *dst); src = dst; dst = dst == &out ? &tmp : &out; }
    return;
  }
  check(zkhip_fr_divide_by_roots_device(in.data(), in.size(), points.empty() ? nullptr : points.data()->l, (uint32_t)points.size(), out.data(), nullptr, nullptr),
        "divide_by_roots");
}
// evaluations the queries lack: one batched eval_polynomial per distinct point
inline void evaluate_queries(std::vector<ProverQuery>& queries, size_t n) {
  std::vector<char> done(queries.size(), 0);
  for (size_t i = 0; i < queries.size(); i++) {
    if (queries[i].has_eval || done[i]) continue;
    std::vector<size_t> idx;
    std::vector<const void*> ptrs;
    for (size_t j = i; j < queries.size(); j++)
      if (!queries[j].has_eval && !done[j] && queries[j].point == queries[i].point) { idx.push_back(j); ptrs.push_back(queries[j].poly->data()); done[j] = 1; }
    DeviceVec d_out(idx.size());
    check(zkhip_fr_eval_polynomial_batch_device(ptrs.data(), ptrs.size(), n, queries[i].point.l, d_out.data(), nullptr), "eval_polynomial_batch");
    const std::vector<Fr> ev = d_out.to_host();
    for (size_t t = 0; t < idx.size(); t++) { queries[idx[t]].eval = ev[t]; queries[idx[t]].has_eval = true; }
  }
}
inline bool less_fr(const Fr& a, const Fr& b) {          // `Ord` of the canonical integers (a BTreeSet<Fr> iterates in this order)
  const Fr one_raw{{1, 0, 0, 0}};
  const Fr ca = mul(a, one_raw), cb = mul(b, one_raw);   // out of Montgomery form
  for (int i = 3; i >= 0; i--) if (ca.l[i] != cb.l[i]) return ca.l[i] < cb.l[i];
  return false;
}
// coefficients (low to high) of the polynomial of degree < m through (points[i], evals[i])
inline std::vector<Fr> lagrange_interpolate(const std::vector<Fr>& points, const std::vector<Fr>& evals) {
  const size_t m = points.size();
  std::vector<Fr> coeffs(m, Fr{});
  for (size_t i = 0; i < m; i++) {
    std::vector<Fr> num{one()};
    Fr den = one();
    for (size_t j = 0; j < m; j++) {
      if (j == i) continue;
      std::vector<Fr> next(num.size() + 1, Fr{});
      for (size_t t = 0; t < num.size(); t++) {
        next[t + 1] = add_fr(next[t + 1], num[t]);
        next[t] = sub_fr(next[t], mul(points[j], num[t]));
      }
      num = std::move(next);
      den = mul(den, sub_fr(points[i], points[j]));
    }
    const Fr scale = mul(evals[i], invert(den));
    for (size_t t = 0; t < m; t++) coeffs[t] = add_fr(coeffs[t], mul(scale, num[t]));
  }
  return coeffs;
}
// the Lagrange basis over `points`: basis[i] = coefficients (low to high) of the polynomial that is 1 at points[i] and 0 at the others.
// One inversion per point of the SET -- interpolating hundreds of polynomials over the same few points reuses it
// (interpolant of evals = sum_i evals[i] * basis[i]: lagrange_interpolate above, without its per-call inversions)
inline std::vector<std::vector<Fr>> lagrange_basis(const std::vector<Fr>& points) {
  std::vector<std::vector<Fr>> basis;
  std::vector<Fr> unit(points.size(), Fr{});
  for (size_t i = 0; i < points.size(); i++) {
    unit[i] = one();
    basis.push_back(lagrange_interpolate(points, unit));
    unit[i] = Fr{};
  }
  return basis;
}
inline Fr eval_small(const std::vector<Fr>& coeffs, const Fr& x) {
  Fr acc{};
  for (size_t i = coeffs.size(); i-- > 0;) acc = add_fr(mul(acc, x), coeffs[i]);
  return acc;
}
inline Fr vanishing_at(const std::vector<Fr>& points, const Fr& x) {
  Fr acc = one();
  for (const Fr& p : points) acc = mul(acc, sub_fr(x, p));
  return acc;
}
}  // namespace detail

// how a multi-open prover commits to n device-resident coefficients: a DeviceCommitter's prepared table, or any callable (the C entry
// points zkhip_multiopen_* commit against a base array registered with zkhip_register_bases)
using CommitFn = std::function<G1(const void* d_coeffs)>;
inline CommitFn commit_with(const DeviceCommitter& params) { return [&params](const void* d) { return params.commit(d); }; }

// `ProverGWC::create_proof`: for every distinct point z (order of first appearance): W_z = commit((sum_i v^i p_i - sum_i v^i e_i) / (X - z))
inline std::vector<G1> gwc_create_proof(const CommitFn& commit, uint32_t k, std::vector<ProverQuery> queries, const Fr& v) {
  const size_t n = (size_t)1 << k;
  detail::evaluate_queries(queries, n);
  std::vector<Fr> points;
  for (const auto& q : queries) {
    bool seen = false;
    for (const Fr& p : points) seen = seen || p == q.point;
    if (!seen) points.push_back(q.point);
  }
  DeviceVec batch(n), quot(n);
  std::vector<G1> out;
  for (const Fr& z : points) {
    std::vector<Fr> powers;
    std::vector<const DeviceVec*> cols;
    Fr pw = detail::one(), eval_batch{};
    for (const auto& q : queries) {
      if (!(q.point == z)) continue;
      powers.push_back(pw);
      cols.push_back(q.poly);
      eval_batch = detail::add_fr(eval_batch, detail::mul(pw, q.eval));
      pw = detail::mul(pw, v);
    }
    detail::linear_combination(powers, cols, k, batch);
    detail::sub_const_at(batch, 0, eval_batch);
    detail::divide_by_root(batch, z, quot);
    out.push_back(commit(quot.data()));
  }
  return out;
}
inline std::vector<G1> gwc_create_proof(const DeviceCommitter& params, uint32_t k, std::vector<ProverQuery> queries, const Fr& v) {
  return gwc_create_proof(commit_with(params), k, std::move(queries), v);
}

// `ProverSHPLONK::create_proof` in the two steps the transcript imposes (see zksnap_circuits_halo2_amd/multiopen.py for the formulas; the
// same operations in the same order): `begin` -- y and v are squeezed -- builds h(X) and returns its commitment H; the host writes H to the
// transcript and squeezes u; `finish` builds L(X) / (X - u) and returns H'.  The polynomials of the queries must stay alive in between.
class ShplonkProver {
 public:
  ShplonkProver(CommitFn commit, uint32_t k) : commit_(std::move(commit)), k_(k), n_((size_t)1 << k) {}

  G1 begin(std::vector<ProverQuery> queries, const Fr& y, const Fr& v) {
    if (begun_) throw std::logic_error("ShplonkProver::begin called twice");
    y_ = y;
    detail::evaluate_queries(queries, n_);
    // polynomial -> its set of points (order of first appearance), then sets of points -> their polynomials (order of first appearance)
    struct poly_pts { const DeviceVec* poly; std::vector<Fr> pts; };
    std::vector<poly_pts> by_poly;
    auto insert_sorted = [](std::vector<Fr>& vset, const Fr& p) {
      for (const Fr& e : vset) if (e == p) return;
      auto it = vset.begin();
      while (it != vset.end() && detail::less_fr(*it, p)) ++it;
      vset.insert(it, p);
    };
    for (const auto& q : queries) {
      insert_sorted(super_, q.point);
      bool found = false;
      for (auto& pp : by_poly) if (pp.poly == q.poly) { insert_sorted(pp.pts, q.point); found = true; break; }
      if (!found) by_poly.push_back({q.poly, {q.point}});
    }
    auto same = [](const std::vector<Fr>& a, const std::vector<Fr>& b) {
      if (a.size() != b.size()) return false;
      for (size_t i = 0; i < a.size(); i++) if (!(a[i] == b[i])) return false;
      return true;
    };
    for (const auto& pp : by_poly) {
      rotation_set* rs = nullptr;
      for (auto& s_ : sets_) if (same(s_.points, pp.pts)) rs = &s_;
      if (!rs) { sets_.push_back({pp.pts, {}, {}, detail::lagrange_basis(pp.pts)}); rs = &sets_.back(); }
      std::vector<Fr> ev;
      for (const Fr& z : pp.pts)
        for (const auto& q : queries) if (q.poly == pp.poly && q.point == z) { ev.push_back(q.eval); break; }
      rs->polys.push_back(pp.poly);
      rs->evals.push_back(std::move(ev));
    }
    // h(X)
    std::vector<const DeviceVec*> quotients;
    for (const auto& rs : sets_) {
      std::vector<Fr> ypow;
      Fr yp = detail::one();
      for (size_t j = 0; j < rs.polys.size(); j++) { ypow.push_back(yp); yp = detail::mul(yp, y); }
      DeviceVec* acc = fresh();
      DeviceVec* tmp = fresh();
      detail::linear_combination(ypow, rs.polys, k_, *acc);
      // the quotient by Z_S is the same polynomial whether or not the interpolant sum_j y^j R_j (degree < |S|) is subtracted first: one division
      // by the whole point set, no patching of the low coefficients
      detail::divide_by_roots(*acc, rs.points, *tmp);
      DeviceVec* src = tmp;
      quotients.push_back(src);
    }
    Fr vp = detail::one();
    for (size_t i = 0; i < sets_.size(); i++) { vpow_.push_back(vp); vp = detail::mul(vp, v); }
    h_x_ = fresh();
    detail::linear_combination(vpow_, quotients, k_, *h_x_);
    begun_ = true;
    return commit_(h_x_->data());
  }

  G1 finish(const Fr& u) {
    if (!begun_ || finished_) throw std::logic_error("ShplonkProver::finish without begin (or twice)");
    finished_ = true;
    std::vector<Fr> z_diffs;
    for (const auto& rs : sets_) {
      std::vector<Fr> diff;
      for (const Fr& p : super_) { bool in = false; for (const Fr& q : rs.points) in = in || q == p; if (!in) diff.push_back(p); }
      z_diffs.push_back(detail::vanishing_at(diff, u));
    }
    const Fr zt_eval = detail::vanishing_at(super_, u), norm = detail::invert(z_diffs[0]);
    std::vector<Fr> coeffs;
    std::vector<const DeviceVec*> cols;
    Fr constant{};
    for (size_t i = 0; i < sets_.size(); i++) {
      std::vector<Fr> basis_at_u;                          // R_ij(u) = sum_t evals[j][t] basis_t(u)
      for (const auto& b : sets_[i].basis) basis_at_u.push_back(detail::eval_small(b, u));
      Fr yp = detail::one();
      for (size_t j = 0; j < sets_[i].polys.size(); j++) {
        const Fr c = detail::mul(detail::mul(detail::mul(vpow_[i], z_diffs[i]), yp), norm);
        cols.push_back(sets_[i].polys[j]);
        coeffs.push_back(c);
        Fr r_at_u{};
        for (size_t t = 0; t < basis_at_u.size(); t++) r_at_u = detail::add_fr(r_at_u, detail::mul(sets_[i].evals[j][t], basis_at_u[t]));
        constant = detail::add_fr(constant, detail::mul(c, r_at_u));
        yp = detail::mul(yp, y_);
      }
    }
    cols.push_back(h_x_);
    coeffs.push_back(detail::neg_fr(detail::mul(zt_eval, norm)));
    DeviceVec* l_x = fresh();
    DeviceVec* tmp = fresh();
    detail::linear_combination(coeffs, cols, k_, *l_x);
    detail::sub_const_at(*l_x, 0, constant);
    {
      DeviceVec chk(1);
      check(zkhip_fr_eval_polynomial_device(l_x->data(), n_, u.l, chk.data(), nullptr), "eval_polynomial");
      const Fr r = chk.to_host()[0];
      if (!(r == Fr{})) throw std::runtime_error("SHPLONK: L(u) != 0 -- an evaluation does not belong to its polynomial");
    }
    detail::divide_by_root(*l_x, u, *tmp);
    return commit_(tmp->data());
  }

 private:
  struct rotation_set { std::vector<Fr> points; std::vector<const DeviceVec*> polys; std::vector<std::vector<Fr>> evals; std::vector<std::vector<Fr>> basis; };
  DeviceVec* fresh() { keep_.emplace_back(new DeviceVec(n_)); return keep_.back().get(); }
  CommitFn commit_;
  uint32_t k_;
  size_t n_;
  Fr y_{};
  std::vector<Fr> super_, vpow_;
  std::vector<rotation_set> sets_;
  std::vector<std::unique_ptr<DeviceVec>> keep_;
  DeviceVec* h_x_ = nullptr;
  bool begun_ = false, finished_ = false;
};

inline std::pair<G1, G1> shplonk_create_proof(const CommitFn& commit, uint32_t k, std::vector<ProverQuery> queries, const Fr& y, const Fr& v, const Fr& u) {
  ShplonkProver prover(commit, k);
  const G1 H = prover.begin(std::move(queries), y, v);
  const G1 Hp = prover.finish(u);
  return {H, Hp};
}
inline std::pair<G1, G1> shplonk_create_proof(const DeviceCommitter& params, uint32_t k, std::vector<ProverQuery> queries, const Fr& y, const Fr& v, const Fr& u) {
  return shplonk_create_proof(commit_with(params), k, std::move(queries), y, v, u);
}

// ---- the verifiers: `verify_proof`'s pairing and the two multi-open verifiers (zksnap_circuits_halo2_amd/multiopen.py, second half) ---------------
// `multi_miller_loop(..).final_exponentiation().is_identity()` [DEP halo2curves]: is prod_i e(g1[i], g2[i]) one?  At most ZKHIP_MAX_PAIRS pairs;
// a pair with an identity contributes 1; the points are not checked.  Only the verdict leaves the device.
inline bool pairing_check(const std::vector<G1Affine>& g1, const std::vector<G2Affine>& g2) {
  if (g1.size() != g2.size()) throw std::invalid_argument("pairing_check: g1.len() != g2.len()");
  int ok = 0;
  check(zkhip_pairing_check(g1.empty() ? nullptr : g1.data()->x, g2.empty() ? nullptr : g2.data()->x, g1.size(), &ok), "pairing_check");
  return ok != 0;
}

// `poly_id`: two DIFFERENT polynomials of a proof may have EQUAL commitments (two selector columns with the same rows); halo2 tells them apart by
// the address of the commitment (`CommitmentReference` compares pointers), here any non-null pointer, one per polynomial, does -- given for every
// query or for none.  Without it a polynomial is known by its commitment's bytes.
struct VerifierQuery {
  Fr point;
  G1 commitment;
  Fr eval;
  const void* poly_id = nullptr;
};

namespace detail {
inline bool same_point(const G1& a, const G1& b) { return std::memcmp(&a, &b, sizeof(G1)) == 0; }
inline bool same_poly(const VerifierQuery& a, const VerifierQuery& b) { return a.poly_id ? a.poly_id == b.poly_id : same_point(a.commitment, b.commitment); }
// What the set construction would otherwise hide (it keeps the first evaluation of a (polynomial, point) pair, as the prover's repeated queries agree
// by construction): false when one polynomial has two different evaluations at one point or two different commitments -- the verifiers then reject.
// poly_id on some queries and not on others throws: the keys would not be comparable.
inline bool queries_consistent(const std::vector<VerifierQuery>& queries) {
  size_t with_id = 0;
  for (const auto& q : queries) with_id += q.poly_id != nullptr;
  if (with_id != 0 && with_id != queries.size()) throw std::invalid_argument("VerifierQuery::poly_id: give it for every query or for none");
  for (size_t i = 0; i < queries.size(); i++)
    for (size_t j = 0; j < i; j++) {
      if (!same_poly(queries[i], queries[j])) continue;
      if (!same_point(queries[i].commitment, queries[j].commitment)) return false;
      if (queries[i].point == queries[j].point && !(queries[i].eval == queries[j].eval)) return false;
    }
  return true;
}
// sum_i scalars[i] * points[i] as an affine point: the points normalised, one small MSM, the result normalised
inline G1Affine g1_combination(const std::vector<Fr>& scalars, const std::vector<G1>& points) {
  if (scalars.size() != points.size() || points.empty()) throw std::invalid_argument("g1_combination: lengths");
  std::vector<G1Affine> aff(points.size());
  check(zkhip_g1_batch_normalize(points.data()->x, points.size(), aff.data()->x), "batch_normalize");
  const G1 acc = best_multiexp(scalars, aff);
  G1Affine out;
  check(zkhip_g1_batch_normalize(acc.x, 1, out.x), "batch_normalize");
  return out;
}
inline G1 to_g1(const G1Affine& a) {
  G1 p;
  std::memcpy(p.x, a.x, 32);
  std::memcpy(p.y, a.y, 32);
  const Fq one_q = fq_one();
  std::memcpy(p.z, one_q.l, 32);
  return p;
}
inline G2Affine g2_point(const std::array<uint64_t, 16>& w) { G2Affine p; std::memcpy(&p, w.data(), 128); return p; }
// e(left, g2) e(right_negated, [s]_2) = 1
inline bool final_pairing(const ParamsKZG& params, const G1Affine& left, const G1Affine& right_negated) {
  return pairing_check({left, right_negated}, {g2_point(params.g2()), g2_point(params.s_g2())});
}
}  // namespace detail

// `ParamsKZG::verify_opening` of the Python mirror: e(C - value G + z W, g2) e(-W, [s]_2) = 1, W a commitment to (p(X) - value) / (X - z)
inline bool verify_opening(const ParamsKZG& params, const G1& commitment, const Fr& z, const Fr& value, const G1& witness) {
  const G1Affine left = detail::g1_combination({detail::one(), detail::neg_fr(value), z}, {commitment, detail::to_g1(params.get_g()[0]), witness});
  const G1Affine right_neg = detail::g1_combination({detail::neg_fr(detail::one())}, {witness});
  return detail::final_pairing(params, left, right_neg);
}

// `VerifierGWC::verify_proof`: e(sum_i u^i W_i, [s]_2) = e(sum_i u^i (z_i W_i + sum_j v^j C_ij - (sum_j v^j e_ij) G), g2); sets as gwc_create_proof
class VerifierGWC {
 public:
  explicit VerifierGWC(const ParamsKZG& params) : params_(params) {}
  bool verify_proof(const std::vector<VerifierQuery>& queries, const std::vector<G1>& witnesses, const Fr& v, const Fr& u) const {
    if (!detail::queries_consistent(queries)) return false;
    std::vector<Fr> points;
    for (const auto& q : queries) {
      bool seen = false;
      for (const Fr& p : points) seen = seen || p == q.point;
      if (!seen) points.push_back(q.point);
    }
    if (points.size() != witnesses.size()) throw std::invalid_argument("VerifierGWC: one witness per distinct point");
    std::vector<Fr> left, right;
    std::vector<G1> right_points = witnesses;
    Fr ui = detail::one(), g_scalar{};
    for (const Fr& z : points) {
      left.push_back(detail::neg_fr(ui));
      right.push_back(detail::mul(ui, z));
      ui = detail::mul(ui, u);
    }
    ui = detail::one();
    for (const Fr& z : points) {
      Fr vj = detail::one();
      for (const auto& q : queries) {
        if (!(q.point == z)) continue;
        const Fr c = detail::mul(ui, vj);
        right.push_back(c);
        right_points.push_back(q.commitment);
        g_scalar = detail::sub_fr(g_scalar, detail::mul(c, q.eval));
        vj = detail::mul(vj, v);
      }
      ui = detail::mul(ui, u);
    }
    right.push_back(g_scalar);
    right_points.push_back(detail::to_g1(params_.get_g()[0]));
    return detail::final_pairing(params_, detail::g1_combination(right, right_points), detail::g1_combination(left, witnesses));
  }

 private:
  const ParamsKZG& params_;
};

// `VerifierSHPLONK::verify_proof`: e(Lc + u H', g2) e(-H', [s]_2) = 1 with Lc = sum_ij c_ij (C_ij - R_ij(u) G) - Z_T(u) / Z_{T \ S_0}(u) H and
// c_ij = v^i Z_{T \ S_i}(u) y^j / Z_{T \ S_0}(u); rotation sets as ShplonkProver::begin builds them, keyed by commitment
class VerifierSHPLONK {
 public:
  explicit VerifierSHPLONK(const ParamsKZG& params) : params_(params) {}
  bool verify_proof(const std::vector<VerifierQuery>& queries, const G1& H, const G1& Hp, const Fr& y, const Fr& v, const Fr& u) const {
    if (!detail::queries_consistent(queries)) return false;
    struct poly_pts { const VerifierQuery* poly; std::vector<Fr> pts; };       // a polynomial is named by its first query
    struct rotation_set { std::vector<Fr> points; std::vector<const VerifierQuery*> polys; std::vector<std::vector<Fr>> evals; };
    std::vector<poly_pts> by_poly;
    std::vector<Fr> super;
    auto insert_sorted = [](std::vector<Fr>& vset, const Fr& p) {
      for (const Fr& e : vset) if (e == p) return;
      auto it = vset.begin();
      while (it != vset.end() && detail::less_fr(*it, p)) ++it;
      vset.insert(it, p);
    };
    for (const auto& q : queries) {
      insert_sorted(super, q.point);
      bool found = false;
      for (auto& pp : by_poly) if (detail::same_poly(*pp.poly, q)) { insert_sorted(pp.pts, q.point); found = true; break; }
      if (!found) by_poly.push_back({&q, {q.point}});
    }
    auto same = [](const std::vector<Fr>& a, const std::vector<Fr>& b) {
      if (a.size() != b.size()) return false;
      for (size_t i = 0; i < a.size(); i++) if (!(a[i] == b[i])) return false;
      return true;
    };
    std::vector<rotation_set> sets;
    for (const auto& pp : by_poly) {
      rotation_set* rs = nullptr;
      for (auto& s_ : sets) if (same(s_.points, pp.pts)) rs = &s_;
      if (!rs) { sets.push_back({pp.pts, {}, {}}); rs = &sets.back(); }
      std::vector<Fr> ev;
      for (const Fr& z : pp.pts)
        for (const auto& q : queries) if (detail::same_poly(q, *pp.poly) && q.point == z) { ev.push_back(q.eval); break; }
      rs->polys.push_back(pp.poly);
      rs->evals.push_back(std::move(ev));
    }
    std::vector<Fr> z_diffs;
    for (const auto& rs : sets) {
      std::vector<Fr> diff;
      for (const Fr& p : super) { bool in = false; for (const Fr& q : rs.points) in = in || q == p; if (!in) diff.push_back(p); }
      z_diffs.push_back(detail::vanishing_at(diff, u));
    }
    const Fr norm = detail::invert(z_diffs[0]);
    std::vector<Fr> scalars;
    std::vector<G1> points;
    Fr g_scalar{}, vi = detail::one();
    for (size_t i = 0; i < sets.size(); i++) {
      Fr yj = detail::one();
      for (size_t j = 0; j < sets[i].polys.size(); j++) {
        const Fr c = detail::mul(detail::mul(detail::mul(vi, z_diffs[i]), yj), norm);
        scalars.push_back(c);
        points.push_back(sets[i].polys[j]->commitment);
        g_scalar = detail::sub_fr(g_scalar, detail::mul(c, detail::eval_small(detail::lagrange_interpolate(sets[i].points, sets[i].evals[j]), u)));
        yj = detail::mul(yj, y);
      }
      vi = detail::mul(vi, v);
    }
    scalars.push_back(g_scalar);
    points.push_back(detail::to_g1(params_.get_g()[0]));
    scalars.push_back(detail::neg_fr(detail::mul(detail::vanishing_at(super, u), norm)));
    points.push_back(H);
    scalars.push_back(u);
    points.push_back(Hp);
    return detail::final_pairing(params_, detail::g1_combination(scalars, points), detail::g1_combination({detail::neg_fr(detail::one())}, {Hp}));
  }

 private:
  const ParamsKZG& params_;
};

}  // namespace halo2
}  // namespace zkhip

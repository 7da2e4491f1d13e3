// The SHPLONK accumulation scalars of a batch verifier (include/zkhip.h, "the batch verifier"): the row of scalars that [DEP] halo2-axiom
// poly/kzg/multiopen/shplonk/verifier.rs accumulates per proof, multiopen.shplonk_accumulate in Python integers.  That function interpolates every
// polynomial's evaluations over its rotation set and inverts once per point; here the interpolation is written as Lagrange weights, which a circuit
// fixes up to one inversion per proof.  The PLAN (fixed by the circuit and k): the super point set T of distinct rotations; the rotation sets
// S_0 .. S_(n_sets-1), polynomials grouped by their set of rotations, sets and the polynomials inside a set in order of first appearance; per
// polynomial slot p its set(p) and its position pos(p) inside that set; per query its slot and its rotation.  Per proof, with w the 2^k-th root:
//
//   d_t     = u - x w^rot_t                                   for t in T
//   Z_i     = prod of d_t over T \ S_i (the empty product is 1)             Z_T = prod of d_t over T
//   inv     = 1 / (x Z_0)         norm = inv x = 1 / Z_0        xinv = inv Z_0 = 1 / x                       ONE inversion
//   w_i     = v^i Z_i norm
//   L_(i,a) = w_i (prod of d_b over b in S_i, b != a) xinv^(|S_i| - 1) c_(i,a)       c_(i,a) = 1 / prod of (w^rot_a - w^rot_b), b in S_i, b != a
//
// (c_(i,a) depends on the plan and k alone: the host computes it when it marshals the plan) and the row of A over [H', H | slots | G] is
//
//   u  |  -Z_T norm  |  w_set(p) y^pos(p)  |  -sum_q L_(set(slot(q)), rot(q)) y^pos(slot(q)) e_q
//
// x Z_0 = 0 (x = 0, or u on a point outside S_0) has no such row: the proof's status is 1 and its rows are zeros.  A proof is one workgroup:
//
//   points       one lane per super point: d_t; the y^(2^b) table (b < 16) and v^i (i < n_sets)
//   sets         one lane per set: Z_i; one lane per (set, point) pair: the partial numerator; one lane: Z_T
//   inversion    one lane: inv, norm, xinv and the powers of xinv up to the longest set
//   weights      w_i per set, L_(i,a) per pair
//   columns      one lane per column; G as strided partial sums joined pairwise (gwc_fold.hpp's gf_g_lane over the L table in place of the u
//                table and the y table in place of the v table: a query's word is gf_query_word(pair, pos), a slot's gf_query_word(set, pos))
//
// This file is the arithmetic of one lane, for host and device (tests/cpp/shplonk_fold_host_check.cpp runs it lane by lane under ASan + UBSan),
// and the layout of the plan as the kernel reads it; the exchange through LDS is shplonk_fold.hip's.  Values are in the internal form of fp29.hpp.
#pragma once
#include "gwc_fold.hpp"

namespace zkhip {

constexpr uint32_t SHPLONK_MAX_SETS = 64;          // rotation sets of a plan: the v table of a workgroup
constexpr uint32_t SHPLONK_MAX_POINTS = 64;        // super points: a set is a 64-bit mask over them
constexpr uint32_t SHPLONK_MAX_PAIRS = 256;        // (set, point) pairs: the L table of a workgroup
constexpr uint32_t SHPLONK_THREADS = GWC_THREADS;  // lanes of a proof's workgroup (SHPLONK_THREADS_SHORT for a plan that one wave covers)
constexpr uint32_t SHPLONK_THREADS_SHORT = GWC_THREADS_SHORT;
static_assert(SHPLONK_MAX_PAIRS <= 65536 && SHPLONK_MAX_SETS <= 65536, "a pair or a set is the upper half of a query word");

// The plan as the kernel reads it, in 32-bit words: a head of SF_HEAD_WORDS counts, then
//   omega^rot per point (8 words each) | c per pair (8 words each) | set_start [n_sets + 1] | a word per pair (its point below, its set above
//   bit 16) | a word per slot (gf_query_word(set, pos)) | a word per query (gf_query_word(pair, pos of its slot))
// The counts travel in the head: the kernel keeps six pointers and nothing else.
constexpr uint32_t SF_HEAD_WORDS = 8;              // n_evals, n_sets, n_slots, n_points, n_pairs, longest set, 0, 0
struct sf_layout {
  uint32_t n_evals, n_sets, n_slots, n_points, n_pairs, longest;
  uint32_t point_omega, pair_coeff, set_start, pair_word, slot_word, query_word, words;      // offsets in words; the two element tables are 32-byte aligned
};
ZK_HD sf_layout sf_layout_of(uint32_t n_evals, uint32_t n_sets, uint32_t n_slots, uint32_t n_points, uint32_t n_pairs, uint32_t longest) {
  sf_layout l;
  l.n_evals = n_evals; l.n_sets = n_sets; l.n_slots = n_slots; l.n_points = n_points; l.n_pairs = n_pairs; l.longest = longest;
  l.point_omega = SF_HEAD_WORDS;
  l.pair_coeff = l.point_omega + n_points * 8;
  l.set_start = l.pair_coeff + n_pairs * 8;
  l.pair_word = l.set_start + n_sets + 1;
  l.slot_word = l.pair_word + n_pairs;
  l.query_word = l.slot_word + n_slots;
  l.words = l.query_word + n_evals;                // at most 8 + 512 + 2048 + 65 + 256 + 65536 + 65527: no wrap
  return l;
}
ZK_HD sf_layout sf_layout_read(const uint32_t* head) { return sf_layout_of(head[0], head[1], head[2], head[3], head[4], head[5]); }

// d_t = u - x omega^rot_t.  u, x < 2p; w_lazy: omega^rot_t just unpacked (< 32p).  N form, < 5p: a factor fe_mul accepts beside any value < 32p
template <class P>
ZK_HD fe sf_diff(const fe& u, const fe& x, const fe& w_lazy) { return ip_sub<P>(u, fe_mul<P>(x, w_lazy)); }      // 2p 32p / (169 p) + p < 2p, then 2p + 3p

// the points of a set as a mask over the super points: entries begin .. end - 1 of the pair list; word(j) yields pair j's word
template <class W>
ZK_HD uint64_t sf_set_mask(uint32_t begin, uint32_t end, W&& word) {
  uint64_t mask = 0;
  for (uint32_t j = begin; j < end; j++) mask |= (uint64_t)1 << (word(j) & 0xffffu);       // a point is below SHPLONK_MAX_POINTS = 64
  return mask;
}

// the product of d_t over the super points outside `mask`: Z_i for a set's mask, Z_T for the empty one.  d_t < 5p; < 2p (no factor: one)
template <class P>
ZK_HD fe sf_outside(const fe* diff, uint32_t n_points, uint64_t mask) {
  fe acc = fe_one<P>();
  for (uint32_t t = 0; t < n_points; t++)
    if (!((mask >> t) & 1u)) acc = fe_mul<P>(acc, diff[t]);                                // 2p 5p / (169 p) + p < 2p
  return acc;
}

// the partial numerator of pair `skip`: the product of d_b over the other pairs begin .. end - 1 of its set; < 2p (a set of one point: one)
template <class P, class W>
ZK_HD fe sf_numerator(const fe* diff, uint32_t begin, uint32_t end, uint32_t skip, W&& word) {
  fe acc = fe_one<P>();
  for (uint32_t j = begin; j < end; j++)
    if (j != skip) acc = fe_mul<P>(acc, diff[word(j) & 0xffffu]);                          // 2p 5p / (169 p) + p < 2p
  return acc;
}

// the one inversion of a proof.  x, z0 < 2p.  bad: x Z_0 = 0, nothing is inverted that could be (fe_inverse leaves a zero as it is)
struct sf_inverse {
  fe norm, xinv;                                   // 1 / Z_0 and 1 / x, < 2p
  bool bad;
};
template <class P>
ZK_HD sf_inverse sf_invert(const fe& x, const fe& z0) {
  sf_inverse r;
  const fe xz = fe_mul<P>(x, z0);                                                          // 2p 2p / (169 p) + p < 2p
  r.bad = fe_mulout_is_zero<P>(xz);                                                        // (an N-form value below 2p: 0 or p)
  const fe inv = fe_inverse<P>(xz);                                                        // < 2p
  r.norm = fe_mul<P>(inv, x);                                                              // 2p 2p / (169 p) + p < 2p
  r.xinv = fe_mul<P>(inv, z0);
  return r;
}

// xinv^j for j < count into table[0 .. count - 1] (count >= 1: the longest set has a point); entries < 2p
template <class P>
ZK_HD void sf_xinv_powers(fe* table, uint32_t count, const fe& xinv) {
  table[0] = fe_one<P>();
  for (uint32_t j = 1; j < count; j++) table[j] = fe_mul<P>(table[j - 1], xinv);           // 2p 2p / (169 p) + p < 2p
}

// w_i = v^i Z_i norm; all < 2p
template <class P>
ZK_HD fe sf_weight(const fe& vi, const fe& zi, const fe& norm) { return fe_mul<P>(fe_mul<P>(vi, zi), norm); }      // 2p 2p / (169 p) + p < 2p, twice

// L_(i,a) = w_i numerator xinv^(|S_i| - 1) c_(i,a).  wi, numerator, xpow < 2p; c_lazy: c_(i,a) just unpacked (< 32p); < 2p
template <class P>
ZK_HD fe sf_lagrange(const fe& wi, const fe& numerator, const fe& xpow, const fe& c_lazy) {
  return fe_mul<P>(fe_mul<P>(fe_mul<P>(wi, numerator), xpow), c_lazy);                     // 2p 2p / (169 p) + p < 2p, twice, then 2p 32p / (169 p) + p < 2p
}

// the H column: -Z_T norm, canonical (Z_T = 0: an exact zero)
template <class P>
ZK_HD fe sf_h_column(const fe& zt, const fe& norm) { return gf_neg<P>(fe_canon_lt2p<P>(fe_mul<P>(zt, norm))); }      // 2p 2p / (169 p) + p < 2p

// ---- the host's side of a plan: c_(i,a) -------------------------------------------------------------------------------------------------------
// 1 / prod of (w_a - w_b) over the other points b of the set; omega_of(point): omega^rot of a super point, < 2p; the set's points are entries
// begin .. end - 1 of `set_point`.  Distinct rotations below 2^k and an omega of order 2^k: no factor is zero (a zero product is left as zero)
template <class P, class O>
ZK_HD fe sf_pair_coefficient(const uint32_t* set_point, uint32_t begin, uint32_t end, uint32_t at, O&& omega_of) {
  fe acc = fe_one<P>();
  const fe wa = omega_of(set_point[at]);
  for (uint32_t j = begin; j < end; j++)
    if (j != at) acc = fe_mul<P>(acc, ip_sub<P>(wa, omega_of(set_point[j])));              // 2p 5p / (169 p) + p < 2p
  return fe_inverse<P>(acc);
}

}  // namespace zkhip

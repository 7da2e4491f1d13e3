// The scalar side of a batch verifier (include/zkhip.h, "the batch verifier"): the GWC accumulation scalars of every proof of a batch, and the
// scaling and folding of such rows by per-proof random multipliers.  [DEP] halo2-axiom poly/kzg/multiopen/gwc/verifier.rs accumulates, per proof,
//
//   A = sum_i u^i (z_i W_i + sum_j v^j C_ij - (sum_j v^j e_ij) G)        C = sum_i u^i W_i            z_i = x omega^rot_i
//
// over the proof's point sets i (one witness W_i each) and the queries j of a set; multiopen.gwc_accumulate states the same in Python integers.
// A circuit fixes which query lies in which set, at which position, and which polynomial it opens: the PLAN.  What changes from proof to proof is
// (x, v, u) and the evaluations.  So a proof is one workgroup over a plan that is shared by the batch:
//
//   tables       v^(2^b), b < 16, and u^i, i < n_sets, one lane per entry, kept in LDS (positions are below 2^16, sets at most 64)
//   columns      one lane per output column: a witness column is two products, a polynomial's column walks the CSR list of its queries
//                (u^set v^pos each, v^pos by square-and-multiply from the table): no atomics
//   G            lane t takes the queries t, t + T, ...; the partial sums are joined pairwise through LDS
//
// and a fold is, per shared column, lanes over the rows i = t, t + T, ... joined the same way.  This file is the arithmetic of one lane and of
// one join, for host and device (tests/cpp/gwc_fold_host_check.cpp runs it lane by lane under ASan + UBSan); the exchange through LDS and the
// memory layout are gwc_fold.hip's.
//
// Two forms of a value occur.  The GWC functions work in the internal form of fp29.hpp (a 2^261) and end in fe_to_ext.  The fold functions
// never leave the external form (a 2^256): with r unpacked by fe_unpack<5> (the integer r 2^261, below 32p) and a by fe_unpack<0> (a 2^256,
// below p), fe_mul gives r a 2^256, the product in external form, and fe_one (the integer 2^261 mod p) is the factor that leaves a sum as it is.
#pragma once
#include "identity_points.hpp"

namespace zkhip {

constexpr uint32_t GWC_MAX_SETS = 64;              // point sets of a plan: the u table of a workgroup
constexpr uint32_t GWC_MAX_EVALS = 65527;          // evaluations (= queries) of a proof, as in the identity call
constexpr uint32_t GWC_MAX_SLOTS = 65536;          // opened polynomials of a plan
constexpr uint32_t GWC_V_BITS = 16;                // positions are below 2^16: v^(2^b) for b < 16
constexpr uint32_t GWC_THREADS = 256;              // lanes of a proof's workgroup (GWC_THREADS_SHORT for a plan that one wave covers)
constexpr uint32_t GWC_THREADS_SHORT = 64;

constexpr uint32_t FOLD_THREADS = 256;             // lanes of a fold workgroup
constexpr uint32_t FOLD_LANE_ROWS = 16;            // rows a lane sums at most
constexpr uint32_t FOLD_SPAN = FOLD_THREADS * FOLD_LANE_ROWS;      // rows of a column one workgroup sums: above it a second level joins the workgroups' sums
constexpr uint64_t FOLD_MAX_ROWS = (uint64_t)1 << 24;              // = FOLD_SPAN^2: the second level is one workgroup
static_assert((uint64_t)FOLD_SPAN * FOLD_SPAN >= FOLD_MAX_ROWS, "two levels cover every batch the call admits");

// a query of the plan as the kernel reads it: its position in the low 16 bits, its set above them
ZK_HD uint32_t gf_query_word(uint32_t set, uint32_t pos) { return pos | (set << 16); }

// an element just unpacked from its external words (below 32p, limbs below 2^29) -> below 2p
template <class P>
ZK_HD fe gf_reduce(const fe& lazy) { return fe_mul<P>(fe_one<P>(), lazy); }               // p 32p / (169 p) + p < 2p

// v^(2^b) by b squarings; v < 2p, result < 2p
template <class P>
ZK_HD fe gf_v_entry(fe v, uint32_t b) {
  for (uint32_t i = 0; i < b; i++) v = fe_sqr<P>(v);                                      // 2p 2p / (169 p) + p < 2p
  return v;
}

// v^e for e < 2^16 from the table of v^(2^b); entries < 2p, result < 2p (e = 0: one)
template <class P>
ZK_HD fe gf_v_pow(const fe* vtab, uint32_t e) {
  fe acc = fe_one<P>();
  for (uint32_t b = 0; e; b++, e >>= 1)
    if (e & 1u) acc = fe_mul<P>(acc, vtab[b]);                                            // 2p 2p / (169 p) + p < 2p
  return acc;
}

// u^set v^pos of a query word; < 2p
template <class P>
ZK_HD fe gf_coeff(const fe* upow, const fe* vtab, uint32_t word) { return fe_mul<P>(upow[word >> 16], gf_v_pow<P>(vtab, word & 0xffffu)); }

// column i < n_sets of a row of A: u^i x omega^rot_i.  ui, x < 2p; w_lazy: omega^rot_i just unpacked (< 32p)
template <class P>
ZK_HD fe gf_witness_column(const fe& ui, const fe& x, const fe& w_lazy) {
  return fe_mul<P>(fe_mul<P>(ui, x), w_lazy);                                             // 2p 2p / (169 p) + p < 2p, then 2p 32p / (169 p) + p < 2p
}

// the column of a polynomial: the sum of u^set v^pos over entries begin .. end - 1 of its query list; word(i) yields entry i's query word
template <class P, class Q>
ZK_HD fe gf_slot_column(const fe* upow, const fe* vtab, uint32_t begin, uint32_t end, Q&& word) {
  const fe one = fe_one<P>();
  fe acc = fe_zero();
  for (uint32_t i = begin; i < end; i++) {
    const uint32_t w = word(i);
    acc = fe_mul_add<P>(acc, one, upow[w >> 16], gf_v_pow<P>(vtab, w & 0xffffu));         // (2p p + 2p 2p) / (169 p) + p < 2p
  }
  return acc;
}

// lane t of T of the G column: sum over q = t, t + T, ... < n_evals of u^set v^pos e_q, canonical.  word(q): the query word; value(q): e_q just
// unpacked (< 32p).  n_evals <= 65527 and T <= 256: q does not wrap.
template <class P, class Q, class V>
ZK_HD fe gf_g_lane(const fe* upow, const fe* vtab, uint32_t n_evals, uint32_t t, uint32_t T, Q&& word, V&& value) {
  const fe one = fe_one<P>();
  fe acc = fe_zero();
  for (uint32_t q = t; q < n_evals; q += T)
    acc = fe_mul_add<P>(acc, one, gf_coeff<P>(upow, vtab, word(q)), value(q));            // (2p p + 2p 32p) / (169 p) + p < 2p
  return fe_canon_lt2p<P>(acc);
}

// a + b for canonical a, b: canonical.  Symmetric, and exact in either form of a value.
template <class P>
ZK_HD fe gf_join(const fe& a, const fe& b) { return fe_canon_lt2p<P>(fe_norm(fe_add(a, b))); }      // limbs < 2^30 before the carries, value < 2p

// -a for canonical a: canonical (p - a; zero stays zero)
template <class P>
ZK_HD fe gf_neg(const fe& a) {
  fe d;
  int32_t borrow = 0;
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const int32_t t = (int32_t)P::P[i] - (int32_t)a.l[i] + borrow;
    borrow = t >> 31;                                                                     // 0 or -1; a < p: none leaves the top limb
    d.l[i] = (uint32_t)t & LMASK;
    any |= a.l[i];
  }
#pragma unroll
  for (int i = 0; i < NL; i++) d.l[i] = any ? d.l[i] : 0u;
  return d;
}

// ---- the fold, in external form throughout: r5 = fe_unpack<5> of a multiplier, a0 = fe_unpack<0> of an element ----
// +- r a, canonical
template <class P>
ZK_HD fe gf_scale(const fe& r5, const fe& a0, bool negate) {
  const fe m = fe_canon_lt2p<P>(fe_mul<P>(r5, a0));                                       // 32p p / (169 p) + p < 2p
  return negate ? gf_neg<P>(m) : m;
}

// lane t of T of one column's sum over `count` rows: sum over i = t, t + T, ... < count of r_i a_i, canonical.  mult(i): r_i unpacked with <5>;
// elem(i): a_i unpacked with <0>.  count <= FOLD_SPAN: i does not wrap.
template <class P, class R, class A>
ZK_HD fe gf_fold_lane(uint32_t count, uint32_t t, uint32_t T, R&& mult, A&& elem) {
  const fe one = fe_one<P>();
  fe acc = fe_zero();
  for (uint32_t i = t; i < count; i += T) acc = fe_mul_add<P>(acc, one, mult(i), elem(i));          // (2p p + 32p p) / (169 p) + p < 2p
  return fe_canon_lt2p<P>(acc);
}

// lane t of T of the second level: the join of the canonical partial sums t, t + T, ... < count
template <class P, class A>
ZK_HD fe gf_join_lane(uint32_t count, uint32_t t, uint32_t T, A&& partial) {
  fe acc = fe_zero();
  for (uint32_t i = t; i < count; i += T) acc = gf_join<P>(acc, partial(i));
  return acc;
}

#if defined(__HIPCC__)
// ---- what the kernels of gwc_fold.hip and shplonk_fold.hip share on the device: element loads and stores, and the join through LDS ----
ZK_D fe gf_load5(const uint32_t* p) {
  uint32_t w[8];
  load_words(p, w);
  return fe_from_ext_lazy(w);
}

ZK_D fe gf_load0(const uint32_t* p) {
  uint32_t w[8];
  load_words(p, w);
  return fe_unpack<0>(w);
}

ZK_D void gf_store_ext(uint32_t* p, const fe& internal) {
  uint32_t w[8];
  fe_to_ext<FrParams>(internal, w);
  store_words(p, w);
}

ZK_D void gf_store_packed(uint32_t* p, const fe& canonical) {
  uint32_t w[8];
  fe_pack(canonical, w);
  store_words(p, w);
}

// the pairwise joins of a workgroup's T canonical values (T a power of two); the sum is left in part[0]
ZK_D void gf_join_block(fe* part, uint32_t t, uint32_t T) {
  __syncthreads();
  for (uint32_t d = T >> 1; d; d >>= 1) {
    if (t < d) part[t] = gf_join<FrParams>(part[t], part[t + d]);
    __syncthreads();
  }
}
#endif

}  // namespace zkhip

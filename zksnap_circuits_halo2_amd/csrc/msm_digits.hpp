// Scalar -> signed window digits of the MSM (msm.hip step 1), host and device: the window layout, the conversion of a caller's Montgomery
// word into the canonical integer, one step of the generic recoding, and the recoding specialised on a layout known at compile time.
// tests/cpp/digits_host_check.cpp runs all of it on the host against an independent big-integer reference.
#pragma once
#include <cstdint>
#include "fp29.hpp"

namespace zkhip {

// Balanced windows of the wide prepared path.  W = ceil(256 / c) windows of c bits cover W c >= 256 bits, and with uniform widths the surplus sits
// in the top window: at c = 20 it holds 15 bits, so its 2^20 digits fall into the lowest 2^14 buckets, which then hold ~90 entries = two tasks
// (a combining addition each, and the longest chains of the accumulation) while every other bucket holds ~26.  Here the last `narrow` = W c - 256
// windows are c - 1 bits wide instead (c = 20: nine windows of 20 bits, four of 19): every window fills at least half of the bucket range.  The top
// window still ends at bit 256, two bits above any scalar, so the signed recoding never carries out of it.  Offsets: win_off(w).
struct win_layout { int c, W, narrow; };
ZK_HD constexpr int win_bits(const win_layout& L, int w) { return w < L.W - L.narrow ? L.c : L.c - 1; }
ZK_HD constexpr int win_off(const win_layout& L, int w) { return w <= L.W - L.narrow ? w * L.c : (L.W - L.narrow) * L.c + (w - (L.W - L.narrow)) * (L.c - 1); }

// A caller's scalar a, as the 256-bit word x = a 2^256 mod r, -> the integer a in canonical limbs.
//   in : any 256-bit x.  Unpacked with the 5-bit shift it is the integer 32 x < 2^261 in N form (nine limbs below 2^29): "x 2^5 is the
//        internal form" of fp29.hpp, so the reduction alone divides by 2^261 -- no product by the constant 2^5
//   out: fe_mont_reduce gives N form, value <= r; one conditional subtraction makes it canonical: every limb below 2^29, value < r < 2^254
ZK_HD fe fr_ext_to_canon(const uint32_t (&x)[8]) { return fe_canon_lt2p<FrParams>(fe_mont_reduce<FrParams>(fe_unpack<5>(x))); }

// One window of the signed recoding: v = the window's bits + the carry in; v >= 2^(cw-1) becomes v - 2^cw and carries.  |digit| <= 2^(cw-1).
ZK_HD int32_t recode_step(uint32_t v, int cw, uint32_t& carry) {
  v += carry;
  carry = v >= (1u << (cw - 1)) ? 1u : 0u;
  return (int32_t)v - (int32_t)(carry << cw);
}

// The generic form: window `win` of a run-time layout, cut from the packed words of the canonical integer.
ZK_HD int32_t recode_window(const uint32_t (&w)[8], const win_layout& lay, int win, uint32_t& carry) {
  const int bit = win_off(lay, win), cw = win_bits(lay, win);
  uint32_t v = 0;
  if (bit < 256) {
    const int wi = bit >> 5, sh = bit & 31;
    uint64_t two = w[wi];
    if (wi + 1 < 8) two |= (uint64_t)w[wi + 1] << 32;
    v = (uint32_t)(two >> sh) & ((1u << cw) - 1);
  }
  return recode_step(v, cw, carry);
}

// The layout as template arguments: every offset, width and limb index is a constant, and the digits come from the canonical limbs
// themselves -- a window of at most 29 bits touches two limbs.  Same digits as recode_window on fe_pack(s), digit for digit.
template <int C, int W, int NARROW>
ZK_HD void recode_fixed(const fe& s /* canonical */, int32_t (&d)[W]) {
  static_assert(C >= 2 && C <= LB && NARROW >= 0 && NARROW <= W, "a window spans at most two limbs");
  constexpr win_layout lay{C, W, NARROW};
  uint32_t carry = 0;
#pragma unroll
  for (int win = 0; win < W; win++) {
    const int bit = win_off(lay, win), cw = win_bits(lay, win), li = bit / LB, sh = bit % LB;
    uint32_t v = 0;
    if (li < NL) {
      v = s.l[li] >> sh;
      if (sh + cw > LB && li + 1 < NL) v |= s.l[li + 1] << (LB - sh);
      v &= (1u << cw) - 1;
    }
    d[win] = recode_step(v, cw, carry);
  }
}

}  // namespace zkhip

// PLUME signing on secp256k1 (include/zkhip.h, "PLUME nullifiers on secp256k1", `sign`): `gen_test_nullifier` of the reference
// (voter_tests/src/lib.rs:88-119) for a whole batch in one launch, so that a population of distinct voters can be made where the verifier, the
// members tree and the nullifier tree read it.  The arithmetic is secp256k1.hpp, sha256.hpp and secp256k1_h2c.hpp, which a host program runs
// unchanged (plume_sign there).  A translation unit of its own: it compiles beside plume.hip.
//
//   k_plume_sign     TWO adjacent lanes per voter, 32 voters per wavefront, as k_plume_verify.  A voter costs four ladders and two images of
//                    the map: lane 0 carries the scalar sk and lane 1 the scalar r through ONE ladder site that a two-trip loop passes twice
//                    -- over G (lane 0: pk = sk G, lane 1: r G), then over H (lane 0: N = sk H, lane 1: r H).  After each trip the lanes
//                    exchange the affine results (16 words).  Between the trips both lanes derive H = H(msg, pk) exactly as the verifier does:
//                    each maps one of u0 / u1 and they exchange the image (24 words).  Behind the second trip both lanes hash the challenge and
//                    form s = r + sk c mod n alike; lane 0 stores.
//
// A malformed input (sk or r outside [1, n)) never leaves the straight line: the scalar 1 stands in, the status 2 and the zeros are chosen at
// the store.  The single-scalar ladder (table {P}) is used: the joint one would carry a second scalar and two more table entries for nothing.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "secp256k1_h2c.hpp"
#include "plume_io.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

__device__ __forceinline__ sk_aff ps_swap_point(const sk_aff& a) {
  sk_aff o;
  o.x = pm_swap(a.x);
  o.y = pm_swap(a.y);
  return o;
}
__device__ __forceinline__ sk_aff ps_sel_point(bool c, const sk_aff& a, const sk_aff& b) {
  sk_aff o;
  o.x = sk_sel(c, a.x, b.x);
  o.y = sk_sel(c, a.y, b.y);
  return o;
}

__global__ void __launch_bounds__(PLUME_BLOCK) k_plume_sign(const h2c_prefix pre, const uint64_t* __restrict__ sk, const uint64_t* __restrict__ r, size_t count,
                                                            uint64_t* __restrict__ pk, uint64_t* __restrict__ nullifier, uint64_t* __restrict__ s,
                                                            uint64_t* __restrict__ c, uint32_t* __restrict__ status, uint64_t* __restrict__ h_out) {
  const size_t v = (size_t)blockIdx.x * PLUME_VOTERS + (threadIdx.x >> 1);
  if (v >= count) return;                                     // both lanes of a voter leave together
  const bool second = threadIdx.x & 1u;
  const sk_fe SK = pm_load(sk + v * 4), R = pm_load(r + v * 4);
  const bool sk_ok = plume_secret_ok(SK), r_ok = plume_secret_ok(R);
  const sk_fe one = sk_small(1);
  const sk_fe key = sk_sel(sk_ok, SK, one), nonce = sk_sel(r_ok, R, one);
  const sk_fe mine = sk_sel(second, nonce, key);              // the scalar this lane carries through both trips

  plume_signature sig;
  sk_aff rg, rh;                                              // r G and r H
  sk_aff base = sk_generator();
#pragma unroll 1
  for (int trip = 0; trip < 2; trip++) {
    const sk_aff got = sk_to_affine(sk_mul_proj(mine, base));
    const sk_aff other = ps_swap_point(got);
    const sk_aff by_key = ps_sel_point(second, other, got), by_nonce = ps_sel_point(second, got, other);
    if (trip == 0) {
      sig.pk = by_key;
      rg = by_nonce;
      sk_fe u0, u1;
      h2c_hash_to_field(pre, sig.pk, u0, u1);
      const sk_pt image = h2c_map(sk_sel(second, u1, u0));
      sk_pt twin;
      twin.X = pm_swap(image.X);
      twin.Y = pm_swap(image.Y);
      twin.Z = pm_swap(image.Z);
      sig.h = sk_to_affine(sk_padd(image, twin));             // the formulas are symmetric and the results canonical: both lanes hold the same H
      base = sig.h;
    } else {
      sig.nullifier = by_key;
      rh = by_nonce;
    }
  }
  plume_sign_finish(key, nonce, rg, rh, sig);
  if (!second) {
    const bool ok = sk_ok && r_ok;
    const sk_fe zero = sk_small(0);
    pm_store_point(pk + v * 8, sig.pk, ok);
    pm_store_point(nullifier + v * 8, sig.nullifier, ok);
    pm_store(s + v * 4, sk_sel(ok, sig.s, zero));
    pm_store(c + v * 4, sk_sel(ok, sig.c, zero));
    status[v] = ok ? PLUME_OK : PLUME_MALFORMED;
    if (h_out) pm_store_point(h_out + v * 8, sig.h, ok);
  }
}

int plume_sign_device(const h2c_prefix& pre, const uint64_t* d_sk, const uint64_t* d_r, size_t count, uint64_t* d_pk, uint64_t* d_nullifier, uint64_t* d_s, uint64_t* d_c,
                      uint32_t* d_status, uint64_t* d_h_out, hipStream_t stream) {
  if (count == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_plume_sign, pm_grid(count, PLUME_VOTERS), dim3(PLUME_BLOCK), 0, stream, pre, d_sk, d_r, count, d_pk, d_nullifier, d_s, d_c, d_status, d_h_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

// PLUME nullifiers on secp256k1 (include/zkhip.h, "PLUME nullifiers on secp256k1"): the check the reference makes of every ballot before it builds
// a round's inputs (`verify_nullifier`, reference voter_tests/src/lib.rs:57-86, called from aggregator/src/utils.rs:289-290), for a whole batch
// in one launch.  The arithmetic is secp256k1.hpp, sha256.hpp and secp256k1_h2c.hpp, which a host program runs unchanged.
//
//   k_sk_lincomb      one lane per element: out[i] = a[i] P[i] + b[i] Q[i] by the joint ladder.
//   k_sk_h2c          one lane per key: H(msg, pk[i]) -- both images of the map, their sum, one inversion.
//   k_plume_verify    TWO adjacent lanes per voter, 32 voters per wavefront.  A voter costs two images of the map and two ladders, and each
//                     pair is independent and equal in cost: lane 0 maps u0 and computes A = s G - c pk, lane 1 maps u1 and computes
//                     B = s H - c N.  They exchange through the wavefront's cross-lane moves twice (the image, 24 words; the affine
//                     result, 16 words); what is cheap -- the validity tests, `expand_message_xmd`, the sum of the images and its
//                     inversion, the challenge hash -- both lanes do alike, so the lanes never part ways except inside the map's
//                     second square root.  Lane 0 stores the verdict and H and speaks for the voter in the report (check_report.hpp).
//
// A malformed input never leaves the straight line: the generator stands in for a point that is off the curve, the verdict 2 and the zeros are
// chosen at the store.  Blocks are one wavefront: a lane runs about 10^4 field products, so a batch is spread over the SIMDs as thinly as it goes.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "secp256k1_h2c.hpp"
#include "plume_io.hpp"
#include "check_report.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

__global__ void __launch_bounds__(PLUME_BLOCK) k_sk_lincomb(const uint64_t* __restrict__ a, const uint64_t* __restrict__ p, const uint64_t* __restrict__ b,
                                                            const uint64_t* __restrict__ q, size_t count, uint64_t* __restrict__ out, uint32_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * PLUME_BLOCK + threadIdx.x;
  if (i >= count) return;
  const sk_aff P = pm_load_point(p + i * 8), Q = pm_load_point(q + i * 8);
  const bool p_ok = sk_on_curve(P), q_ok = sk_on_curve(Q);
  const sk_aff r = sk_lincomb(pm_load(a + i * 4), pm_point_or_generator(P, p_ok), pm_load(b + i * 4), pm_point_or_generator(Q, q_ok));
  pm_store_point(out + i * 8, r, p_ok && q_ok);
  status[i] = p_ok && q_ok ? PLUME_OK : PLUME_MALFORMED;
}

__global__ void __launch_bounds__(PLUME_BLOCK) k_sk_h2c(const h2c_prefix pre, const uint64_t* __restrict__ pk, size_t count, uint64_t* __restrict__ out,
                                                        uint32_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * PLUME_BLOCK + threadIdx.x;
  if (i >= count) return;
  const sk_aff K = pm_load_point(pk + i * 8);
  const bool ok = sk_on_curve(K);
  pm_store_point(out + i * 8, h2c_hash(pre, pm_point_or_generator(K, ok)), ok);
  status[i] = ok ? PLUME_OK : PLUME_MALFORMED;
}

__global__ void __launch_bounds__(PLUME_BLOCK) k_plume_verify(const h2c_prefix pre, const uint64_t* __restrict__ pk, const uint64_t* __restrict__ nullifier,
                                                              const uint64_t* __restrict__ s, const uint64_t* __restrict__ c, size_t count,
                                                              uint32_t* __restrict__ status, unsigned long long* __restrict__ report, uint64_t* __restrict__ h_out) {
  const size_t v = (size_t)blockIdx.x * PLUME_VOTERS + (threadIdx.x >> 1);
  if (v >= count) return;                                     // both lanes of a voter leave together
  const bool second = threadIdx.x & 1u;
  const sk_aff K = pm_load_point(pk + v * 8), Nf = pm_load_point(nullifier + v * 8);
  const sk_fe S = pm_load(s + v * 4), C = pm_load(c + v * 4);
  const bool pk_ok = sk_on_curve(K), n_ok = sk_on_curve(Nf);
  const bool all_ok = pk_ok && n_ok && sk_scalar_ok(S) && sk_scalar_ok(C);
  const sk_aff key = pm_point_or_generator(K, pk_ok), nul = pm_point_or_generator(Nf, n_ok);

  sk_fe u0, u1;
  h2c_hash_to_field(pre, key, u0, u1);
  const sk_pt mine = h2c_map(sk_sel(second, u1, u0));
  sk_pt other;
  other.X = pm_swap(mine.X);
  other.Y = pm_swap(mine.Y);
  other.Z = pm_swap(mine.Z);
  const sk_aff h = sk_to_affine(sk_padd(mine, other));        // the formulas are symmetric and the results canonical: both lanes hold the same H

  const sk_aff g = sk_generator();
  sk_aff base, sub;
  base.x = sk_sel(second, h.x, g.x);
  base.y = sk_sel(second, h.y, g.y);
  sub.x = sk_sel(second, nul.x, key.x);
  sub.y = sk_sel(second, nul.y, key.y);
  const sk_aff r = sk_lincomb(S, base, C, sk_neg_affine(sub)); // lane 0: A = s G - c pk, lane 1: B = s H - c N
  sk_aff o;
  o.x = pm_swap(r.x);
  o.y = pm_swap(r.y);
  sk_aff A, B;
  A.x = sk_sel(second, o.x, r.x);
  A.y = sk_sel(second, o.y, r.y);
  B.x = sk_sel(second, r.x, o.x);
  B.y = sk_sel(second, r.y, o.y);
  const bool accepted = plume_challenge_is(key, h, nul, A, B, C);
  const uint32_t verdict = !all_ok ? PLUME_MALFORMED : accepted ? PLUME_OK : PLUME_REFUSED;
  if (!second) {
    status[v] = verdict;
    if (h_out) pm_store_point(h_out + v * 8, h, pk_ok);
  }
  check_report_wave(!second && verdict != PLUME_OK, v, report);
}

int secp256k1_lincomb_device(const uint64_t* d_a, const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_q, size_t count, uint64_t* d_out, uint32_t* d_status,
                             hipStream_t stream) {
  if (count == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_sk_lincomb, pm_grid(count, PLUME_BLOCK), dim3(PLUME_BLOCK), 0, stream, d_a, d_p, d_b, d_q, count, d_out, d_status);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int secp256k1_hash_to_curve_device(const h2c_prefix& pre, const uint64_t* d_pk, size_t count, uint64_t* d_out, uint32_t* d_status, hipStream_t stream) {
  if (count == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_sk_h2c, pm_grid(count, PLUME_BLOCK), dim3(PLUME_BLOCK), 0, stream, pre, d_pk, count, d_out, d_status);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// the report is initialised by the call (0 failures, no first); count == 0 writes nothing else
int plume_verify_device(const h2c_prefix& pre, const uint64_t* d_pk, const uint64_t* d_nullifier, const uint64_t* d_s, const uint64_t* d_c, size_t count, uint32_t* d_status,
                        void* d_report, uint64_t* d_h_out, hipStream_t stream) {
  const int rc = check_reports_init_device(d_report, 1, stream);
  if (rc != ZKHIP_OK || count == 0) return rc;
  hipLaunchKernelGGL(k_plume_verify, pm_grid(count, PLUME_VOTERS), dim3(PLUME_BLOCK), 0, stream, pre, d_pk, d_nullifier, d_s, d_c, count, d_status,
                     (unsigned long long*)d_report, d_h_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

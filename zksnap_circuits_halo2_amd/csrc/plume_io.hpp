// What the PLUME kernels (plume.hip, plume_sign.hip) share: the wavefront's shape, loads and stores of canonical words, and the exchange
// between the two lanes of a voter.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "secp256k1.hpp"

namespace zkhip {

constexpr int PLUME_BLOCK = 64;
constexpr int PLUME_VOTERS = PLUME_BLOCK / 2;   // voters of a workgroup of k_plume_verify and k_plume_sign

__device__ __forceinline__ sk_fe pm_load(const uint64_t* __restrict__ p) {
  uint64_t w[4];
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = p[i];
  return sk_from_words(w);
}
__device__ __forceinline__ void pm_store(uint64_t* __restrict__ p, const sk_fe& a) {
  uint64_t w[4];
  sk_to_words(a, w);
#pragma unroll
  for (int i = 0; i < 4; i++) p[i] = w[i];
}
__device__ __forceinline__ sk_aff pm_load_point(const uint64_t* __restrict__ p) {
  sk_aff a;
  a.x = pm_load(p);
  a.y = pm_load(p + 4);
  return a;
}
// a, or (0, 0) where keep is false
__device__ __forceinline__ void pm_store_point(uint64_t* __restrict__ p, const sk_aff& a, bool keep) {
  const sk_fe zero = sk_small(0);
  pm_store(p, sk_sel(keep, a.x, zero));
  pm_store(p + 4, sk_sel(keep, a.y, zero));
}
__device__ __forceinline__ sk_aff pm_point_or_generator(const sk_aff& a, bool ok) {
  const sk_aff g = sk_generator();
  sk_aff r;
  r.x = sk_sel(ok, a.x, g.x);
  r.y = sk_sel(ok, a.y, g.y);
  return r;
}
// the neighbour's value: lanes 2k and 2k + 1 swap
__device__ __forceinline__ sk_fe pm_swap(const sk_fe& a) {
  sk_fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = (uint32_t)__shfl_xor((int)a.l[i], 1);
  return r;
}

static inline dim3 pm_grid(size_t items, int per_block) { return dim3((unsigned)((items + per_block - 1) / per_block)); }

}  // namespace zkhip

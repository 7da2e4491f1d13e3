// Poseidon on the device (include/zkhip.h, "Poseidon"): one lane per message or tree node over fp29.hpp's Fr, the permutation body of
// poseidon.hpp.  The reference hashes its membership trees level by level on one CPU thread (`MerkleTree::new`,
// /root/reference/voter/src/merkletree/native.rs:30-49): two permutations per node, 828 field products each, no node of a level depending
// on another.
//
//   k_poseidon_hash_many  n messages of `width` Montgomery Fr, row-major -> n digests: a fresh sponge per lane.
//   k_poseidon_hash_points  n secp256k1 points as the PLUME calls leave them in HBM -> the nullifier tree's values or the members tree's leaves:
//                         the host packers' byte chunks are cut in registers, so a signed population never returns to the host to be packed.
//   k_poseidon_merkle     the n - 1 inner nodes of a tree over n leaves in ONE launch.  A workgroup of POSEIDON_SUBTREE / 2 lanes takes a run
//                         of POSEIDON_SUBTREE neighbouring elements of a level and folds it PM_DEPTH levels up -- level 1 from global
//                         memory, level 2 through LDS, whole waves busy on both -- and hands its POSEIDON_SUBTREE >> PM_DEPTH nodes on
//                         with a ticket: the workgroup that brings the LAST share of the next run folds that run in turn.  A level of at
//                         most POSEIDON_SUBTREE elements is one run, folded all the way to the root.  No launch per level, no workgroup
//                         left alone with everything above the first subtrees, and a hand-off (microseconds) is nothing beside a hash.
//
// The table (round constants, matrix, 2^64, 1) is device memory read at indices that depend on the round counter only: scalar loads.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "poseidon.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

constexpr int PH_BLOCK = 128;
constexpr uint32_t PM_SUBTREE = ZKHIP_POSEIDON_SUBTREE;    // leaves (or handed-on roots) one workgroup folds
constexpr int PM_BLOCK = PM_SUBTREE / 2;
constexpr uint32_t PM_DEPTH = 2;                           // levels a workgroup folds before it hands on: the narrowest one still fills a wave
static_assert((PM_SUBTREE & (PM_SUBTREE - 1)) == 0 && (PM_SUBTREE >> PM_DEPTH) % 64 == 0, "a subtree is a power of two and every level folded from it whole waves");

// external Montgomery-256 words -> Montgomery-261, N form, < 1.2 r
__device__ __forceinline__ fe ps_from_words(const uint32_t (&w)[8]) { return fe_mul<FrParams>(fe_one<FrParams>(), fe_from_ext_lazy(w)); }
__device__ __forceinline__ fe ps_load(const uint32_t* p) {
  uint32_t w[8];
  load_words(p, w);
  return ps_from_words(w);
}
__device__ __forceinline__ void ps_store(uint32_t* p, const fe& v) {
  uint32_t w[8];
  fe_to_ext<FrParams>(v, w);
  store_words(p, w);
}

__global__ void __launch_bounds__(PH_BLOCK) k_poseidon_hash_many(const uint32_t* __restrict__ in, size_t n, uint32_t width, uint32_t* __restrict__ out,
                                                                 const fe* __restrict__ tab) {
  const size_t i = (size_t)blockIdx.x * PH_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* msg = in + i * width * 8;
  const fe h = poseidon_hash<poseidon_dev_field>(width, tab, [&](uint32_t j) { return ps_load(msg + (size_t)j * 8); });
  ps_store(out + i * 8, h);
}

// The 11-, 11- and 10-byte little-endian chunks of a 32-byte coordinate (eight words): bits 0 .. 87, 88 .. 175 and 176 .. 255.  All three are cut
// with shifts known when the code is compiled and `which` picks one by conditional moves, so that nothing is indexed at run time.
__device__ __forceinline__ void ps_chunk(const uint32_t (&w)[8], uint32_t which, uint32_t (&out)[3]) {
  const uint32_t a[3] = {w[0], w[1], w[2] & 0x00ffffffu};
  const uint32_t b[3] = {(w[2] >> 24) | (w[3] << 8), (w[3] >> 24) | (w[4] << 8), ((w[4] >> 24) | (w[5] << 8)) & 0x00ffffffu};
  const uint32_t c[3] = {(w[5] >> 16) | (w[6] << 16), (w[6] >> 16) | (w[7] << 16), w[7] >> 16};
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = which == 0 ? a[k] : which == 1 ? b[k] : c[k];
}
// a canonical integer below 2^96 -> Montgomery-261, N form: v 2^522 2^-261, the product far below r^2, so the result is < 1.1 r
__device__ __forceinline__ fe ps_from_small(const uint32_t (&v)[3]) {
  const uint32_t w[8] = {v[0], v[1], v[2], 0, 0, 0, 0, 0};
  fe r2;
#pragma unroll
  for (int i = 0; i < NL; i++) r2.l[i] = FrParams::R2[i];
  return fe_mul<FrParams>(r2, fe_unpack<0>(w));
}

// One lane per secp256k1 point (x then y, eight canonical words each, ANY 256-bit values): the message the host packers build
// (poseidon.py `compress_nullifier`, `pack_member`) is cut from the point in registers and hashed.  layout 0: (2 + (y & 1), the three chunks
// of x), width 4; layout 1: the chunks of x, then those of y, width 6.  The layout is uniform over the launch.
__global__ void __launch_bounds__(PH_BLOCK) k_poseidon_hash_points(const uint32_t* __restrict__ points, size_t n, uint32_t layout, uint32_t* __restrict__ out,
                                                                   const fe* __restrict__ tab) {
  const size_t i = (size_t)blockIdx.x * PH_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], y[8];
  load_words(points + i * 16, x);
  load_words(points + i * 16 + 8, y);
  const fe h = poseidon_hash<poseidon_dev_field>(layout ? 6u : 4u, tab, [&](uint32_t j) {
    // layout 0: element 0 is the tag and element j > 0 chunk j - 1 of x; layout 1: element j is chunk j % 3 of x (j < 3) or y
    const bool of_y = layout && j >= 3;
    const uint32_t which = layout ? (of_y ? j - 3 : j) : j - 1;
    uint32_t w[8], v[3];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = of_y ? y[k] : x[k];
    ps_chunk(w, which, v);
    const bool tag = !layout && j == 0;
    v[0] = tag ? 2u + (y[0] & 1u) : v[0];
    v[1] = tag ? 0u : v[1];
    v[2] = tag ? 0u : v[2];
    return ps_from_small(v);
  });
  ps_store(out + i * 8, h);
}

// Level L >= 1 of a tree over n leaves holds n >> L nodes and starts at node n - (n >> (L - 1)) of `nodes`.
__device__ __forceinline__ size_t pm_level_start(size_t n, uint32_t L) { return n - (n >> (L - 1)); }

// tickets: one uint32 per run of handed-on nodes, every tier's runs behind those of the tier before; zero before the launch.
__global__ void __launch_bounds__(PM_BLOCK) k_poseidon_merkle(const uint32_t* __restrict__ leaves, size_t n, uint32_t* nodes, uint32_t* tickets,
                                                              const fe* __restrict__ tab) {
  __shared__ __align__(16) uint32_t lds[PM_BLOCK][8];      // the level just made, external words; [0][0] doubles as the ticket's verdict
  const uint32_t t = threadIdx.x;
  const uint32_t* src = leaves;                            // the level this workgroup folds from, and its number
  uint32_t level = 0;
  size_t count = n;                                        // elements of that level
  size_t g = blockIdx.x;                                   // which run of it
  size_t ticket_base = 0;
  for (;;) {
    const bool top = count <= PM_SUBTREE;                  // one run is the whole level: fold it to the root
    const uint32_t c = top ? (uint32_t)count : PM_SUBTREE; // elements of the run: a power of two >= 2
    const uint32_t out = top ? 1u : PM_SUBTREE >> PM_DEPTH;
    uint32_t lv = 1;
    for (uint32_t half = c >> 1; half >= out; half >>= 1, lv++) {
      uint32_t lw[8], rw[8];
      if (t < half) {
        if (lv == 1) {
          load_words(src + (g * c + 2 * t) * 8, lw);
          load_words(src + (g * c + 2 * t + 1) * 8, rw);
        } else {
          load_words(&lds[2 * t][0], lw);
          load_words(&lds[2 * t + 1][0], rw);
        }
      }
      __syncthreads();                                     // every lane has read its two children
      if (t < half) {
        const fe h = poseidon_hash<poseidon_dev_field>(2, tab, [&](uint32_t j) {
          uint32_t w[8];
#pragma unroll
          for (int k = 0; k < 8; k++) w[k] = j ? rw[k] : lw[k];
          return ps_from_words(w);
        });
        uint32_t w[8];
        fe_to_ext<FrParams>(h, w);
        store_words(&lds[t][0], w);
        store_words(nodes + (pm_level_start(n, level + lv) + g * half + t) * 8, w);
      }
      __syncthreads();
    }
    level += lv - 1;
    count >>= lv - 1;                                      // elements at `level` now
    if (top) return;                                       // lane 0 has written the root
    // Hand the `out` nodes on: every storing wave drains its stores, lane 0 releases them to the device and draws the ticket; the last
    // arriver of a run acquires before any lane of its workgroup loads the run.
    const uint32_t arrivals = (uint32_t)(count < PM_SUBTREE ? count : PM_SUBTREE) / out;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the fence's own wait can be dropped by the compiler; this one cannot
      const uint32_t drawn = __hip_atomic_fetch_add(tickets + ticket_base + g / arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t last = drawn == arrivals - 1;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      lds[0][0] = last;
    }
    __syncthreads();
    const uint32_t last = lds[0][0];
    __syncthreads();                                       // lds is written again below
    if (!last) return;
    ticket_base += (count + PM_SUBTREE - 1) / PM_SUBTREE;
    g /= arrivals;
    src = nodes + pm_level_start(n, level) * 8;
  }
}

int poseidon_hash_many_device(const uint32_t* d_in, size_t n, uint32_t width, uint32_t* d_out, const uint32_t* d_tab, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_poseidon_hash_many, dim3((unsigned)((n + PH_BLOCK - 1) / PH_BLOCK)), dim3(PH_BLOCK), 0, stream, d_in, n, width, d_out, (const fe*)d_tab);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int poseidon_hash_points_device(const uint32_t* d_points, size_t n, uint32_t layout, uint32_t* d_out, const uint32_t* d_tab, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_poseidon_hash_points, dim3((unsigned)((n + PH_BLOCK - 1) / PH_BLOCK)), dim3(PH_BLOCK), 0, stream, d_points, n, layout, d_out, (const fe*)d_tab);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

size_t poseidon_merkle_workspace(size_t n) {
  size_t tickets = 1;
  for (size_t count = n; count > PM_SUBTREE;) {
    count >>= PM_DEPTH;
    tickets += (count + PM_SUBTREE - 1) / PM_SUBTREE;
  }
  return tickets * sizeof(uint32_t);
}

// n a power of two >= 2; ws: poseidon_merkle_workspace(n) bytes
int poseidon_merkle_device(const uint32_t* d_leaves, size_t n, uint32_t* d_nodes, const uint32_t* d_tab, void* ws, size_t ws_bytes, hipStream_t stream) {
  const size_t need = poseidon_merkle_workspace(n);
  if (ws_bytes < need) { set_error("poseidon_merkle: workspace too small"); return ZKHIP_EINVAL; }
  HIPCHK(hipMemsetAsync(ws, 0, need, stream));
  const size_t blocks = n <= PM_SUBTREE ? 1 : n / PM_SUBTREE;
  hipLaunchKernelGGL(k_poseidon_merkle, dim3((unsigned)blocks), dim3(PM_BLOCK), 0, stream, d_leaves, n, d_nodes, (uint32_t*)ws, (const fe*)d_tab);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

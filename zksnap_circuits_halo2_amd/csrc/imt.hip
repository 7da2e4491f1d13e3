// The indexed Merkle tree on the device (include/zkhip.h, "indexed Merkle tree"): the witnesses of a whole batch of insertions, level by level.
// The reference rebuilds the whole tree twice per insertion (`IndexedMerkleTree::new`, /root/reference/aggregator/src/utils.rs:101-197); here an
// insertion is two EVENTS, (leaf, time 2 i) for the low leaf and (leaf, time 2 i + 1) for the new one, and every level is one launch with one
// lane per event over the permutation body of poseidon.hpp:
//
//   k_imt_leaves   the width-3 hash of every event's preimage, in the order (leaf, time) the host sorted the keys into.
//   k_imt_level    level L -> L + 1.  The events of a level lie sorted by (node, time).  A lane looks for the latest earlier event on its sibling
//                  node with one binary search over the keys; none: the sibling's value in the tree as it was before the batch.  That value is the
//                  proof element of the level; hash(left, right) is the event's value one level up.  The runs of two sibling nodes are neighbours
//                  in the order, and the same search says how many sibling events precede the lane's own: its place in the MERGED run of the
//                  parent is p + q - m (p its own place, q the search's answer, m where the right child's run begins), so the order one level up
//                  is written by this launch and nothing is sorted again.  The launch also SETTLES level L - 1: the last event of every run of
//                  that level stores its value (at level 0 its preimage too) into the tree.  Level L - 1 was read by the launch before and
//                  is read by none after it, and this launch reads level L only: no launch reads a cell one of its own lanes writes.
//   k_imt_finish   settles level depth - 1 and the root, and copies the roots out of the top level, which is in time order.
//
// depth + 2 launches per batch, 2 B independent hashes in each but the last; three sets of (keys, values) used in turn.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "poseidon.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

constexpr int IMT_BLOCK = 64;          // one wave: a batch is latency-bound, its lanes spread over as many SIMDs as there are

__device__ __forceinline__ fe imt_from_words(const uint32_t (&w)[8]) { return fe_mul<FrParams>(fe_one<FrParams>(), fe_from_ext_lazy(w)); }
__device__ __forceinline__ fe imt_load(const uint32_t* p) {
  uint32_t w[8];
  load_words(p, w);
  return imt_from_words(w);
}
__device__ __forceinline__ void imt_copy(uint32_t* dst, const uint32_t* src, int elements) {
  for (int j = 0; j < elements; j++) {
    uint32_t w[8];
    load_words(src + 8 * j, w);
    store_words(dst + 8 * j, w);
  }
}
// the first place of `keys` (ascending, n of them) whose key is not below `key`
__device__ __forceinline__ uint32_t imt_lower_bound(const uint64_t* __restrict__ keys, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(IMT_BLOCK) k_imt_fill(uint32_t* __restrict__ dst, size_t n, uint4 lo, uint4 hi) {
  const size_t i = (size_t)blockIdx.x * IMT_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint4* q = reinterpret_cast<uint4*>(dst + i * 8);
  q[0] = lo;
  q[1] = hi;
}

// keys: (leaf << 32) | time, ascending; pre: the preimage an event leaves behind, 3 elements, by TIME
__global__ void __launch_bounds__(IMT_BLOCK) k_imt_leaves(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pre, uint32_t n_ev, uint32_t* __restrict__ vals,
                                                          uint32_t* __restrict__ out_new_leaves, const fe* __restrict__ tab) {
  const uint32_t p = blockIdx.x * IMT_BLOCK + threadIdx.x;
  if (p >= n_ev) return;
  const uint32_t t = (uint32_t)keys[p];
  const uint32_t* msg = pre + (size_t)t * 24;
  const fe h = poseidon_hash<poseidon_dev_field>(3, tab, [&](uint32_t j) { return imt_load(msg + (size_t)j * 8); });
  uint32_t w[8];
  fe_to_ext<FrParams>(h, w);
  store_words(vals + (size_t)p * 8, w);
  if (out_new_leaves && (t & 1)) imt_copy(out_new_leaves + (size_t)(t >> 1) * 24, msg, 3);
}

// The last event of every run of (keys, vals) stores its value into cells[node]; with `preimages` (level 0) also the preimage it leaves behind.
__device__ __forceinline__ void imt_settle(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t p, uint32_t n_ev, uint32_t* __restrict__ cells,
                                           const uint32_t* __restrict__ pre, uint32_t* __restrict__ preimages) {
  const uint64_t key = keys[p];
  const uint32_t x = (uint32_t)(key >> 32);
  if (p + 1 < n_ev && (uint32_t)(keys[p + 1] >> 32) == x) return;
  imt_copy(cells + (size_t)x * 8, vals + (size_t)p * 8, 1);
  if (preimages) imt_copy(preimages + (size_t)x * 24, pre + (size_t)(uint32_t)key * 24, 3);
}

// level: the tree's level L before the batch (cell x at word 8 x), read.  keys_in / vals_in: level L's events; keys_out / vals_out: level L + 1's,
// every place written exactly once.  keys_prev / vals_prev (null at L = 0): level L - 1's events, settled into `below`, the tree's level L - 1.
__global__ void __launch_bounds__(IMT_BLOCK) k_imt_level(const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t n_ev,
                                                         const uint32_t* __restrict__ level, uint64_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                         const uint64_t* __restrict__ keys_prev, const uint32_t* __restrict__ vals_prev, uint32_t* __restrict__ below,
                                                         const uint32_t* __restrict__ pre, uint32_t* __restrict__ preimages, uint32_t* __restrict__ out_low_proofs,
                                                         uint32_t* __restrict__ out_new_proofs, uint32_t depth, uint32_t L, const fe* __restrict__ tab) {
  const uint32_t p = blockIdx.x * IMT_BLOCK + threadIdx.x;
  if (p >= n_ev) return;
  if (keys_prev) imt_settle(keys_prev, vals_prev, p, n_ev, below, pre, L == 1 ? preimages : nullptr);
  const uint64_t key = keys_in[p];
  const uint32_t x = (uint32_t)(key >> 32), t = (uint32_t)key, sib = x ^ 1u;
  const uint32_t q = imt_lower_bound(keys_in, n_ev, ((uint64_t)sib << 32) | t);     // events before (sib, t)
  const uint32_t m = imt_lower_bound(keys_in, n_ev, (uint64_t)(x | 1u) << 32);      // where the right child's run begins
  const bool earlier = q > 0 && (uint32_t)(keys_in[q - 1] >> 32) == sib;            // the sibling has an event before this one
  uint32_t own[8], other[8];
  load_words(vals_in + (size_t)p * 8, own);
  load_words(earlier ? vals_in + (size_t)(q - 1) * 8 : level + (size_t)sib * 8, other);
  const bool is_left = !(x & 1u);
  const fe h = poseidon_hash<poseidon_dev_field>(2, tab, [&](uint32_t j) {
    uint32_t w[8];
    const bool take_own = (j == 0) == is_left;
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = take_own ? own[k] : other[k];
    return imt_from_words(w);
  });
  uint32_t w[8];
  fe_to_ext<FrParams>(h, w);
  // left child: p - (own run's start) + (q - m) earlier sibling events, from the left run's start; right child: the mirror image
  const uint32_t place = p + q - m;
  if (place >= n_ev) return;                                                        // cannot happen over sorted distinct keys
  keys_out[place] = ((uint64_t)(x >> 1) << 32) | t;
  store_words(vals_out + (size_t)place * 8, w);
  uint32_t* proofs = (t & 1) ? out_new_proofs : out_low_proofs;
  if (proofs) store_words(proofs + ((size_t)(t >> 1) * depth + L) * 8, other);
}

// keys_prev / vals_prev: level depth - 1's events, settled into `below`; top: the top level's values, place = time, the last one the root
__global__ void __launch_bounds__(IMT_BLOCK) k_imt_finish(const uint64_t* __restrict__ keys_prev, const uint32_t* __restrict__ vals_prev, const uint32_t* __restrict__ pre,
                                                          uint32_t n_ev, uint32_t* __restrict__ below, uint32_t* __restrict__ preimages, const uint32_t* __restrict__ top,
                                                          uint32_t* __restrict__ root, uint32_t* __restrict__ out_roots) {
  const uint32_t p = blockIdx.x * IMT_BLOCK + threadIdx.x;
  if (p >= n_ev) return;
  imt_settle(keys_prev, vals_prev, p, n_ev, below, pre, preimages);
  if (p + 1 == n_ev) imt_copy(root, top + (size_t)p * 8, 1);
  if (out_roots && (p & 1)) imt_copy(out_roots + (size_t)((p >> 1) + 1) * 8, top + (size_t)p * 8, 1);
}

int imt_fill_device(uint32_t* d_dst, size_t n, const uint32_t value[8], hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  const uint4 lo = make_uint4(value[0], value[1], value[2], value[3]), hi = make_uint4(value[4], value[5], value[6], value[7]);
  hipLaunchKernelGGL(k_imt_fill, dim3((unsigned)((n + IMT_BLOCK - 1) / IMT_BLOCK)), dim3(IMT_BLOCK), 0, stream, d_dst, n, lo, hi);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

size_t imt_workspace_bytes(size_t n_new) { return 2 * n_new * (size_t)IMT_WS_EVENT_BYTES; }

// ws: imt_workspace_bytes(n_new) bytes whose first 2 n_new x 8 bytes hold the level-0 keys and whose next 2 n_new x 96 the preimages by time.
// d_leaves, d_nodes, d_preimages: the tree, updated.  The out_* pointers are all null or all set.
int imt_insert_device(uint32_t depth, size_t n_new, void* ws, uint32_t* d_leaves, uint32_t* d_nodes, uint32_t* d_preimages, uint32_t* out_roots,
                      uint32_t* out_new_leaves, uint32_t* out_low_proofs, uint32_t* out_new_proofs, const uint32_t* d_tab, hipStream_t stream) {
  const uint32_t n_ev = (uint32_t)(2 * n_new);
  const size_t n = (size_t)1 << depth;
  char* base = (char*)ws;
  uint64_t* keys[3];
  uint32_t* vals[3];
  const uint32_t* pre = (const uint32_t*)(base + (size_t)n_ev * 8);
  keys[0] = (uint64_t*)base;
  char* at = base + (size_t)n_ev * (8 + 96);
  for (int i = 0; i < 3; i++) {
    if (i) { keys[i] = (uint64_t*)at; at += (size_t)n_ev * 8; }
    vals[i] = (uint32_t*)at;
    at += (size_t)n_ev * 32;
  }
  const dim3 grid((n_ev + IMT_BLOCK - 1) / IMT_BLOCK), block(IMT_BLOCK);
  const fe* tab = (const fe*)d_tab;
  if (out_roots) HIPCHK(hipMemcpyAsync(out_roots, d_nodes + (n - 2) * 8, 32, hipMemcpyDeviceToDevice, stream));   // the root before the batch
  hipLaunchKernelGGL(k_imt_leaves, grid, block, 0, stream, keys[0], pre, n_ev, vals[0], out_new_leaves, tab);
  HIPCHK(hipGetLastError());
  // level L's events live in set L % 3: the launch of level L reads set L, writes set L + 1 and settles set L - 1
  auto cells = [&](uint32_t L) { return L == 0 ? d_leaves : d_nodes + (n - (n >> (L - 1))) * 8; };
  for (uint32_t L = 0; L < depth; L++) {
    const int in = L % 3, out = (L + 1) % 3, prev = (L + 2) % 3;
    hipLaunchKernelGGL(k_imt_level, grid, block, 0, stream, keys[in], vals[in], n_ev, cells(L), keys[out], vals[out], L ? keys[prev] : (const uint64_t*)nullptr,
                       L ? vals[prev] : (const uint32_t*)nullptr, L ? cells(L - 1) : (uint32_t*)nullptr, pre, d_preimages, out_low_proofs, out_new_proofs, depth, L, tab);
    HIPCHK(hipGetLastError());
  }
  const int last = (depth - 1) % 3, top = depth % 3;
  hipLaunchKernelGGL(k_imt_finish, grid, block, 0, stream, keys[last], vals[last], pre, n_ev, cells(depth - 1), depth == 1 ? d_preimages : (uint32_t*)nullptr, vals[top],
                     cells(depth), out_roots);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

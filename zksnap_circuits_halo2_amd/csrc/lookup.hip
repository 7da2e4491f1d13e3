// The lookup argument's `permute_expression_pair` ([DEP] halo2-axiom halo2_proofs/src/plonk/lookup/prover.rs, reached from
// create_proof, /root/reference/aggregator/src/wrapper.rs:129).  Given the compressed input
// column A and table column S over the usable rows, the reference
//   * sorts A (by the canonical integer value of each element: `Ord for Fr` compares `to_repr()`)            -> A'
//   * at the first row of every run of equal values in A' puts that value into S' and takes one instance of it out of a
//     BTreeMap (value -> count) of the table (an input value missing from the table is an error),
//   * hands the map's leftover entries, in ascending order, to the remaining rows taken from the *end* (Vec::pop).
// Restated for a GPU as sorts, a binary search and two scans:
//   keys      canonical integers of A and S (one Montgomery multiply each)
//   sort      both key arrays (rocPRIM: radix sort of the low limbs when every key fits 64 bits -- range checks --, else a merge sort
//             with a 256-bit comparison; plain library sorts, not hot kernels)
//   mark      first-of-run rows of A'; each looks up its value in the sorted table (lower bound) and marks that instance used
//   scan      rank of every repeated row among the repeated rows; rank of every unused table instance among the unused ones
//   assign    S'[first row] = A'[row];  S'[repeated row of rank r] = unused instance of rank R - 1 - r   (R = number of repeated rows)
// Rows >= usable_rows (the blinding rows) are left to the caller.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <cstdint>
#include <vector>
#include "check_report.hpp"
#include "fp29.hpp"
#include "fr_vec.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

struct key256 {   // canonical integer, little-endian 64-bit limbs
  uint64_t w[4];
};

struct key256_less {
  __host__ __device__ bool operator()(const key256& a, const key256& b) const {
    if (a.w[3] != b.w[3]) return a.w[3] < b.w[3];
    if (a.w[2] != b.w[2]) return a.w[2] < b.w[2];
    if (a.w[1] != b.w[1]) return a.w[1] < b.w[1];
    return a.w[0] < b.w[0];
  }
};

__device__ __forceinline__ bool key_eq(const key256& a, const key256& b) {
  return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3];
}

// Montgomery words x*2^256 -> the integer x (one multiply by 2^5 in the radix-2^261 domain).  *wide is set when a key does not fit 64
// bits: range-check lookups (the common case: values below 2^lookup_bits) then sort 8-byte keys with a radix sort instead.
__device__ __forceinline__ key256 canonical_key(const uint32_t* __restrict__ in, size_t i) {
  fe c;
#pragma unroll
  for (int k = 0; k < NL; k++) c.l[k] = Fr::FROM_EXT_CANON[k];
  uint32_t w[8];
  fe_pack(fe_canon_lt2p<Fr>(fe_mul<Fr>(load_ext(in, i), c)), w);
  key256 out;
#pragma unroll
  for (int k = 0; k < 4; k++) out.w[k] = (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
  return out;
}

__global__ void __launch_bounds__(256) k_lookup_keys(const uint32_t* __restrict__ in, size_t n, key256* __restrict__ keys, uint64_t* __restrict__ low,
                                                     uint32_t* __restrict__ wide) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const key256 out = canonical_key(in, i);
  keys[i] = out;
  low[i] = out.w[0];
  if (out.w[1] | out.w[2] | out.w[3]) atomicOr(wide, 1u);
}

__global__ void __launch_bounds__(256) k_lookup_widen(const uint64_t* __restrict__ low, size_t n, key256* __restrict__ keys) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key256 out;
  out.w[0] = low[i]; out.w[1] = 0; out.w[2] = 0; out.w[3] = 0;
  keys[i] = out;
}

// first-of-run flags of the sorted input; every first row claims the first instance of its value in the sorted table
__global__ void __launch_bounds__(256) k_lookup_mark(const key256* __restrict__ a, const key256* __restrict__ t, uint32_t n,
                                                     uint32_t* __restrict__ repeated, uint32_t* __restrict__ unused, uint32_t* __restrict__ error) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const key256 v = a[i];
  const bool first = i == 0 || !key_eq(v, a[i - 1]);
  repeated[i] = first ? 0u : 1u;
  if (!first) return;
  uint32_t lo = 0, hi = n;                     // lower bound of v in t
  const key256_less less;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (less(t[mid], v)) lo = mid + 1; else hi = mid;
  }
  if (lo < n && key_eq(t[lo], v)) unused[lo] = 0u;      // distinct values have distinct lower bounds: no two rows write one slot
  else atomicOr(error, 1u);
}

__global__ void __launch_bounds__(256) k_fill_u32(uint32_t* __restrict__ p, uint32_t n, uint32_t v) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// leftover[rank] = unused table instance, in ascending order
__global__ void __launch_bounds__(256) k_lookup_compact(const key256* __restrict__ t, const uint32_t* __restrict__ unused,
                                                        const uint32_t* __restrict__ unused_rank, uint32_t n, key256* __restrict__ leftover) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n && unused[j]) leftover[unused_rank[j]] = t[j];
}

__device__ __forceinline__ void store_key_as_fr(const key256& k, uint32_t* out, size_t i) {   // integer x -> Montgomery words x*2^256
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 4; j++) { w[2 * j] = (uint32_t)k.w[j]; w[2 * j + 1] = (uint32_t)(k.w[j] >> 32); }
  fe r2;
#pragma unroll
  for (int j = 0; j < NL; j++) r2.l[j] = Fr::R2[j];
  const fe internal = fe_mul<Fr>(fe_unpack<0>(w), r2);       // x * 2^261
  uint32_t o[8];
  fe_to_ext<Fr>(internal, o);
  store_words(out + i * 8, o);
}

__global__ void __launch_bounds__(256) k_lookup_assign(const key256* __restrict__ a, const uint32_t* __restrict__ repeated,
                                                       const uint32_t* __restrict__ repeated_rank, const key256* __restrict__ leftover,
                                                       uint32_t n, uint32_t n_repeated, uint32_t* __restrict__ out_input,
                                                       uint32_t* __restrict__ out_table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const key256 v = a[i];
  store_key_as_fr(v, out_input, i);
  // Vec::pop hands the ascending leftovers to the repeated rows from the last one backwards
  store_key_as_fr(repeated[i] ? leftover[n_repeated - 1 - repeated_rank[i]] : v, out_table, i);
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t sort_temp_bytes(size_t u) {
  size_t bytes = 0;
  (void)rocprim::merge_sort(nullptr, bytes, (key256*)nullptr, (key256*)nullptr, u, key256_less{});
  return bytes;
}
static size_t radix_temp_bytes(size_t u) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_keys(nullptr, bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, u);
  return bytes;
}
static size_t scan_temp_bytes(size_t u) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, u, rocprim::plus<uint32_t>{});
  return bytes;
}

size_t lookup_permute_workspace_bytes(size_t u) {
  const size_t st = sort_temp_bytes(u), rt = radix_temp_bytes(u);
  return 5 * al256(u * sizeof(key256)) + 4 * al256(u * sizeof(uint64_t)) + 4 * al256((u + 1) * sizeof(uint32_t)) + al256(st > rt ? st : rt) +
         al256(scan_temp_bytes(u + 1)) + 512;
}

// d_input / d_table: n elements each; the first `u` rows are permuted into d_out_input / d_out_table (which may not alias the inputs)
int lookup_permute_device(const uint32_t* d_input, const uint32_t* d_table, size_t u, uint32_t* d_out_input, uint32_t* d_out_table,
                          void* ws, size_t ws_bytes, hipStream_t stream) {
  if (u == 0) return ZKHIP_OK;
  if (u >= (1ull << 31)) { set_error("lookup_permute: %zu rows is too many", u); return ZKHIP_EINVAL; }
  if (ws_bytes < lookup_permute_workspace_bytes(u)) { set_error("lookup_permute: workspace too small"); return ZKHIP_EINVAL; }
  char* p = (char*)ws;
  auto carve = [&](size_t bytes) { void* r = p; p += al256(bytes); return r; };
  key256* ka = (key256*)carve(u * sizeof(key256));
  key256* ks = (key256*)carve(u * sizeof(key256));
  key256* sa = (key256*)carve(u * sizeof(key256));
  key256* st = (key256*)carve(u * sizeof(key256));
  key256* leftover = (key256*)carve(u * sizeof(key256));
  uint32_t* repeated = (uint32_t*)carve((u + 1) * 4);
  uint32_t* unused = (uint32_t*)carve((u + 1) * 4);
  uint32_t* repeated_rank = (uint32_t*)carve((u + 1) * 4);
  uint32_t* unused_rank = (uint32_t*)carve((u + 1) * 4);
  uint64_t* la = (uint64_t*)carve(u * sizeof(uint64_t));
  uint64_t* ls = (uint64_t*)carve(u * sizeof(uint64_t));
  uint64_t* la_sorted = (uint64_t*)carve(u * sizeof(uint64_t));
  uint64_t* ls_sorted = (uint64_t*)carve(u * sizeof(uint64_t));
  size_t sort_bytes = sort_temp_bytes(u), radix_bytes = radix_temp_bytes(u), scan_bytes = scan_temp_bytes(u + 1);
  void* sort_tmp = carve(sort_bytes > radix_bytes ? sort_bytes : radix_bytes);
  void* scan_tmp = carve(scan_bytes);
  uint32_t* flags = (uint32_t*)carve(512);         // [0] error, [1] some key wider than 64 bits
  const uint32_t n = (uint32_t)u;
  const dim3 grid((unsigned)((u + 255) / 256)), grid1((unsigned)((u + 256) / 256)), block(256);
  HIPCHK(hipMemsetAsync(flags, 0, 512, stream));
  hipLaunchKernelGGL(k_lookup_keys, grid, block, 0, stream, d_input, u, ka, la, flags + 1);
  hipLaunchKernelGGL(k_lookup_keys, grid, block, 0, stream, d_table, u, ks, ls, flags + 1);
  uint32_t wide = 1;
  HIPCHK(hipMemcpyAsync(&wide, flags + 1, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (wide) {                                      // full-width values (theta-compressed multi-column lookups): 256-bit comparison sort
    HIPCHK(rocprim::merge_sort(sort_tmp, sort_bytes, ka, sa, u, key256_less{}, stream));
    HIPCHK(rocprim::merge_sort(sort_tmp, sort_bytes, ks, st, u, key256_less{}, stream));
  } else {                                         // every key fits 64 bits: radix sort of the low limbs
    HIPCHK(rocprim::radix_sort_keys(sort_tmp, radix_bytes, la, la_sorted, u, 0, 64, stream));
    HIPCHK(rocprim::radix_sort_keys(sort_tmp, radix_bytes, ls, ls_sorted, u, 0, 64, stream));
    hipLaunchKernelGGL(k_lookup_widen, grid, block, 0, stream, (const uint64_t*)la_sorted, u, sa);
    hipLaunchKernelGGL(k_lookup_widen, grid, block, 0, stream, (const uint64_t*)ls_sorted, u, st);
  }
  hipLaunchKernelGGL(k_fill_u32, grid1, block, 0, stream, unused, n + 1, 1u);
  HIPCHK(hipMemsetAsync(repeated + u, 0, 4, stream));
  hipLaunchKernelGGL(k_lookup_mark, grid, block, 0, stream, (const key256*)sa, (const key256*)st, n, repeated, unused, flags);
  // exclusive scans over u + 1 entries: the last entry of each is the total
  HIPCHK(rocprim::exclusive_scan(scan_tmp, scan_bytes, repeated, repeated_rank, 0u, u + 1, rocprim::plus<uint32_t>{}, stream));
  HIPCHK(rocprim::exclusive_scan(scan_tmp, scan_bytes, unused, unused_rank, 0u, u + 1, rocprim::plus<uint32_t>{}, stream));
  uint32_t host[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(&host[0], flags, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&host[1], repeated_rank + u, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&host[2], unused_rank + u, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  // `unused` had its sentinel entry u set to 1 by the fill: the scan total at u does not include it
  if (host[0] != 0 || host[1] != host[2]) {
    set_error("lookup_permute: an input value is missing from the table (the reference returns Error::ConstraintSystemFailure)");
    return ZKHIP_EINVAL;
  }
  hipLaunchKernelGGL(k_lookup_compact, grid, block, 0, stream, (const key256*)st, (const uint32_t*)unused, (const uint32_t*)unused_rank, n, leftover);
  hipLaunchKernelGGL(k_lookup_assign, grid, block, 0, stream, (const key256*)sa, (const uint32_t*)repeated, (const uint32_t*)repeated_rank,
                     (const key256*)leftover, n, host[1], d_out_input, d_out_table);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}


// ---- every lookup of a circuit in one call ------------------------------------------------------------------------------------------------
// An input value that is not in the table is an error, so the sorted input column is a function of the sorted table and a histogram: with
// t[0..u) the table's keys in ascending order, j = lower_bound(t, key) of every input row (t[j] != key: the lookup fails) and cnt[j] the
// number of rows that landed on slot j (only the first instance of a value ever receives a count),
//   A'   = t[j] repeated cnt[j] times, j ascending: row i belongs to the slot j with start[j] <= i < start[j + 1], start = exclusive scan of cnt
//   S'   = t[j] at the first row of run j; the repeated row of rank r (in row order) takes the unused instance (cnt == 0) of rank R - 1 - r
// which is k_lookup_mark / k_lookup_compact / k_lookup_assign with the input sort replaced by the histogram.  The rank of a repeated row needs no
// scan of its own: sum_{j' < j} max(cnt - 1, 0) = start[j] - (j - unused_rank[j]), and R = unused_rank[u] once every row has been counted.  The
// two scans that remain share one 64-bit word per slot (low half start, high half unused_rank).  No input column is sorted, a table is sorted
// once per distinct address, 64-bit and full-width keys take one path, and every kernel has the lookup as blockIdx.y: the launches of a call
// are  table keys, one library sort per distinct table, histogram, 2 * scan levels - 1 scan kernels, expand  -- whatever the number of lookups,
// with one host wait, for the status word.
constexpr uint32_t LOOKUP_OK = 0xFFFFFFFFu;
constexpr uint32_t SCAN_PER_THREAD = 8, SCAN_TILE = 256 * SCAN_PER_THREAD;       // slots of one workgroup of the scans

__global__ void __launch_bounds__(256) k_lookup_table_keys(const uint64_t* __restrict__ args, uint32_t n_lookups, uint32_t u, key256* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= u) return;
  const uint32_t* table = (const uint32_t*)args[n_lookups + blockIdx.y];
  keys[(size_t)blockIdx.y * u + i] = canonical_key(table, i);
}

// the key search the histogram and the membership check share: the lower bound of v among the u ascending keys t; true when v is there
__device__ __forceinline__ bool lookup_find(const key256* __restrict__ t, uint32_t u, const key256& v, uint32_t* slot) {
  uint32_t lo = 0, hi = u;
  const key256_less less;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (less(t[mid], v)) lo = mid + 1; else hi = mid;
  }
  *slot = lo;
  return lo < u && key_eq(t[lo], v);
}

// One thread per (lookup, input row): the row's key in registers, its lower bound in the lookup's sorted table, one count.  Padding rows make
// real columns skewed (one slot can take most of a column) and the compiler folds atomicAdd(p, 1) into one add per wavefront only for a uniform
// p: the lanes that share the slot of the first pending lane are counted with one atomic, four rounds at the most (the heavy slots), and what
// is still pending then adds for itself.  Integer counts: the result does not depend on the order of arrival.  The counters are in global memory
// over a full grid: one workgroup per lookup with the counters in LDS keeps only L CUs busy and was 1.6 x / 2.8 x slower per call at (k, L) =
// (13, 8) / (15, 11) (profiles/r09_lookup_arguments.txt).
__global__ void __launch_bounds__(256) k_lookup_hist(const uint64_t* __restrict__ args, uint32_t n_lookups, uint32_t n_tables, uint32_t u,
                                                     const key256* __restrict__ sorted, uint32_t* __restrict__ cnt, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  const key256* t = sorted + (size_t)(uint32_t)args[n_lookups + n_tables + l] * u;
  bool pending = false;
  uint32_t slot = 0;
  if (i < u) {
    const key256 v = canonical_key((const uint32_t*)args[l], i);
    if (lookup_find(t, u, v, &slot)) pending = true;
    else atomicMin(status, l);                                       // the lowest failing lookup
  }
  uint32_t* c = cnt + (size_t)l * (u + 1);
  const uint32_t lane = threadIdx.x & 63u;
  for (int round = 0; round < 4; round++) {
    const unsigned long long active = __ballot(pending);
    if (!active) break;
    const uint32_t leader = (uint32_t)__ffsll(active) - 1u;
    const uint32_t lslot = __shfl(slot, (int)leader);
    const bool same = pending && slot == lslot;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(c + lslot, (uint32_t)__popcll(m));
    if (same) pending = false;
  }
  if (pending) atomicAdd(c + slot, 1u);
}

// Membership only (zkhip_check_lookups_device): one thread per (lookup, input row), the same search, no counters -- the rows whose value the
// table does not hold go to the lookup's report record, item index = row
__global__ void __launch_bounds__(256) k_lookup_member(const uint64_t* __restrict__ args, uint32_t n_lookups, uint32_t n_tables, uint32_t u,
                                                       const key256* __restrict__ sorted, unsigned long long* __restrict__ reports) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  const key256* t = sorted + (size_t)(uint32_t)args[n_lookups + n_tables + l] * u;
  bool failing = false;
  if (i < u) {
    uint32_t slot;
    failing = !lookup_find(t, u, canonical_key((const uint32_t*)args[l], i), &slot);
  }
  check_report_wave(failing, i, reports + 2 * (size_t)l);
}

// exclusive scan of 256 values, one per thread of the workgroup; *total: their sum
__device__ __forceinline__ unsigned long long block_exclusive_scan(unsigned long long v, unsigned long long* total) {
  __shared__ unsigned long long wave_sum[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(incl, d);
    if (lane >= (uint32_t)d) incl += o;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  unsigned long long off = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; w++) { if (w < wave) off += wave_sum[w]; all += wave_sum[w]; }
  *total = all;
  return off + incl - v;
}

// One level of the scans, blockIdx.y = lookup: a workgroup scans SCAN_TILE entries from 0 and hands their sum up.  Level 0 (cnt != nullptr) reads
// the counters: slot j < u is worth cnt[j] + 2^32 [cnt[j] == 0], entry u closes the array; the higher levels scan the sums below them in place.
__global__ void __launch_bounds__(256) k_lookup_scan(const uint32_t* __restrict__ cnt, uint32_t u, unsigned long long* __restrict__ data, uint32_t count,
                                                     unsigned long long* __restrict__ sums, uint32_t n_sums) {
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD, l = blockIdx.y;
  unsigned long long* d = data + (size_t)l * count;
  unsigned long long v[SCAN_PER_THREAD], mine = 0;
#pragma unroll
  for (uint32_t e = 0; e < SCAN_PER_THREAD; e++) {
    const uint32_t j = base + e;
    v[e] = 0;
    if (cnt) {
      if (j < u) { const uint32_t c = cnt[(size_t)l * count + j]; v[e] = c ? (unsigned long long)c : 1ull << 32; }
    } else if (j < count) v[e] = d[j];
    mine += v[e];
  }
  unsigned long long total;
  unsigned long long run = block_exclusive_scan(mine, &total);
#pragma unroll
  for (uint32_t e = 0; e < SCAN_PER_THREAD; e++) {
    const uint32_t j = base + e;
    if (j < count) d[j] = run;
    run += v[e];
  }
  if (sums && threadIdx.x == 0) sums[(size_t)l * n_sums + blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_lookup_scan_add(unsigned long long* __restrict__ data, uint32_t count, const unsigned long long* __restrict__ sums,
                                                         uint32_t n_sums) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (j < count && j >= SCAN_TILE) data[(size_t)l * count + j] += sums[(size_t)l * n_sums + j / SCAN_TILE];
}

// One thread per (lookup, output row).  R is read here, from the scan's last entry, not handed in by the host.
__global__ void __launch_bounds__(256) k_lookup_expand(const uint64_t* __restrict__ args, uint32_t n_lookups, uint32_t n_tables, uint32_t u, size_t n,
                                                       const key256* __restrict__ sorted, const unsigned long long* __restrict__ scan,
                                                       const uint32_t* __restrict__ status, uint32_t* __restrict__ out_input, uint32_t* __restrict__ out_table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (i >= u || *status != LOOKUP_OK) return;          // a failed call: not every row was counted, the searches below would not be bounded
  const key256* t = sorted + (size_t)(uint32_t)args[n_lookups + n_tables + l] * u;
  const unsigned long long* s = scan + (size_t)l * (u + 1);
  uint32_t lo = 0, hi = u;                             // the first entry whose start is above i (start[u] = u is): the run is the slot before it
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint32_t)s[mid] <= i) lo = mid + 1; else hi = mid;
  }
  const uint32_t j = lo - 1;
  const unsigned long long sj = s[j];
  const uint32_t start = (uint32_t)sj;
  const key256 v = t[j];
  uint32_t* oa = out_input + (size_t)l * n * 8;
  uint32_t* os = out_table + (size_t)l * n * 8;
  store_key_as_fr(v, oa, i);
  if (i == start) { store_key_as_fr(v, os, i); return; }
  const uint32_t total_unused = (uint32_t)(s[u] >> 32);                        // = R: as many repeated rows as unused instances
  const uint32_t r = start - (j - (uint32_t)(sj >> 32)) + (i - start - 1);     // repeated rows of the earlier runs + those of this run before row i
  const uint32_t want = total_unused - 1 - r;                                  // Vec::pop: the ascending leftovers are handed out from the last one
  lo = 0; hi = u;                                      // the first entry with more than `want` unused slots before it: the slot before it is unused
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint32_t)(s[mid] >> 32) <= want) lo = mid + 1; else hi = mid;
  }
  store_key_as_fr(t[lo - 1], os, i);
}

static uint32_t scan_levels(size_t count, size_t* counts) {                     // counts[k]: entries of level k; the last level is one tile
  uint32_t levels = 0;
  counts[levels++] = count;
  while (counts[levels - 1] > SCAN_TILE) { counts[levels] = (counts[levels - 1] + SCAN_TILE - 1) / SCAN_TILE; levels++; }
  return levels;
}

size_t lookup_permute_many_workspace_bytes(uint32_t n_lookups, size_t u) {
  const size_t L = n_lookups;
  size_t counts[8], sums = 0;
  const uint32_t levels = scan_levels(u + 1, counts);
  for (uint32_t k = 1; k < levels; k++) sums += al256(L * counts[k] * 8);
  return al256(3 * L * 8) + 2 * al256(L * u * sizeof(key256)) + al256(sort_temp_bytes(u)) + al256(L * (u + 1) * 4) + al256(L * (u + 1) * 8) + sums + 256;
}

// the argument block of a many-lookup call: [inputs L][distinct tables T][table index of every lookup L]; equal table addresses are one table
static std::vector<uint64_t> lookup_args(const void* const* d_inputs_host, const void* const* d_tables_host, uint32_t L) {
  std::vector<uint64_t> tables, index(L);
  for (uint32_t l = 0; l < L; l++) {
    const uint64_t addr = (uint64_t)(uintptr_t)d_tables_host[l];
    size_t t = 0;
    while (t < tables.size() && tables[t] != addr) t++;
    if (t == tables.size()) tables.push_back(addr);
    index[l] = t;
  }
  std::vector<uint64_t> host;
  for (uint32_t l = 0; l < L; l++) host.push_back((uint64_t)(uintptr_t)d_inputs_host[l]);
  host.insert(host.end(), tables.begin(), tables.end());
  host.insert(host.end(), index.begin(), index.end());
  return host;
}

// the block uploaded to `args`, then the keys of every distinct table and their ascending order (sorted[t * u ..]): what both many-lookup calls start with
static int lookup_sort_tables(const std::vector<uint64_t>& host, uint32_t L, uint32_t T, size_t u, uint64_t* args, key256* keys, key256* sorted, void* sort_tmp,
                              size_t sort_bytes, hipStream_t stream, arg_ring* ring) {
  int rc = upload_args(ring, args, host.data(), host.size() * 8, stream);
  if (rc != ZKHIP_OK) return rc;
  hipLaunchKernelGGL(k_lookup_table_keys, dim3((unsigned)((u + 255) / 256), T), dim3(256), 0, stream, (const uint64_t*)args, L, (uint32_t)u, keys);
  for (uint32_t t = 0; t < T; t++)                                      // a library sort, once per distinct table: 256-bit comparison, no dispatch on the width
    HIPCHK(rocprim::merge_sort(sort_tmp, sort_bytes, keys + (size_t)t * u, sorted + (size_t)t * u, u, key256_less{}, stream));
  return ZKHIP_OK;
}

// d_inputs_host / d_tables_host: n_lookups device addresses each, in host memory.  out_input / out_table: [n_lookups][n] dense.
int lookup_permute_many_device(const void* const* d_inputs_host, const void* const* d_tables_host, uint32_t n_lookups, size_t n, size_t u,
                               uint32_t* d_out_input, uint32_t* d_out_table, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring) {
  if (n_lookups == 0 || u == 0) return ZKHIP_OK;
  if (n_lookups > 65535) { set_error("lookup_permute_many: more than 65535 lookups"); return ZKHIP_EINVAL; }
  if (ws_bytes < lookup_permute_many_workspace_bytes(n_lookups, u)) { set_error("lookup_permute_many: workspace too small"); return ZKHIP_EINVAL; }
  const uint32_t L = n_lookups, un = (uint32_t)u;
  const std::vector<uint64_t> host = lookup_args(d_inputs_host, d_tables_host, L);
  const uint32_t T = (uint32_t)host.size() - 2 * L;
  char* p = (char*)ws;
  auto carve = [&](size_t bytes) { void* r = p; p += al256(bytes); return r; };
  uint64_t* args = (uint64_t*)carve(3 * (size_t)L * 8);
  key256* keys = (key256*)carve((size_t)L * u * sizeof(key256));
  key256* sorted = (key256*)carve((size_t)L * u * sizeof(key256));
  size_t sort_bytes = sort_temp_bytes(u);
  void* sort_tmp = carve(sort_bytes);
  uint32_t* cnt = (uint32_t*)carve((size_t)L * (u + 1) * 4);
  size_t counts[8];
  const uint32_t levels = scan_levels(u + 1, counts);
  unsigned long long* level[8];
  level[0] = (unsigned long long*)carve((size_t)L * (u + 1) * 8);
  for (uint32_t k = 1; k < levels; k++) level[k] = (unsigned long long*)carve((size_t)L * counts[k] * 8);
  uint32_t* status = (uint32_t*)carve(256);
  HIPCHK(hipMemsetAsync(status, 0xFF, 4, stream));
  HIPCHK(hipMemsetAsync(cnt, 0, (size_t)L * (u + 1) * 4, stream));
  const dim3 block(256), rows((unsigned)((u + 255) / 256), L);
  int rc = lookup_sort_tables(host, L, T, u, args, keys, sorted, sort_tmp, sort_bytes, stream, ring);
  if (rc != ZKHIP_OK) return rc;
  hipLaunchKernelGGL(k_lookup_hist, rows, block, 0, stream, (const uint64_t*)args, L, T, un, (const key256*)sorted, cnt, status);
  for (uint32_t k = 0; k < levels; k++) {                               // up: tiles of every level, their sums are the level above
    const uint32_t tiles = (uint32_t)((counts[k] + SCAN_TILE - 1) / SCAN_TILE);
    hipLaunchKernelGGL(k_lookup_scan, dim3(tiles, L), block, 0, stream, k == 0 ? (const uint32_t*)cnt : (const uint32_t*)nullptr, un, level[k], (uint32_t)counts[k],
                       k + 1 < levels ? level[k + 1] : (unsigned long long*)nullptr, k + 1 < levels ? (uint32_t)counts[k + 1] : 0u);
  }
  for (uint32_t k = levels - 1; k-- > 0;)                               // down: every tile takes the scanned sum of the tiles before it
    hipLaunchKernelGGL(k_lookup_scan_add, dim3((unsigned)((counts[k] + 255) / 256), L), block, 0, stream, level[k], (uint32_t)counts[k],
                       (const unsigned long long*)level[k + 1], (uint32_t)counts[k + 1]);
  hipLaunchKernelGGL(k_lookup_expand, rows, block, 0, stream, (const uint64_t*)args, L, T, un, n, (const key256*)sorted, (const unsigned long long*)level[0],
                     (const uint32_t*)status, d_out_input, d_out_table);
  HIPCHK(hipGetLastError());
  uint32_t failed = LOOKUP_OK;
  HIPCHK(hipMemcpyAsync(&failed, status, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (failed != LOOKUP_OK) {
    set_error("lookup_permute_many: lookup %u: an input value is missing from the table (the reference returns Error::ConstraintSystemFailure)", failed);
    return ZKHIP_EINVAL;
  }
  return ZKHIP_OK;
}

// ---- lookup membership: the witness check -------------------------------------------------------------------------------------------------
size_t lookup_check_workspace_bytes(uint32_t n_lookups, size_t u) {
  const size_t L = n_lookups;
  return al256(3 * L * 8) + 2 * al256(L * u * sizeof(key256)) + al256(sort_temp_bytes(u)) + 256;
}

// Nothing here waits for the stream: the argument block goes through the ring, the sort is enqueued, the verdicts stay in d_reports.
int lookup_check_device(const void* const* d_inputs_host, const void* const* d_tables_host, uint32_t n_lookups, size_t u, void* d_reports, void* ws, size_t ws_bytes,
                        hipStream_t stream, arg_ring* ring) {
  if (n_lookups == 0) return ZKHIP_OK;
  if (u >= (1ull << 31)) { set_error("check_lookups: %zu rows is too many", u); return ZKHIP_EINVAL; }
  if (u && ws_bytes < lookup_check_workspace_bytes(n_lookups, u)) { set_error("check_lookups: workspace too small"); return ZKHIP_EINVAL; }
  int rc = check_reports_init_device(d_reports, n_lookups, stream);
  if (rc != ZKHIP_OK || u == 0) return rc;
  const uint32_t L = n_lookups;
  const std::vector<uint64_t> host = lookup_args(d_inputs_host, d_tables_host, L);
  const uint32_t T = (uint32_t)host.size() - 2 * L;
  char* p = (char*)ws;
  auto carve = [&](size_t bytes) { void* r = p; p += al256(bytes); return r; };
  uint64_t* args = (uint64_t*)carve(3 * (size_t)L * 8);
  key256* keys = (key256*)carve((size_t)L * u * sizeof(key256));
  key256* sorted = (key256*)carve((size_t)L * u * sizeof(key256));
  const size_t sort_bytes = sort_temp_bytes(u);
  void* sort_tmp = carve(sort_bytes);
  if ((rc = lookup_sort_tables(host, L, T, u, args, keys, sorted, sort_tmp, sort_bytes, stream, ring)) != ZKHIP_OK) return rc;
  hipLaunchKernelGGL(k_lookup_member, dim3((unsigned)((u + 255) / 256), L), dim3(256), 0, stream, (const uint64_t*)args, L, T, (uint32_t)u, (const key256*)sorted,
                     (unsigned long long*)d_reports);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

// The level plan of the chunked scans (poly.hip, paillier.hip) and the workspace sizes built on it.  Host-only C++17: it compiles without HIP.
//
// Every scan is a linear recurrence cut into chunks of SCAN_CH elements, one lane per chunk: a pass reduces each chunk to one aggregate, the
// aggregates are a scan of 1 / SCAN_CH the length, a last pass re-runs each chunk from its carry.  Level 0 is the caller's array of n[0]
// elements; level k holds the n[k] = scan_chunks(n[k - 1]) aggregates of level k - 1, one row of row_bytes per element (a row = the lanes of a
// call side by side: the batch, the roots, the columns), at byte off[k] of the workspace.  Level k is stored while level k - 1 has more than
// SCAN_CH elements, so the last stored level is one chunk.  Every driver is the same two loops over one plan:
//   up    k = 1 .. L:   reduce level k - 1 into level k            (an evaluation adds k = L + 1: n[L + 1] = 1 aggregate, the result)
//   down  k = L .. 0:   scan level k from the carries in level k + 1 (none for k = L), n[k + 1] chunks
// and every *_workspace_bytes below is the `bytes` of the driver's own plan plus what rides with the levels.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/zkhip.h"

namespace zkhip {

constexpr uint32_t SCAN_CH = 16;
constexpr int SCAN_MAX_LEVELS = 16;           // 16^16 = 2^64 elements
inline size_t scan_chunks(size_t n) { return (n + SCAN_CH - 1) / SCAN_CH; }
inline size_t scan_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

struct scan_plan {
  int L = 0;                                  // stored levels: 1 .. L
  size_t n[SCAN_MAX_LEVELS + 2];              // n[0 .. L + 1]: the elements of level k = the chunks of level k - 1
  size_t off[SCAN_MAX_LEVELS + 1] = {};       // off[1 .. L], multiples of 256
  size_t bytes = 0;                           // all levels
  scan_plan(size_t n0, size_t row_bytes) {
    n[0] = n0;
    while (n[L] > SCAN_CH) {
      L++;
      n[L] = scan_chunks(n[L - 1]);
      off[L] = bytes;
      bytes += scan_align(n[L] * row_bytes);
    }
    n[L + 1] = scan_chunks(n[L]);
  }
  template <class T>
  T* level(void* ws, int k) const { return (T*)((char*)ws + off[k]); }
};

// poly.hip.  Scans of Fr elements (32 bytes).  eval_polynomial, kate_division and prefix_product scan one array and park their multiplier in
// the last 256 bytes (stage_const); batch_invert keeps n x 36 bytes of prefix products
inline size_t poly_workspace_bytes(size_t n) { return scan_plan(n, 32).bytes + 256 + scan_align(n * 36); }
// [pointer table][256: the multipliers][levels of `count` lanes]
inline size_t poly_batch_workspace_bytes(size_t n, size_t count) { return scan_align(count * 8) + 256 + scan_plan(n, 32 * count).bytes; }
inline size_t poly_roots_workspace_bytes(size_t n, uint32_t m) {          // levels of m lanes
  const size_t total = 256 + scan_plan(n, 32 * (size_t)m).bytes, single = poly_workspace_bytes(n);   // m = 1 without evaluations runs kate_division
  return total > single ? total : single;
}
inline size_t perm_workspace_bytes(uint32_t nperm, uint32_t chunk, uint32_t log_n) {   // [tables][batch_invert, then prefix_product, of all sets as one array]
  const size_t n = (size_t)1 << log_n, nsets = chunk ? (nperm + chunk - 1) / chunk : 0;
  const uint32_t h = (log_n + 1) / 2;
  const size_t tables = scan_align((size_t)nperm * 16) + scan_align((size_t)nperm * 32) + (((size_t)1 << h) + (n >> h)) * 32 + 768;
  return tables + poly_workspace_bytes(nsets * n);
}
// [pointer table][batch_invert of all lookups as one array, then levels of n_lookups lanes]
inline size_t lookup_products_workspace_bytes(uint32_t n_lookups, uint32_t log_n) {
  const size_t n = (size_t)1 << log_n;
  return scan_align((size_t)n_lookups * 16) + 256 + scan_plan(n, 32 * (size_t)n_lookups).bytes + poly_workspace_bytes((size_t)n_lookups * n);
}
// paillier.hip.  Levels of n_cols lanes of one ciphertext each
inline size_t paillier_tally_workspace_bytes(size_t n_ballots, uint32_t n_cols) {
  return 256 + scan_plan(n_ballots, (size_t)n_cols * ZKHIP_PAILLIER_WORDS * 8).bytes;
}

}  // namespace zkhip

// Launch arithmetic of the row MSM (row_msm.hip; include/zkhip.h, "KZG accumulators"), host-only and free of HIP so that
// tests/cpp/kzg_limbs_host_check.cpp can compile it: how a row of n_cols columns is cut into chunks, how many launches that takes, the grids
// and the scratch the partial sums need.
//
// A workgroup is ONE wavefront: lane j of chunk c runs the ladder of column 64 c + j, and a tree in LDS adds the 64 lanes.  The call is a
// dependent chain per lane (~127 doublings + additions), so what matters is how many chains run side by side, not how full a workgroup is:
// one wavefront per workgroup lets the dispatcher spread a batch of narrow rows (33 columns at the wrapper's shape) over as many SIMDs as
// there are rows.  A row of at most 64 columns is done after the first launch; a wider one (954 columns at the voter's shape: 15 chunks)
// leaves one XYZZ partial sum per chunk, which a second launch adds per row (lane j takes chunks j, j + 64, ...).
#pragma once
#include <cstddef>
#include <cstdint>

namespace zkhip {

constexpr uint32_t ROW_MSM_LANES = 64;                    // columns per chunk = lanes per workgroup
constexpr uint32_t ROW_MSM_MAX_BLOCKS = 1u << 16;         // workgroups per launch; beyond that each takes several chunks (rows) in turn
constexpr uint64_t ROW_MSM_MAX_ELEMS = 1ull << 31;        // n_rows * n_cols
constexpr size_t ROW_MSM_XYZZ_BYTES = 144;                // a partial sum: 4 coordinates of 9 limbs

struct row_msm_plan {
  uint32_t chunks = 0;       // per row
  uint32_t stages = 0;       // launches: 0 (nothing to do), 1 or 2
  uint64_t units = 0;        // stage 1: n_rows * chunks (row, chunk) pairs
  uint32_t grid1 = 0;        // stage 1 workgroups
  uint32_t grid2 = 0;        // stage 2 workgroups (0 when stages < 2)
  size_t partial_bytes = 0;  // scratch between the stages
};

// valid = the shape is one the call accepts (n_cols >= 1, n_rows * n_cols <= 2^31)
inline bool row_msm_make_plan(uint64_t n_rows, uint64_t n_cols, row_msm_plan* p) {
  *p = row_msm_plan();
  if (n_cols == 0 || n_cols > ROW_MSM_MAX_ELEMS || n_rows > ROW_MSM_MAX_ELEMS || n_rows * n_cols > ROW_MSM_MAX_ELEMS) return false;
  if (n_rows == 0) return true;
  p->chunks = (uint32_t)((n_cols + ROW_MSM_LANES - 1) / ROW_MSM_LANES);
  p->stages = p->chunks == 1 ? 1 : 2;
  p->units = n_rows * p->chunks;
  p->grid1 = (uint32_t)(p->units < ROW_MSM_MAX_BLOCKS ? p->units : ROW_MSM_MAX_BLOCKS);
  if (p->stages == 2) {
    p->grid2 = (uint32_t)(n_rows < ROW_MSM_MAX_BLOCKS ? n_rows : ROW_MSM_MAX_BLOCKS);
    p->partial_bytes = (size_t)p->units * ROW_MSM_XYZZ_BYTES;
  }
  return true;
}

// [a, a + na) and [b, b + nb) share a byte (empty ranges share nothing)
inline bool row_msm_ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na && nb && x < y + nb && y < x + na;
}

// Everything the C call refuses, decided from the arguments alone (no HIP).  Returns nullptr when the call may go on, else what is wrong.
inline const char* row_msm_refusal(const void* d_rows, uint64_t n_cols, const void* d_own, uint64_t n_own, uint64_t own_stride, const void* d_shared, uint64_t n_rows,
                                   const void* d_out) {
  row_msm_plan p;
  if (n_cols == 0) return "n_cols = 0";
  if (n_own > n_cols) return "n_own > n_cols";
  if (own_stride < n_own) return "own_stride < n_own";
  if (!row_msm_make_plan(n_rows, n_cols, &p)) return "n_rows * n_cols above 2^31";
  if (n_rows == 0) return nullptr;
  if (own_stride > (1ull << 40) / (n_rows > 1 ? n_rows - 1 : 1)) return "own points spread over more than 2^40 elements";   // (keeps the byte counts below in 64 bits)
  const uint64_t n_shared = n_cols - n_own;
  auto bad = [](const void* q) { return q == nullptr || ((uintptr_t)q & 15) != 0; };
  if (bad(d_rows) || bad(d_out) || (n_own && bad(d_own)) || (n_shared && bad(d_shared))) return "null or misaligned pointer";
  const uint64_t out_bytes = n_rows * 96;
  const uint64_t own_bytes = n_own ? ((n_rows - 1) * own_stride + n_own) * 64 : 0;
  if (row_msm_ranges_overlap(d_out, out_bytes, d_rows, n_rows * n_cols * 32) || row_msm_ranges_overlap(d_out, out_bytes, d_own, own_bytes) ||
      row_msm_ranges_overlap(d_out, out_bytes, d_shared, n_shared * 64))
    return "the output overlaps an input";
  return nullptr;
}

}  // namespace zkhip

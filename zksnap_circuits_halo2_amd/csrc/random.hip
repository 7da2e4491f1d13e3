// Random Fr columns produced in HBM: the stream of fr_random.hpp, one lane per element (one ChaCha20 block of ten unrolled double rounds,
// one fe_mul_add, two 16-byte stores).  The seed words and the counters are kernel arguments, so nothing is read from memory but the
// rows form's table of column addresses.
#include "zkhip_internal.hpp"
#include "fr_random.hpp"

namespace zkhip {

constexpr int RANDOM_BLOCK = 256;
constexpr size_t RANDOM_LAUNCH_MAX = (size_t)1 << 30;   // elements of one launch (grid.x stays far below 2^31)

// d_out[t] = element first + t, t < n
__global__ __launch_bounds__(RANDOM_BLOCK) void k_fr_random(fr_random_key key, uint64_t stream_id, uint64_t first, uint64_t n, uint32_t* __restrict__ d_out) {
  const uint64_t t = (uint64_t)blockIdx.x * RANDOM_BLOCK + threadIdx.x;
  if (t >= n) return;
  uint32_t w[8];
  fr_random_element(key, stream_id, first + t, w);
  store_words(d_out + t * 8, w);
}

// row row0 + j of column c = element first + c * count + j, for t = c * count + j < total
__global__ __launch_bounds__(RANDOM_BLOCK) void k_fr_random_rows(fr_random_key key, uint64_t stream_id, uint64_t first, uint32_t* const* __restrict__ d_cols,
                                                                uint64_t total, uint64_t row0, uint64_t count) {
  const uint64_t t = (uint64_t)blockIdx.x * RANDOM_BLOCK + threadIdx.x;
  if (t >= total) return;
  const uint64_t c = t / count, j = t - c * count;
  uint32_t w[8];
  fr_random_element(key, stream_id, first + t, w);
  store_words(d_cols[c] + (row0 + j) * 8, w);
}

int fr_random_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, size_t n, uint32_t* d_out, hipStream_t stream) {
  const fr_random_key key = fr_random_key_from_seed(seed);
  for (size_t done = 0; done < n; done += RANDOM_LAUNCH_MAX) {
    const size_t m = n - done < RANDOM_LAUNCH_MAX ? n - done : RANDOM_LAUNCH_MAX;
    hipLaunchKernelGGL(k_fr_random, dim3((unsigned)((m + RANDOM_BLOCK - 1) / RANDOM_BLOCK)), dim3(RANDOM_BLOCK), 0, stream, key, stream_id, first + done, (uint64_t)m,
                       d_out + done * 8);
    HIPCHK(hipGetLastError());
  }
  return ZKHIP_OK;
}

size_t fr_random_rows_workspace_bytes(uint32_t n_cols) { return (size_t)n_cols * sizeof(void*); }

int fr_random_rows_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, const void* const* d_cols_host, uint32_t n_cols, size_t row0, size_t count,
                          void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring) {
  if (ws_bytes < fr_random_rows_workspace_bytes(n_cols)) { set_error("fr_random_rows: workspace too small"); return ZKHIP_EINVAL; }
  const uint64_t total = (uint64_t)n_cols * count;
  if (total > RANDOM_LAUNCH_MAX) { set_error("fr_random_rows: %llu elements in one call (at most 2^30)", (unsigned long long)total); return ZKHIP_EINVAL; }
  const fr_random_key key = fr_random_key_from_seed(seed);
  int rc = upload_args(ring, ws, d_cols_host, (size_t)n_cols * sizeof(void*), stream);
  if (rc != ZKHIP_OK) return rc;
  hipLaunchKernelGGL(k_fr_random_rows, dim3((unsigned)((total + RANDOM_BLOCK - 1) / RANDOM_BLOCK)), dim3(RANDOM_BLOCK), 0, stream, key, stream_id, first,
                     (uint32_t* const*)ws, total, (uint64_t)row0, (uint64_t)count);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

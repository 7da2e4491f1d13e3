// Internal declarations shared by the translation units of libzkhip.so (not installed).
#pragma once
#include <string>
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/zkhip.h"
#include "scan_plan.hpp"      // defines the *_workspace_bytes of the chunked scans declared below (inline, host-only)
#include "rowvm_blob.hpp"     // the row programs' blob: its plan and row_vm_workspace_bytes (inline, host-only)

namespace zkhip {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// four little-endian words below the modulus of Fr
static inline bool fr_words_canonical(const uint64_t w[4]) {
  constexpr uint64_t R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
  for (int i = 3; i >= 0; i--)
    if (w[i] != R[i]) return w[i] < R[i];
  return false;
}

// a failed HIP call ends the function it is in: its text and HIP's message become the thread's error, ZKHIP_EHIP the return value
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { ::zkhip::set_error("%s failed: %s", #x, hipGetErrorString(e_)); return ZKHIP_EHIP; } } while (0)

// profiler (capi.hip): when enabled, device paths drop named HIP events on their stream between phases
void prof_begin(hipStream_t stream);
void prof_mark(hipStream_t stream, const char* name);

// msm.hip
int g1_gen_walk_device(const uint32_t t0_ext[8], const uint32_t d_ext[8], size_t n, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
size_t g1_gen_walk_workspace(size_t n);
size_t g1_fixed_base_table_bytes();
size_t g1_fixed_base_workspace(size_t n);
int g1_fixed_base_table_build(uint32_t* d_table, void* ws, size_t ws_bytes, hipStream_t stream);
int g1_fixed_base_mul_device(const uint32_t* d_scalars, size_t n, const uint32_t* d_table, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
int msm_pick_window(size_t n);
size_t msm_workspace_bytes(size_t n, int c, bool prepared = false, size_t batch = 1, size_t xyzz_bytes = 144);
// one run of a bucket's sorted point references, handed to one accumulate lane (or lane group) of either curve
struct task_t {
  uint32_t bucket, start, len;
};
// what the curve-specific kernels (accumulate, combine, bucket reduction) need once the scalars are sorted into tasks
struct msm_tasks_view {
  int c, W, WB;                    // window bits, windows, bucket sets
  uint32_t B, NB, task_shift;      // buckets per set, buckets in all, log2 task length
  size_t max_tasks, nk;
  const task_t* tasks;
  uint32_t* ntasks;                // device: number of tasks
  uint32_t* max_parts;             // device: largest task count of one bucket
  const uint4* order;              // execution order records (task | 0x80000000 + bucket, start, len, first reference)
  const uint32_t* sorted;          // point references (bit 31 = negate), bucket by bucket
  const uint32_t* task_off;        // first task of every bucket (NB + 1)
  uint32_t *partials, *pyrA, *pyrB, *winsum;   // work arrays of xyzz_bytes-sized points
  int combine_lanes;               // G1 combine step: lanes per bucket, partials it sums per bucket, and the list of buckets with more
  uint32_t seq_parts;
  const uint32_t* heavy_count;
  const void* heavy;               // uint2 (bucket, slice) entries
  uint32_t heavy_cap;
  uint32_t* heavy_done;
  uint32_t* endo;                  // G1 general path with GLV digits: room for the endomorphism images of the n bases
};
// glv (general path of either curve): the scalars are split with the curve's endomorphism (msm.hip k_digits_glv): the sort sees 2 n points and
// ceil(128 / c) windows, point references >= n mean "the image of point ref - n"
int msm_glv_windows(int c);
int msm_build_tasks(const uint32_t* d_scalars, size_t n, size_t batch, size_t scalar_stride, int c, bool shared_buckets, uint32_t ref_base, uint32_t ref_stride,
                    size_t xyzz_bytes, void* ws, size_t ws_bytes, hipStream_t stream, msm_tasks_view* out, bool glv = false);
// msm_g2.hip
size_t msm_g2_workspace_bytes(size_t n);
int msm_g2_device(const uint32_t* d_scalars, const uint32_t* d_bases, size_t n, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
int test_g2_op(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, size_t n, hipStream_t stream);
int test_g2_formula_op(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, uint32_t* d_work, size_t n, hipStream_t stream);   // selftest.hip: ops 7 .. 11 and 256 + 5 .. 256 + 11
// pairing.hip: n <= ZKHIP_MAX_PAIRS; d_ok one uint32.  which: bit 0 the quad policy (d_out), bit 1 the single-lane policy (d_out + 96 words)
int pairing_check_device(const uint32_t* d_g1, const uint32_t* d_g2, size_t n, uint32_t* d_ok, hipStream_t stream);
int test_fq12_op(int op, int which, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, hipStream_t stream);
struct prepared_bases {   // table[w * n + i] = 2^(o_w) * P_i with o_w the bit offset of window w (c w; balanced widths above 16 bits: msm.hip win_off)
  uint32_t* table;
  size_t n;
  int c, W;
  uint32_t* direct = nullptr;   // small sets only (msm.hip "Direct tables"): [i][w < 32][m - 1 < 128] = m 2^(8 w) P_i, or null
};
// bucket-free MSM over a direct table (single vector, n <= 2^15 by default)
size_t direct_table_bytes(size_t n);
size_t msm_direct_workspace_bytes(size_t n);
int prepare_direct_table(prepared_bases* pb, const uint32_t* d_bases, hipStream_t stream);
int msm_g1_direct(const uint32_t* d_scalars, size_t n, const prepared_bases* pb, size_t off, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
int msm_pick_window_prepared(size_t n);
int msm_g1_device(const uint32_t* d_scalars, const uint32_t* d_bases, size_t n, uint32_t* d_out, void* ws, size_t ws_bytes,
                  int c_override, hipStream_t stream, const prepared_bases* prepared = nullptr, size_t prepared_off = 0, size_t batch = 1,
                  size_t scalar_stride = 0);
// chunked prepared MSM: pieces of at most chunk_cap scalars, sorted and accumulated one by one into one bucket set, one reduction at the end
size_t msm_chunk_workspace_bytes(size_t chunk_cap, int c);
int msm_chunk_add(const uint32_t* d_scalars, size_t n, const prepared_bases* pb, size_t pb_off, size_t chunk_cap, bool first, void* ws, size_t ws_bytes, hipStream_t stream);
int msm_chunk_finish(const prepared_bases* pb, size_t chunk_cap, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
// n_whole: size of the array this set is a shard of (0 = n): the direct table is meant for SMALL base sets, not for the shards of a large one
int prepare_bases_device(const uint32_t* d_bases, size_t n, hipStream_t stream, prepared_bases** out, int c_override = 0, size_t n_whole = 0);
void release_prepared(prepared_bases* pb);
// d_out[b] = sum over i < m of d_in[i * count + b], b < count (count = 1: the plain fold of m points)
int sum_jacobian_device(const uint32_t* d_in, int m, uint32_t* d_out, hipStream_t stream, size_t count = 1);
size_t g1_batch_normalize_workspace(size_t n);
int g1_batch_normalize_device(const uint32_t* d_in, size_t n, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
size_t g1_fft_workspace(size_t n);
int g1_fft_device(const uint32_t* d_in, int in_format, uint32_t* d_out, int out_format, uint32_t log_n, const uint32_t omega_ext[8],
                  const uint32_t* scale_ext, void* ws, size_t ws_bytes, hipStream_t stream);

// ntt.hip
int ntt_passes(uint32_t L);
int ntt_transform(const uint32_t* d_in, uint32_t in_len, uint32_t in_stride, uint32_t* d_out, uint32_t out_len, uint32_t out_stride,
                  uint32_t batch, uint32_t L, const uint32_t omega_ext[8], const uint32_t* in_scale, uint32_t in_period,
                  const uint32_t* out_scale, uint32_t out_period, uint32_t* tmp0, uint32_t* tmp1, hipStream_t stream);
int fr_mul_periodic_device(uint32_t* d_a, size_t n, const uint32_t* d_table_ext, uint32_t period, hipStream_t stream);
int fr_scale_device(uint32_t* d_a, size_t n, const uint32_t scale_ext[8], hipStream_t stream);
void ntt_clear_cache();

// Small host arrays of a `_device` call (lists of column addresses, coefficients) on their way to device memory WITHOUT waiting for the stream:
// copied into a pinned slot first (the caller's memory is free when the call returns), then from there with hipMemcpyAsync.  Eight slots used in
// turn, an event per slot: the host runs up to eight uploads ahead of the stream before it has to wait for the oldest.  Owned by the caller's
// scratch set.  Anything larger than a slot -- or a null ring -- takes the plain path: copy from the caller's memory and synchronise the stream.
struct arg_ring {
  static constexpr int SLOTS = 8;
  static constexpr size_t SLOT_BYTES = 32768;
  void* host = nullptr;
  hipEvent_t ev[SLOTS] = {};
  bool used[SLOTS] = {};
  int turn = 0;
  int upload(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    if (bytes == 0) return ZKHIP_OK;
    if (bytes > SLOT_BYTES) return plain(dst, src, bytes, stream);
    if (!host && hipHostMalloc(&host, SLOTS * SLOT_BYTES, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); host = nullptr; return plain(dst, src, bytes, stream); }
    const int s = turn;
    turn = (turn + 1) % SLOTS;
    if (!ev[s] && hipEventCreateWithFlags(&ev[s], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev[s] = nullptr; return plain(dst, src, bytes, stream); }
    if (used[s] && hipEventSynchronize(ev[s]) != hipSuccess) { set_error("arg_ring: event wait failed"); return ZKHIP_EHIP; }
    void* slot = (char*)host + (size_t)s * SLOT_BYTES;
    std::memcpy(slot, src, bytes);
    if (hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, stream) != hipSuccess || hipEventRecord(ev[s], stream) != hipSuccess) { set_error("arg_ring: copy failed"); return ZKHIP_EHIP; }
    used[s] = true;
    return ZKHIP_OK;
  }
  static int plain(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) { set_error("upload of call arguments failed"); return ZKHIP_EHIP; }
    return ZKHIP_OK;
  }
  void release() {
    for (int i = 0; i < SLOTS; i++) if (ev[i]) { if (used[i]) (void)hipEventSynchronize(ev[i]); (void)hipEventDestroy(ev[i]); ev[i] = nullptr; used[i] = false; }
    if (host) { (void)hipHostFree(host); host = nullptr; }
  }
};
static inline int upload_args(arg_ring* ring, void* dst, const void* src, size_t bytes, hipStream_t stream) {
  return ring ? ring->upload(dst, src, bytes, stream) : arg_ring::plain(dst, src, bytes, stream);
}

// poly.hip
size_t poly_workspace_bytes(size_t n);
int fr_eval_polynomial_device(const uint32_t* d_a, size_t n, const uint32_t x_host[8], uint32_t* d_result, void* ws, size_t ws_bytes, hipStream_t stream);
size_t poly_batch_workspace_bytes(size_t n, size_t count);
int fr_eval_polynomial_batch_device(const void* const* d_polys_host, size_t count, size_t n, const uint32_t x_host[8], uint32_t* d_results,
                                    void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);
int fr_kate_division_device(const uint32_t* d_a, size_t n, const uint32_t b_host[8], uint32_t* d_q, void* ws, size_t ws_bytes, hipStream_t stream);
// quotient of a(X) by prod_i (X - roots[i]) (m <= ZKHIP_MAX_ROOTS distinct canonical roots, external words, host memory): d_q gets n elements (n - m
// coefficients, m zeros), d_evals (nullable) a(roots[i]).  d_q must not overlap d_a.
size_t poly_roots_workspace_bytes(size_t n, uint32_t m);
int fr_divide_by_roots_device(const uint32_t* d_a, size_t n, const uint32_t (*roots_host)[8], uint32_t m, uint32_t* d_q, uint32_t* d_evals, void* ws,
                              size_t ws_bytes, hipStream_t stream);
int fr_prefix_product_device(const uint32_t* d_v, size_t n, uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
int fr_batch_invert_device(uint32_t* d_a, size_t n, void* ws, size_t ws_bytes, hipStream_t stream);
// the l0 / l_last / l_active_row cosets of the proving key over a window of W elements (global rows start, start + 1, ... mod 2^ext_k), closed form.
// consts: zeta, ext_omega, ext_omega^64, ext_omega^-64, ext_omega^(64 n), ext_omega^(-64 n), 1 / n, omega, omega^u, omega^(first index of A)
int fr_lagrange_cosets_window_device(uint32_t* out_l0, uint32_t* out_last, uint32_t* out_active, size_t W, uint64_t start, uint32_t k, uint32_t ext_k,
                                     uint32_t n_terms, int active_is_sum, const uint32_t consts[10][8], hipStream_t stream);
size_t lincomb_workspace_bytes(size_t count, size_t n);
int fr_linear_combination_device(const void* const* d_cols_host, const uint32_t* coeffs_host, size_t count, size_t n, uint32_t* d_out, void* ws, size_t ws_bytes,
                                 hipStream_t stream, arg_ring* ring = nullptr);
size_t perm_workspace_bytes(uint32_t nperm, uint32_t chunk, uint32_t log_n);
int fr_permutation_products_device(const void* const* d_values_host, const void* const* d_sigmas_host, uint32_t nperm, uint32_t chunk, uint32_t log_n,
                                   size_t usable, const uint32_t beta[8], const uint32_t gamma[8], const uint32_t delta[8], const uint32_t omega[8],
                                   uint32_t* d_z, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);
size_t lookup_products_workspace_bytes(uint32_t n_lookups, uint32_t log_n);
int fr_lookup_products_device(const void* const* d_inputs_host, const void* const* d_tables_host, const uint32_t* d_permuted_inputs, const uint32_t* d_permuted_tables,
                              uint32_t n_lookups, uint32_t log_n, size_t usable, const uint32_t beta[8], const uint32_t gamma[8], uint32_t* d_z, void* ws,
                              size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);

// rowvm.hip (the blob a launch reads, its plan, row_vm_workspace_bytes and row_vm_halos: rowvm_blob.hpp)
int row_vm_validate(const zkhip_vm_program* p, uint32_t n_columns, uint32_t log_rows, int accumulate);
// Pinned host staging for the blob of a launch (two buffers, used alternately; an event per buffer says when the copy that read it has
// completed).  With it row_vm_launch never waits for the stream: the host builds launch i + 1 while launch i runs.  Owned by the caller's
// scratch set (one user at a time).
struct vm_staging {
  void* host[2] = {nullptr, nullptr};
  size_t cap[2] = {0, 0};
  hipEvent_t copied[2] = {nullptr, nullptr};
  int turn = 0;
  void release();
};
// One launch of row programs over Fr columns.  The forms:
//   VM_WHOLE   every row of a 2^log_rows domain, column i = 2^log_rows elements indexed modulo the domain.  One program writes d_out
//              (accumulate: reads it first, ZKHIP_SRC_PREV); with d_outs set, n_progs programs run side by side in ONE launch, program p
//              writing d_outs[p] (PREV reads 0; programs that read ZKHIP_SRC_ROWPOW must agree on omega)
//   VM_WINDOW  one program over `count` rows from global row `row0`.  Column i is a window buffer of halo_lo + count + halo_hi elements,
//              element t = column[(row0 - halo_lo + t) mod 2^log_rows] (row_vm_halos); ROWPOW is omega^((row0 + i) mod 2^log_rows); PREV / the
//              output are d_out[i], i < count.  log_rows = 0 makes it `count` independent rows of programs without rotations or ROWPOW
//   VM_CHECK   the witness checks' gates (include/zkhip.h, check_report.hpp): n_progs programs side by side over rows [row0, row0 + count) of
//              whole-domain columns, nothing stored: d_out = n_progs zkhip_check_report records, initialised by the call
// One program alone is tried on the run-time compiler first (rowvm_jit.hip: short programs over many rows) unless interpreter_only;
// *compiled (if given): 1 when a compiled kernel took the call.  ws: row_vm_workspace_bytes(progs, n_progs, n_columns, log_rows).
enum vm_form { VM_WHOLE, VM_WINDOW, VM_CHECK };
struct vm_call {
  const zkhip_vm_program* progs = nullptr;
  uint32_t n_progs = 1;
  const void* const* d_columns = nullptr;
  uint32_t n_columns = 0, log_rows = 0;
  vm_form form = VM_WHOLE;
  uint64_t row0 = 0, count = 0;
  int accumulate = 0;
  uint32_t* d_out = nullptr;
  uint32_t* const* d_outs = nullptr;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  hipStream_t stream = nullptr;
  vm_staging* staging = nullptr;
  bool interpreter_only = false;
  int* compiled = nullptr;
};
int row_vm_launch(const vm_call& c);
// rowvm_jit.hip: row programs compiled at run time with hiprtc (straight-line code per program shape, cached per device)
bool row_vm_jit_wanted(const zkhip_vm_program* p, uint32_t n_columns, uint32_t log_rows);
bool row_vm_jit_wanted_window(const zkhip_vm_program* p, uint32_t n_columns, uint64_t count);
int row_vm_jit_launch(const zkhip_vm_program* p, const void* const* d_columns, uint32_t n_columns, uint32_t log_rows, bool window, uint64_t row0, uint64_t count,
                      int accumulate, const uint32_t* d_consts, const uint32_t* d_pow_lo, const uint32_t* d_pow_hi, uint32_t* d_out, hipStream_t stream);
void row_vm_jit_clear();
uint64_t row_vm_jit_launches();        // how many launches of this process went through a compiled kernel (never reset)
int row_vm_jit_source(const zkhip_vm_program* p, uint32_t n_columns, uint32_t log_rows, std::string* out);
int row_vm_jit_compile_only(const zkhip_vm_program* p, uint32_t n_columns, uint32_t log_rows, size_t* code_bytes);
int fr_pointwise_mul_device(const uint32_t* d_a, const uint32_t* d_b, size_t n, uint32_t* d_out, hipStream_t stream);
int fr_gather_mul_device(const uint32_t* d_a, uint32_t a_len, const uint32_t* d_ia, const uint32_t* d_b, uint32_t b_len, const uint32_t* d_ib, size_t n,
                         uint32_t* d_out, hipStream_t stream);
// The witness checks (include/zkhip.h, "witness checks"; check_report.hpp).  d_reports: zkhip_check_report records, initialised by the call.
// reports[i] = (0, none) for i < n, on `stream`
int check_reports_init_device(void* d_reports, uint32_t n, hipStream_t stream);
// copy constraints: d_columns_dev is the DEVICE array of the n_columns column addresses
int check_copies_device(const void* d_columns_dev, uint32_t n_columns, uint32_t log_n, const uint32_t* d_map_col, const uint32_t* d_map_row, void* d_report,
                        hipStream_t stream);

// lookup.hip
size_t lookup_permute_workspace_bytes(size_t usable_rows);
int lookup_permute_device(const uint32_t* d_input, const uint32_t* d_table, size_t usable_rows, uint32_t* d_out_input, uint32_t* d_out_table,
                          void* ws, size_t ws_bytes, hipStream_t stream);
// every lookup of a circuit at once: n_lookups device addresses each in host memory; outputs [n_lookups][n] dense, rows < usable_rows written
size_t lookup_permute_many_workspace_bytes(uint32_t n_lookups, size_t usable_rows);
int lookup_permute_many_device(const void* const* d_inputs_host, const void* const* d_tables_host, uint32_t n_lookups, size_t n, size_t usable_rows,
                               uint32_t* d_out_input, uint32_t* d_out_table, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);
// lookup membership (the witness check): report l counts the rows i < usable_rows whose input_l[i] is no table_l[j], j < usable_rows
size_t lookup_check_workspace_bytes(uint32_t n_lookups, size_t usable_rows);
int lookup_check_device(const void* const* d_inputs_host, const void* const* d_tables_host, uint32_t n_lookups, size_t usable_rows, void* d_reports, void* ws,
                        size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);

// random.hip: the random Fr stream of fr_random.hpp (include/zkhip.h, "random field elements").  `seed`: 32 bytes of host memory, read before the call returns
int fr_random_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, size_t n, uint32_t* d_out, hipStream_t stream);
// element first + c * count + j to row row0 + j of column c (n_cols device addresses in host memory), one launch; n_cols * count <= 2^30
size_t fr_random_rows_workspace_bytes(uint32_t n_cols);
int fr_random_rows_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, const void* const* d_cols_host, uint32_t n_cols, size_t row0, size_t count,
                          void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);

// serde.hip
int g1_compress_device(const uint32_t* d_points, size_t n, uint32_t* d_out, int layout, hipStream_t stream);
int g1_decompress_device(const uint32_t* d_in, size_t n, uint32_t* d_points, int layout, unsigned long long* d_first_bad, hipStream_t stream);

// transcript.hip: the conversions that feed the transcript's hash (include/zkhip.h, "transcript").  All pointers 16-byte aligned.
uint32_t transcript_chunk(size_t n);      // points that share one inversion in a launch over n points
// n Jacobian points -> n x 96 bytes (canonical x | canonical y | GroupEncoding); the number of identity inputs is added to *d_ident (zero before the launch)
int transcript_points_device(const uint32_t* d_in, size_t n, uint32_t* d_out, int layout, uint32_t* d_ident, hipStream_t stream);
int transcript_scalars_device(const uint32_t* d_in, size_t n, uint32_t* d_out, hipStream_t stream);
// n affine points -> n x 64 bytes (canonical x | y); atomicMin of the indices of (0, 0) points into *d_first_bad
int transcript_affine_device(const uint32_t* d_points, size_t n, uint32_t* d_out, unsigned long long* d_first_bad, hipStream_t stream);

// poseidon.hip (include/zkhip.h, "Poseidon").  d_tab: poseidon.hpp's table in the kernels' limbs (POSEIDON_TAB_LEN x 9 words)
int poseidon_hash_many_device(const uint32_t* d_in, size_t n, uint32_t width, uint32_t* d_out, const uint32_t* d_tab, hipStream_t stream);
// n secp256k1 points (16 canonical words each) packed and hashed: layout 0 the nullifier's (width 4), 1 the member's (width 6)
int poseidon_hash_points_device(const uint32_t* d_points, size_t n, uint32_t layout, uint32_t* d_out, const uint32_t* d_tab, hipStream_t stream);
size_t poseidon_merkle_workspace(size_t n);
int poseidon_merkle_device(const uint32_t* d_leaves, size_t n, uint32_t* d_nodes, const uint32_t* d_tab, void* ws, size_t ws_bytes, hipStream_t stream);

// imt.hip (include/zkhip.h, "indexed Merkle tree").  A batch of n_new insertions is 2 n_new events; the workspace holds, per event, the level-0
// key (8 bytes, uploaded), the preimage the event leaves behind (96 bytes, by time, uploaded) and three sets of (key, value) used level by level.
constexpr size_t IMT_WS_EVENT_BYTES = 8 + 96 + 32 + 2 * (8 + 32);          // the keys first, the preimages behind them: one upload
size_t imt_workspace_bytes(size_t n_new);
int imt_fill_device(uint32_t* d_dst, size_t n, const uint32_t value[8], hipStream_t stream);
int imt_insert_device(uint32_t depth, size_t n_new, void* ws, uint32_t* d_leaves, uint32_t* d_nodes, uint32_t* d_preimages, uint32_t* out_roots,
                      uint32_t* out_new_leaves, uint32_t* out_low_proofs, uint32_t* out_new_proofs, const uint32_t* d_tab, hipStream_t stream);

// paillier.hip (include/zkhip.h, "Paillier tally").  The context of n^2 is built on the host per call (modn.hpp) and handed to the kernels by value.
struct modn_ctx;
bool paillier_context(const uint64_t n[3], modn_ctx* ctx);      // false: n even or n < 3
size_t paillier_tally_workspace_bytes(size_t n_ballots, uint32_t n_cols);
int paillier_mul_device(const modn_ctx& ctx, const uint64_t* d_a, const uint64_t* d_b, size_t count, uint64_t* d_out, hipStream_t stream);
int paillier_tally_device(const modn_ctx& ctx, const uint64_t* d_ballots, size_t n_ballots, uint32_t n_cols, const uint64_t* d_init, uint64_t* d_running, void* ws,
                          size_t ws_bytes, hipStream_t stream);
int paillier_encrypt_device(const modn_ctx& ctx, const uint64_t n[3], const uint64_t g[6], const uint64_t* d_m, const uint64_t* d_r, size_t count, uint64_t* d_out,
                            hipStream_t stream);

// plume.hip (include/zkhip.h, "PLUME nullifiers on secp256k1").  The prefix of a batch's message is built on the host per call (secp256k1_h2c.hpp) and handed
// to the kernels by value.
struct h2c_prefix;
int secp256k1_lincomb_device(const uint64_t* d_a, const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_q, size_t count, uint64_t* d_out, uint32_t* d_status,
                             hipStream_t stream);
int secp256k1_hash_to_curve_device(const h2c_prefix& pre, const uint64_t* d_pk, size_t count, uint64_t* d_out, uint32_t* d_status, hipStream_t stream);
int plume_verify_device(const h2c_prefix& pre, const uint64_t* d_pk, const uint64_t* d_nullifier, const uint64_t* d_s, const uint64_t* d_c, size_t count, uint32_t* d_status,
                        void* d_report, uint64_t* d_h_out, hipStream_t stream);
// plume_sign.hip: d_h_out may be null
int plume_sign_device(const h2c_prefix& pre, const uint64_t* d_sk, const uint64_t* d_r, size_t count, uint64_t* d_pk, uint64_t* d_nullifier, uint64_t* d_s, uint64_t* d_c,
                      uint32_t* d_status, uint64_t* d_h_out, hipStream_t stream);

// verify_identity.hip (include/zkhip.h, "the quotient identity at x").  The two validators touch no device; `who` names the call in the error text.
int identity_domain_validate(const char* who, uint32_t k, uint64_t usable_rows, const uint64_t* omega);
int fr_domain_points_device(uint32_t k, uint32_t usable_rows, const uint64_t* omega, const uint32_t* d_x, uint64_t n_points, uint32_t* d_out, hipStream_t stream);
// Instance columns: `instance_layout` is the host arrays of a call, validated and resolved per query (offset of the query's column in a proof's
// public inputs, its length, its rotation mod 2^k); an empty layout (n_queries = 0) is the identity without instance columns.
constexpr uint32_t INSTANCE_MAX_QUERIES = 64;
struct instance_layout {
  uint64_t total_len = 0;
  uint32_t n_queries = 0;
  uint32_t offset[INSTANCE_MAX_QUERIES], len[INSTANCE_MAX_QUERIES], rot[INSTANCE_MAX_QUERIES];
};
// every column_lens[c] <= max_len (`max_name` says what that is in the error text), every query inside its tables
int instance_queries_validate(const char* who, uint32_t k, uint64_t max_len, const char* max_name, const uint32_t* column_lens, uint32_t n_columns,
                              const uint32_t* query_columns, const uint32_t* query_rotations, uint32_t n_queries, instance_layout* out);
int fr_instance_evals_device(uint32_t k, const uint64_t* omega, const uint32_t* d_x, const uint32_t* d_instances, const instance_layout& lay, uint64_t n_proofs,
                             uint32_t* d_out, hipStream_t stream);
int verify_identity_validate(const zkhip_vm_program* p, uint32_t n_evals, uint32_t n_queries);
size_t verify_identity_columns_bytes(uint32_t n_evals, uint32_t n_queries, uint64_t n_proofs);      // cols_ws: the column-major image, the result column, the in-domain flags
size_t verify_identity_vm_bytes(const zkhip_vm_program* p, uint32_t n_evals, uint32_t n_queries);   // vm_ws: the interpreter's workspace
int verify_identity_device(const zkhip_vm_program* prog, const uint32_t* d_evals, uint32_t n_evals, const uint32_t* d_challenges, uint32_t k, uint32_t usable_rows,
                           const uint64_t* omega, const uint32_t* d_instances, const instance_layout& lay, uint64_t n_proofs, int32_t* d_status, void* d_report,
                           void* cols_ws, void* vm_ws, size_t vm_ws_bytes, hipStream_t stream, vm_staging* staging);

// gwc_fold.hip (include/zkhip.h, "the batch verifier").  The validator touches no device; `ws` holds the plan as the kernel reads it / the
// second level's partial sums.
int gwc_plan_validate(const zkhip_gwc_plan* plan, uint32_t k, const uint64_t* omega);
size_t gwc_scalars_workspace_bytes(const zkhip_gwc_plan* plan);
int gwc_scalars_device(const zkhip_gwc_plan* plan, const uint32_t* d_evals, const uint32_t* d_points, uint32_t k, const uint64_t* omega, uint64_t n_proofs,
                       uint32_t* d_rows_a, uint32_t* d_rows_c, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);
size_t fold_rows_workspace_bytes(uint32_t n_cols, uint32_t n_own, uint64_t n_rows);
int fold_rows_device(const uint32_t* d_rows, uint32_t n_cols, uint32_t n_own, const uint32_t* d_r, uint32_t negate, uint64_t n_rows, uint32_t* d_out_own,
                     uint32_t* d_out_shared, void* ws, size_t ws_bytes, hipStream_t stream);

// shplonk_fold.hip (include/zkhip.h, "the batch verifier").  The marshaller validates the plan and builds the words the kernel reads, touching no
// device; `ws` holds those words.
int shplonk_plan_marshal(const zkhip_shplonk_plan* plan, uint32_t k, const uint64_t* omega, std::vector<uint32_t>* blob);
int shplonk_scalars_device(const std::vector<uint32_t>& blob, const uint32_t* d_evals, const uint32_t* d_points, uint64_t n_proofs, uint32_t* d_rows_a,
                           uint32_t* d_rows_c, uint32_t* d_status, void* ws, size_t ws_bytes, hipStream_t stream, arg_ring* ring = nullptr);

// row_msm.hip (include/zkhip.h, "KZG accumulators"; row_msm.hpp has the refusals and the launch arithmetic, kzg_limbs.hpp the limbs).
// `ws`: g1_row_msm_workspace(n_rows, n_cols) bytes, the partial sums of rows wider than one chunk.
size_t g1_row_msm_workspace(size_t n_rows, size_t n_cols);
int g1_row_msm_device(const uint32_t* d_rows, size_t n_cols, const uint32_t* d_own, size_t n_own, size_t own_stride, const uint32_t* d_shared, size_t n_rows,
                      uint32_t* d_out, void* ws, size_t ws_bytes, hipStream_t stream);
int kzg_limbs_encode_device(const uint64_t* d_affine, size_t n, uint64_t* d_out, hipStream_t stream);
int kzg_limbs_decode_device(const uint64_t* d_in, size_t n, uint64_t* d_affine, uint32_t* d_status, hipStream_t stream);

// selftest.hip
int test_field_op(int field, int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, size_t n, hipStream_t stream);
int g1_check_points_device(const uint32_t* d_points, size_t n, unsigned long long* d_first_bad, hipStream_t stream);
int test_g1_op(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, size_t n, hipStream_t stream);

}  // namespace zkhip

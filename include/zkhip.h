/* libzkhip -- MI355X (gfx950) kernels behind the halo2 prover's MSM / NTT boundary.  C ABI.
 *
 * Each entry point replaces one function of the un-vendored halo2-axiom crate [DEP] that the reference
 * reaches through `create_proof` (/root/reference/aggregator/src/wrapper.rs:129), `keygen_vk`/`keygen_pk`
 * (wrapper.rs:107-108) and `halo2_base::utils::testing::gen_proof`
 * (/root/reference/aggregator/benches/wrapper_circuit.rs:140).  SURVEY.md section 8(b) is the contract.
 *
 * Memory formats are exactly the Rust in-memory formats, so a Rust host passes slices through unchanged:
 *   Fr / Fq   : 4 x u64 little-endian limbs, Montgomery form (x * 2^256 mod p)            32 bytes
 *   G1Affine  : x || y  (identity = all-zero)                                             64 bytes
 *   G1        : x || y || z Jacobian (identity z = 0)                                     96 bytes
 * All buffers are caller-owned and borrowed for the duration of the call (registered bases: until
 * unregistered).  Every function returns ZKHIP_OK (0) or a negative ZKHIP_E* code and never aborts;
 * zkhip_last_error() describes the last failure on the calling thread.  There is no CPU fallback: without a
 * usable HIP device every compute entry point fails with ZKHIP_ENODEV.
 */
#ifndef ZKHIP_H
#define ZKHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ZKHIP_OK 0
#define ZKHIP_EINVAL (-1)  /* bad argument */
#define ZKHIP_ENODEV (-2)  /* no HIP device / init failed */
#define ZKHIP_EHIP (-3)    /* HIP runtime error, see zkhip_last_error() */
#define ZKHIP_ENOMEM (-4)  /* device allocation failed */
#define ZKHIP_EBUSY (-5)   /* zkhip_init with a different device list while host-buffer calls are running */

/* ---- lifecycle ----------------------------------------------------------------------------------- */
/* Name the HIP devices this process drives (`zkhip_init(const int *devices, int ndev)`).  devices == NULL
 * or ndev == 0: device 0 (or $ZKHIP_DEVICE).  devices[0] is the PRIMARY device: every `_device` entry point, every single transform and
 * every other vector operation runs there, and `_device` pointers are pointers into its memory.  With ndev > 1 the MSM over registered
 * bases is sharded by point range over all the devices (zkhip_register_bases below) and the polynomials of a BATCHED transform are
 * spread over them, each transform on one device (zkhip_set_ntt_fanout below) -- the 8 GPUs of one node behind one `create_proof`
 * process (/root/reference/aggregator/src/wrapper.rs:129).  Lazy init on first use is allowed (device 0).
 * Calling it again with the same list is a no-op; with a different list it shuts the library down first (ZKHIP_EBUSY while
 * host-buffer calls of other threads are still running).
 * Environment: ZKHIP_DEVICE (default device), ZKHIP_SHARDS (see zkhip_set_msm_shards), ZKHIP_HOST_LANES (1..4, default 2: host-buffer
 * calls that may be in flight at once, each with its own stream and scratch memory). */
int zkhip_init(const int *devices, int ndev);
void zkhip_shutdown(void);
const char *zkhip_last_error(void);
/* library / device identification, for logs: writes a NUL-terminated string (the primary device) */
int zkhip_device_name(char *buf, size_t len);
/* number of devices the library drives (0 when it cannot initialise) */
int zkhip_device_count(void);
/* Number of point-range shards zkhip_register_bases cuts an array into from now on: shard s of S covers points
 * [s n / S, (s + 1) n / S) (the first n % S shards one point more) and lives on device s % ndev.  Default: one shard per device.
 * More shards than devices ("virtual shards", also $ZKHIP_SHARDS) run the whole multi-GPU path -- per-shard tables, per-shard
 * Pippenger, gather of the 96-byte Jacobian partials, fold -- on fewer devices; the result is the same group element for every
 * shard count.  0 restores the default. */
int zkhip_set_msm_shards(int shards);
int zkhip_msm_shards(void);

/* Threads and streams.  Every entry point may be called from any host thread.  Host-buffer calls (no `_device` suffix) borrow one of
 * the library's lanes for the duration of the call, so up to ZKHIP_HOST_LANES of them run concurrently (one call's PCIe transfer
 * under another's kernels); further callers wait.  `_device` calls are asynchronous on the caller's stream and use scratch memory
 * that belongs to that stream: calls on different streams never share scratch, calls on one stream are ordered by the stream.  Two
 * host threads must not enqueue on the SAME stream at the same time (as with any HIP stream).  The profiling hooks
 * (zkhip_profile_*) are a single-caller debugging aid. */

/* ---- MSM: replaces `best_multiexp(coeffs: &[Fr], bases: &[G1Affine]) -> G1` ------------------------- */
/* [DEP] halo2_proofs/src/arithmetic.rs; called by ParamsKZG::commit / commit_lagrange.  n may be any value
 * (n == 0 gives the identity).  out_xyz: Jacobian, canonical Montgomery limbs, any valid representative. */
int zkhip_msm_g1(const uint64_t *scalars, const uint64_t *bases, size_t n, uint64_t out_xyz[12]);

/* Multi-column commit: `batch` scalar vectors (contiguous, n elements each) against the same bases, e.g. every advice column of
 * a circuit; out_xyz: batch Jacobian points.  With registered bases this is one launch set (see the _device variant). */
int zkhip_msm_g1_batch(const uint64_t *scalars, const uint64_t *bases, size_t n, size_t batch, uint64_t *out_xyz);

/* The same over G2 (`best_multiexp::<G2Affine>`): bases n x 16 limbs (G2Affine = x.c0 || x.c1 || y.c0 || y.c1, Montgomery Fq, all-zero =
 * identity), out 24 limbs (G2 Jacobian x || y || z, each an Fq2).  No call site in the reference prover multiplies in G2 (it reads
 * params.g2() / params.s_g2(): /root/reference/aggregator/src/wrapper.rs:1142-1144); provided because the MSM is generic over the
 * curve.  General path only (per-window bucket sets + window fold). */
int zkhip_msm_g2(const uint64_t *scalars, const uint64_t *bases, size_t n, uint64_t out_xyz[24]);

/* Residency for `ParamsKZG::{g, g_lagrange}` (static per params object): upload once and build the prepared table
 * (2^(c w) * P_i for every window w: W * 64 bytes per point of HBM, one-time ~25 ms per 2^20 points; arrays of at most 2^15 points
 * -- $ZKHIP_DIRECT_MAX_LOG -- also get every multiple of every 8-bit window point, 256 KiB per point, and their single MSMs need no
 * buckets: DESIGN.md section 3c) on every shard's device;
 * zkhip_msm_g1 recognises `bases` pointers inside a registered range (any sub-range), skips the upload and runs the prepared
 * path: one shared bucket set per shard, no window fold, one gather + fold of the shards' partial sums.
 * Contract: the caller keeps [bases, bases + 8 n) alive AND UNCHANGED until zkhip_unregister_bases -- the table is built from the
 * contents at registration.  Recognition is by address, so memory that was freed without unregistering and later reused for other
 * points would alias a stale table; as a guard the library keeps 8 sampled points of the registered array and treats a range whose
 * samples no longer match as not registered (correct result through the general path, slower).  Always unregister before freeing. */
int zkhip_register_bases(const uint64_t *bases, size_t n);
int zkhip_unregister_bases(const uint64_t *bases);

/* ---- NTT: replaces `best_fft(a: &mut [Fr], omega: Fr, log_n: u32)` --------------------------------- */
/* In place, natural order in and out: a[i] <- sum_j a[j] * omega^(i j).  log_n <= 28. */
int zkhip_ntt_fr(uint64_t *a, const uint64_t omega[4], uint32_t log_n);

/* `batch` contiguous polynomials, each transformed in place, one launch set per device.  With several devices (zkhip_init) the batch is
 * cut into contiguous shares, one per device: every transform runs on ONE device (independent polynomials are
 * independent units), every device moves its share over its own PCIe link; results do not depend on the device count. */
int zkhip_ntt_fr_batch(uint64_t *a, const uint64_t omega[4], uint32_t log_n, uint32_t batch);
/* Which batched transforms are spread over the devices: 0 none, 1 (default) the host-buffer forms (zkhip_ntt_fr_batch,
 * zkhip_ifft_scaled_batch, zkhip_coeff_to_extended_batch), 2 also the `_device` batch forms (zkhip_ntt_fr_batch_device,
 * zkhip_ifft_scaled_batch_device, zkhip_coeff_to_extended_device, zkhip_extended_to_coeff_device: a secondary device pulls its
 * polynomials from the primary's HBM over xGMI, transforms them with its own twiddle plan and pushes the results back -- off by
 * default).  $ZKHIP_NTT_FANOUT sets the initial mode. */
int zkhip_set_ntt_fanout(int mode);
int zkhip_ntt_fanout(void);

/* ---- EvaluationDomain pieces ([DEP] halo2_proofs/src/poly/domain.rs), host buffers ----------------- */
/* `EvaluationDomain::ifft`: best_fft with omega_inv, then every element times `divisor`. */
int zkhip_ifft_scaled(uint64_t *a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4]);
/* the same for `batch` contiguous polynomials (`lagrange_to_coeff` of every advice column of a phase in one call) */
int zkhip_ifft_scaled_batch(uint64_t *a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], uint32_t batch);
/* `coeff_to_extended`: a (2^k coeffs) -> out (2^ext_k evaluations on the coset zeta * <ext_omega>):
 * distribute_powers_zeta(into_coset) (a[i] *= {1, zeta, zeta^2}[i % 3]), zero-pad, best_fft. */
int zkhip_coeff_to_extended(const uint64_t *a, uint32_t k, uint64_t *out, uint32_t ext_k, const uint64_t ext_omega[4],
                            const uint64_t zeta[4]);
/* `batch` polynomials: a[b * 2^k ..] -> out[b * 2^ext_k ..] (the per-column loop of the quotient phase in one call) */
int zkhip_coeff_to_extended_batch(const uint64_t *a, uint32_t k, uint64_t *out, uint32_t ext_k, uint32_t batch, const uint64_t ext_omega[4],
                                  const uint64_t zeta[4]);
/* `extended_to_coeff`: ifft on the extended domain, distribute_powers_zeta(out of coset), truncate to
 * out_len elements (= n * quotient_poly_degree).  `a` is consumed (overwritten). */
int zkhip_extended_to_coeff(uint64_t *a, uint32_t ext_k, const uint64_t ext_omega_inv[4], const uint64_t ext_divisor[4],
                            const uint64_t zeta[4], uint64_t *out, size_t out_len);
/* `divide_by_vanishing_poly`: a[i] *= table[i % period] (table = inverted t_evaluations). */
int zkhip_mul_periodic(uint64_t *a, size_t n, const uint64_t *table, uint32_t period);

/* ---- Fr-vector primitives of the prover besides the NTT ------------------------ */
/* `eval_polynomial(poly, point)` [DEP arithmetic.rs]: out = sum poly[i] * point^i. */
int zkhip_fr_eval_polynomial(const uint64_t *poly, size_t n, const uint64_t point[4], uint64_t out[4]);
/* `kate_division(a, b)` [DEP arithmetic.rs]: quotient of a(X) by (X - b), remainder dropped; q has n - 1 elements. */
int zkhip_fr_kate_division(const uint64_t *a, size_t n, const uint64_t b[4], uint64_t *q);
/* `BatchInvert::batch_invert` [DEP ff]: in place, zeros stay zero. */
int zkhip_fr_batch_invert(uint64_t *a, size_t n);
/* grand-product running product [DEP plonk/permutation/prover.rs]: out[0] = 1, out[i] = v[0] * ... * v[i-1] (out may alias v). */
int zkhip_fr_prefix_product(const uint64_t *v, size_t n, uint64_t *out);
int zkhip_fr_eval_polynomial_device(const void *d_poly, size_t n, const uint64_t point[4], void *d_out, void *stream);
int zkhip_fr_kate_division_device(const void *d_a, size_t n, const uint64_t b[4], void *d_q, void *stream);
/* `div_by_vanishing(a, roots)` [DEP poly/kzg/multiopen/shplonk/prover.rs]: quotient of a(X) by Z(X) = prod_i (X - roots[i]) for 1 <= m <=
 * ZKHIP_MAX_ROOTS pairwise distinct canonical roots, remainder dropped -- the same bytes as m successive `kate_division`s in any order, in
 * one pass structure (a read twice, q written once, whatever m).  q has n elements: n - m coefficients followed by m zeros (all zeros when
 * n <= m).  evals (nullable) receives a(roots[i]), i < m: with the roots these are the remainder.  `roots` is host memory ([m][4]) in both
 * forms.  d_q must not overlap d_a.  ZKHIP_EINVAL (nothing enqueued): m = 0, m > ZKHIP_MAX_ROOTS, null roots, null a / q with n > 0, a root
 * >= r, two equal roots.  n = 0 is ZKHIP_OK (evals, if asked for, are zeros). */
#define ZKHIP_MAX_ROOTS 8
int zkhip_fr_divide_by_roots(const uint64_t *a, size_t n, const uint64_t *roots, uint32_t m, uint64_t *q, uint64_t *evals);
int zkhip_fr_divide_by_roots_device(const void *d_a, size_t n, const uint64_t *roots, uint32_t m, void *d_q, void *d_evals, void *stream);
/* multiopen: `count` device-resident polynomials of n coefficients each (d_polys: host array of device pointers), all evaluated at
 * `point`; d_out receives count results (32 bytes each).  One launch per recursion level for the whole batch. */
int zkhip_fr_eval_polynomial_batch_device(const void *const *d_polys, size_t count, size_t n, const uint64_t point[4], void *d_out, void *stream);
int zkhip_fr_batch_invert_device(void *d_a, size_t n, void *stream);
int zkhip_fr_prefix_product_device(const void *d_v, size_t n, void *d_out, void *stream);

/* ---- row programs: the quotient numerator and every other pointwise pass ---------- */
/* [DEP] halo2_proofs/src/plonk/evaluation.rs evaluates h(X)'s numerator row by row over the extended coset with a small
 * straight-line program per row (`GraphEvaluator`: `Calculation::{Add,Sub,Mul,Square,Double,Negate,Horner,Store}` over
 * `ValueSource::{Constant,Intermediate,Fixed,Advice,Instance,Challenge,Beta,Gamma,Theta,Y,PreviousValue}` with rotations
 * `(row + rot * rot_scale) mod rows`), followed by hand-written permutation / lookup terms of the same shape; reached from
 * create_proof, /root/reference/aggregator/src/wrapper.rs:129.  `zkhip_fr_eval_rows` runs such a program for every row in one
 * fused pass: each thread owns a row, the program is decoded once per wavefront.  The same entry point expresses the
 * multiopen linear combinations, `divide_by_vanishing_poly`, and the numerators / denominators of the grand products.
 *
 * Operands (zkhip_vm_operand):
 *   ZKHIP_SRC_CONST   constants[index]                 (Constant / Challenge / Beta / Gamma / Theta / Y of the reference)
 *   ZKHIP_SRC_REG     register `index` < ZKHIP_VM_REGS (Intermediate; registers start at 0 for every row)
 *   ZKHIP_SRC_COLUMN  columns[index][(row + rotations[rot] * rot_scale) mod rows]      (Fixed / Advice / Instance)
 *   ZKHIP_SRC_PREV    out[row] as it was before the call (PreviousValue); 0 unless `accumulate`
 *   ZKHIP_SRC_ROWPOW  omega^row  (the reference's running `beta_term *= extended_omega`; needs `omega`)
 * Instructions: dst = MOV a | a + b | a - b | a * b | -a | 2a | a^2 | a * b + c.   out[row] = register `result_reg`.
 * rows = 2^log_rows; all field elements are canonical Montgomery Fr words, in and out.  The register file stays in VGPRs, and the
 * library runs the kernel variant sized for the highest register a program names (6 / 8 / 12 / 16: fewer registers = more waves in
 * flight), so a host compiling a `GraphEvaluator` should reuse registers (linear scan over last uses) and number them from 0. */
#define ZKHIP_VM_REGS 16
enum { ZKHIP_SRC_CONST = 0, ZKHIP_SRC_REG = 1, ZKHIP_SRC_COLUMN = 2, ZKHIP_SRC_PREV = 3, ZKHIP_SRC_ROWPOW = 4 };
enum { ZKHIP_OP_MOV = 0, ZKHIP_OP_ADD = 1, ZKHIP_OP_SUB = 2, ZKHIP_OP_MUL = 3, ZKHIP_OP_NEG = 4, ZKHIP_OP_DBL = 5, ZKHIP_OP_SQR = 6,
       ZKHIP_OP_MAD = 7 };
typedef struct zkhip_vm_operand { uint8_t kind; uint8_t rot; uint16_t index; } zkhip_vm_operand;
typedef struct zkhip_vm_insn { uint8_t op; uint8_t dst; uint16_t reserved; zkhip_vm_operand a, b, c; } zkhip_vm_insn;   /* 16 bytes */
typedef struct zkhip_vm_program {
  const zkhip_vm_insn *insns; uint32_t n_insns;
  const uint64_t *constants;  uint32_t n_constants;   /* n_constants x 4 words, host memory */
  const int32_t *rotations;   uint32_t n_rotations;   /* rotation slots, in rows of the base domain */
  int32_t rot_scale;                                  /* 1 on the base domain, 2^(extended_k - k) on the extended one */
  uint32_t result_reg;
  const uint64_t *omega;                              /* 4 words or NULL when ZKHIP_SRC_ROWPOW is not used */
} zkhip_vm_program;
/* columns: n_columns host pointers to 2^log_rows elements each; out: 2^log_rows elements (read first when accumulate != 0) */
int zkhip_fr_eval_rows(const zkhip_vm_program *prog, const uint64_t *const *columns, uint32_t n_columns, uint32_t log_rows,
                       int accumulate, uint64_t *out);
/* same with device-resident columns / output (`d_columns` itself is a host array of device pointers; out may alias a column
 * only if that column is read at rotation 0 exclusively) */
int zkhip_fr_eval_rows_device(const zkhip_vm_program *prog, const void *const *d_columns, uint32_t n_columns, uint32_t log_rows,
                              int accumulate, void *d_out, void *stream);
/* Short programs over many rows (at most 256 instructions, at least 2^18 rows, at most 96 columns) run as straight-line code compiled at
 * run time with hiprtc -- once per (program shape, rows, device), cached; constants stay a table, so one compilation serves every proof of a
 * circuit -- and every other program, or any failure to compile, through the interpreter: same results.  $ZKHIP_VM_JIT = 0 switches it off.
 * zkhip_vm_jit_source returns the generated source (buf may be NULL; *len = bytes needed incl. NUL); zkhip_vm_jit_compile compiles it without
 * launching anything (no device needed), e.g. at keygen, so that the first proof does not pay the seconds of compilation. */
int zkhip_vm_jit_source(const zkhip_vm_program *prog, uint32_t n_columns, uint32_t log_rows, char *buf, size_t cap, size_t *len);
int zkhip_vm_jit_compile(const zkhip_vm_program *prog, uint32_t n_columns, uint32_t log_rows, size_t *code_bytes);
/* Test hook: how many row-program launches of this process went through a compiled kernel (every entry point: whole-domain, window, sharded;
 * never reset).  The interpreter takes over silently with the same results, so this is the only way to tell which executor a call ran. */
uint64_t zkhip_test_rows_compiled_count(void);
/* Window form: `count` rows starting at global row `row0` of a 2^log_rows domain, e.g. one device's share of the rows.  With
 * o_i = rotations[i] * rot_scale (signed, not reduced), halo_lo = max(0, max_i(-o_i)) and halo_hi = max(0, max_i(o_i)), each d_windows[c]
 * is a WINDOW BUFFER of W = halo_lo + count + halo_hi elements: element t = column_c[(row0 - halo_lo + t) mod 2^log_rows] (valid for W >
 * 2^log_rows too: the values repeat).  Operand COLUMN@rot at local row i reads window[i + halo_lo + o_rot]; ROWPOW is
 * omega^((row0 + i) mod 2^log_rows); PREV and the result are d_out[i], i < count.  Both executors (interpreter and compiled; the compiled one
 * for windows of at least 2^18 rows, one code object for every row0 / count).  ZKHIP_EINVAL for row0 >= 2^log_rows, count == 0 or
 * count > 2^log_rows, a null window, or a program zkhip_fr_eval_rows_device rejects. */
int zkhip_fr_eval_rows_window_device(const zkhip_vm_program *prog, const void *const *d_windows, uint32_t n_columns, uint32_t log_rows,
                                     uint64_t row0, uint64_t count, int accumulate, void *d_out, void *stream);
/* The quotient numerator sharded by rows over the devices of zkhip_init.  Column c is ZKHIP_COL_COEFF (2^k coefficients on the primary
 * device, taken to the extended coset with coeff_to_extended(ext_omega, zeta) on the device that owns it) or ZKHIP_COL_EXTENDED (2^ext_k
 * coset values already on the primary: the proving key's fixed / sigma / l_0 / l_last / l_active cosets).  d_out (2^ext_k elements on the
 * primary) receives, byte for byte, what zkhip_coeff_to_extended_device on every COEFF column followed by
 * zkhip_fr_eval_rows_device(prog, ..., ext_k, accumulate = 0) writes (PREV reads 0), for every device count.
 * With S devices: rows are cut by shard_range(2^ext_k, j, S) and the COEFF columns, in argument order, by shard_range(n_coeff, j, S); each
 * owner pulls its COEFF columns from the primary and transforms them; device j fills its window buffers (peer copies from the owners and
 * from the primary), runs the window kernel and copies its rows into d_out.  S = 1: the transforms and the whole-domain launch, no copies.
 * Asynchronous on `stream` like every `_device` call; back-to-back calls on one stream, and calls on different streams, are safe.
 * Scratch is kept until zkhip_shutdown (S = 1: per caller stream; S > 1: per device); a second call of the same shape allocates nothing.
 * No host thread waits for a device, except when S > 1 and a call needs more scratch than any call before it: then the previous call's
 * copies are waited for before the buffers they read are replaced.  With zkhip_profile_enable the call records the phases transform,
 * exchange, rows_compiled | rows_interpreted (the primary's executor) and gather on `stream`, for every S (exchange and gather are empty
 * intervals when S = 1).  ZKHIP_EINVAL: a null pointer, a form other than 0 / 1 / 2, k > ext_k, ext_k > 28, a program
 * zkhip_fr_eval_rows_device rejects. */
#define ZKHIP_COL_COEFF    0u
#define ZKHIP_COL_EXTENDED 1u
/* ZKHIP_COL_ROW_SHARDS: d_columns[c] is a HOST pointer to a zkhip_row_shard_ref naming column `col` of a row-shard set (below).  Device j
 * passes its own window of that column to the window kernel, offset by (set halo_lo - program halo_lo) elements: no copy (S = 1: the whole-domain
 * launch reads the same buffer from offset halo_lo).  ZKHIP_EINVAL, nothing enqueued, when the pointer is device memory, the set is not live,
 * was made under another device count, has another ext_k, has halos narrower than the program's, or `col` is out of range. */
#define ZKHIP_COL_ROW_SHARDS 2u
int zkhip_fr_eval_rows_sharded_device(const zkhip_vm_program *prog, const void *const *d_columns, const uint32_t *forms, uint32_t n_columns,
                                      uint32_t k, uint32_t ext_k, const uint64_t ext_omega[4], const uint64_t zeta[4], void *d_out, void *stream);
/* Row-shard sets: n_cols columns of a 2^ext_k domain cut by rows over the S devices zkhip_init has at creation, rows of device j =
 * shard_range(2^ext_k, j, S) (the sharded evaluator's cut).  Device j holds, per column, one window buffer in the layout of
 * zkhip_fr_eval_rows_window_device: halo_lo + count_j + halo_hi elements, element t = column[(row0_j - halo_lo + t) mod 2^ext_k] (also when the
 * window is longer than the domain); one allocation per device, [col][W_j].  What they are for: the proving key's cosets stay on the device
 * that evaluates their rows, from keygen / key load on, and the quotient pulls nothing from the primary for them.
 * The `_device` calls are asynchronous on `stream` like the evaluator (secondaries start behind an entry event, the caller's stream waits for
 * them): a set written on a stream and read by a call on the same stream needs no host sync.  _scatter_device / _gather_device: a whole column
 * (2^ext_k elements on the primary) into / out of the set.  _upload: each device's window straight from host memory (hipMemcpy over that
 * device's own link, device after device; the host buffer may be reused on return; waits for the set's earlier work first).  _window: the
 * address, device ordinal, row0 and count of one shard's window of one column.  _destroy waits for the work enqueued on the set (its own
 * events, not the devices) and frees it; zkhip_shutdown frees every set.  ZKHIP_EINVAL with a message, nothing enqueued: a handle the library
 * did not issue or has freed, a set made under another device count, col / shard out of range, a null pointer. */
typedef struct zkhip_row_shards zkhip_row_shards;
typedef struct { const zkhip_row_shards *set; uint32_t col; } zkhip_row_shard_ref;
int zkhip_row_shards_create(uint32_t ext_k, uint32_t n_cols, uint32_t halo_lo, uint32_t halo_hi, zkhip_row_shards **out);
int zkhip_row_shards_destroy(zkhip_row_shards *set);
int zkhip_row_shards_window(const zkhip_row_shards *set, uint32_t shard, uint32_t col, void **d_window, int *device, uint64_t *row0, uint64_t *count);
int zkhip_row_shards_scatter_device(zkhip_row_shards *set, uint32_t col, const void *d_src, void *stream);
int zkhip_row_shards_gather_device(const zkhip_row_shards *set, uint32_t col, void *d_dst, void *stream);
int zkhip_row_shards_upload(zkhip_row_shards *set, uint32_t col, const void *host_src);
/* Columns col0 .. col0 + n_polys - 1 of the set = coeff_to_extended(ext_omega, zeta) of n_polys polynomials of 2^k coefficients on the primary
 * (polynomial i at d_coeff + i * coeff_stride elements): the bytes of zkhip_coeff_to_extended_device followed by a scatter.  The polynomials
 * are spread over the devices by shard_range(n_polys, j, S); each owner transforms one at a time into a 2^ext_k scratch of its own (its own
 * twiddle plan) and sends every device its window.  Nothing of n_polys x 2^ext_k is allocated. */
int zkhip_coeff_to_extended_row_shards_device(const void *d_coeff, uint32_t k, uint32_t n_polys, size_t coeff_stride, const uint64_t ext_omega[4],
                                              const uint64_t zeta[4], zkhip_row_shards *set, uint32_t col0, void *stream);
/* Columns col0, col0 + 1, col0 + 2 of the set = the proving key's l0, l_last (row u) and l_active_row (rows < u) on the extended coset, for a
 * 2^k domain with generator omega: l_i(X) = omega^i (X^n - 1) / (n (X - omega^i)) at X = zeta ext_omega^t, l_active = the shorter of
 * sum_{i<u} l_i and 1 - sum_{i>=u} l_i.  Every device writes its own windows (one kernel, no transform, no copy); the bytes equal
 * zkhip_ifft_scaled + zkhip_coeff_to_extended of the indicator columns.  ZKHIP_EINVAL unless 1 <= u < 2^k and k <= the set's ext_k. */
int zkhip_lagrange_cosets_row_shards_device(uint32_t k, uint64_t usable_rows, const uint64_t omega[4], const uint64_t ext_omega[4], const uint64_t zeta[4],
                                            zkhip_row_shards *set, uint32_t col0, void *stream);
/* out[row] = sum_p weights[p] * progs[p](row): `n_progs` independent row programs over the same columns, run side by side in one launch
 * (one grid row per program) and combined with zkhip_fr_linear_combination_device's kernel.  Programs that read ZKHIP_SRC_ROWPOW must
 * name the same omega.  For programs that are
 * long and run over few rows: the quotient numerator of a circuit with hundreds of columns at 2^13 .. 2^15 rows (the reference's voter and
 * state-transition shapes) is thousands of instructions, and one program there is a handful of wavefronts walking the whole list.  The
 * y-fold of `evaluate_h` is linear in its terms, h = sum_i term_i y^(T-1-i), so a host cuts the term list into consecutive runs, folds each
 * into a program of its own and passes weights[p] = y^(number of terms after run p) (zksnap_circuits_halo2_amd/evaluation.py
 * `evaluate_h_parts`).  `weights`: n_progs x 4 words.  ZKHIP_SRC_PREV reads 0 in every program (there is no previous value). */
int zkhip_fr_eval_rows_sum_device(const zkhip_vm_program *progs, const uint64_t *weights, uint32_t n_progs, const void *const *d_columns, uint32_t n_columns,
                                  uint32_t log_rows, void *d_out, void *stream);
/* out[j] = a[index_a[j]] * b[index_b[j]] (u32 indices, device-resident): the inner loop of `permutation::keygen::Assembly::build_pk`
 * [DEP halo2-axiom plonk/permutation/keygen.rs; keygen_pk at /root/reference/aggregator/src/wrapper.rs:108] -- sigma_i[j] =
 * delta^(column the cell (i, j) maps to) * omega^(its row) -- so that the sigma columns of a proving key are built in HBM.  Indices
 * must be below the table lengths (they are reduced modulo the length rather than trusted: no fault on a bad index). */
int zkhip_fr_gather_mul_device(const void *d_a, size_t a_len, const void *d_index_a, const void *d_b, size_t b_len, const void *d_index_b, size_t n,
                               void *d_out, void *stream);
/* grand product of the permutation / lookup arguments [DEP plonk/permutation/prover.rs, plonk/lookup/prover.rs]:
 * z[0] = 1, z[i+1] = z[i] * num[i] / den[i] for i < n - 1  (zero denominators count as zero, like BatchInvert).
 * num is preserved, den is overwritten (inverted in place), z may alias num. */
int zkhip_fr_grand_product(const uint64_t *num, const uint64_t *den, size_t n, uint64_t *z);
int zkhip_fr_grand_product_device(const void *d_num, void *d_den, size_t n, void *d_z, void *stream);
/* out[i] = sum_j coeffs[j] * d_cols[j][i] for i < n: the y- / v-combinations and L(X) of the multi-open provers over `count` device-resident
 * polynomials ([DEP] poly/kzg/multiopen/shplonk/prover.rs; hundreds of polynomials at the voter / state-transition column counts).  The
 * columns are cut into groups that run side by side, two products under one reduction, so the call does not degrade into `count`
 * dependent multiply-adds per row the way the same sum written as a row program does on few rows.  `d_cols` and `coeffs` (count x 4
 * words, Montgomery) are host arrays; d_out may be one of the columns.  count = 0 gives zeros. */
int zkhip_fr_linear_combination_device(const void *const *d_cols, const uint64_t *coeffs, size_t count, size_t n, void *d_out, void *stream);
/* The KZG multi-open provers for a host that keeps its polynomials as device addresses (a Rust host's handles: rust-shim/prover_patch.rs):
 * `ProverGWC::create_proof` (the reference's gen_snark path, /root/reference/aggregator/src/wrapper.rs:59-60, 127-137) and
 * `ProverSHPLONK::create_proof` (the benches' gen_proof path, /root/reference/aggregator/benches/wrapper_circuit.rs:140)
 * [DEP halo2-axiom poly/kzg/multiopen/{gwc, shplonk}/prover.rs].  A query opens the polynomial of 2^k coefficients at `d_poly` at
 * `point`; `eval` is its value there when `has_eval` is non-zero (the prover has computed and written it to the transcript already:
 * zkhip_fr_eval_polynomial_batch_device), otherwise the library evaluates.  Polynomials are told apart by their addresses.  `bases` is a
 * base array registered with zkhip_register_bases (`ParamsKZG::g`): the commitments are MSMs against its first 2^k points.  The
 * transcript stays with the host: challenges come in, commitments (Jacobian, 12 words each) go out.
 *   GWC      one witness commitment per distinct point, in the order the points first appear among the queries; `capacity` is the room
 *            of `out_points` in points, `*n_out` the number there are (ZKHIP_EINVAL if that is more than `capacity`).
 *   SHPLONK  `begin` (y and v squeezed) returns H = commit(h(X)) and a state; the host writes H, squeezes u; `finish` returns H' and
 *            releases the state whatever it returns (ZKHIP_EINVAL when an evaluation does not belong to its polynomial: the reference's
 *            L(u) = 0 debug assertion).  The polynomials must stay alive and unchanged in between.  `abort` releases a state unused. */
typedef struct zkhip_prover_query {
  uint64_t point[4];
  const void *d_poly;
  uint64_t eval[4];
  uint32_t has_eval;
  uint32_t reserved;
} zkhip_prover_query;   /* 80 bytes */
typedef struct zkhip_shplonk zkhip_shplonk;
int zkhip_multiopen_gwc_device(const uint64_t *bases, uint32_t k, const zkhip_prover_query *queries, size_t n_queries, const uint64_t v[4],
                               uint64_t *out_points, size_t capacity, size_t *n_out);
int zkhip_multiopen_shplonk_begin_device(const uint64_t *bases, uint32_t k, const zkhip_prover_query *queries, size_t n_queries, const uint64_t y[4],
                                         const uint64_t v[4], uint64_t out_h[12], zkhip_shplonk **state);
int zkhip_multiopen_shplonk_finish_device(zkhip_shplonk *state, const uint64_t u[4], uint64_t out_hp[12]);
int zkhip_multiopen_shplonk_abort(zkhip_shplonk *state);
/* The permutation argument's grand products, every set in one call: [DEP] halo2-axiom plonk/permutation/prover.rs `Argument::commit`
 * (the loop over `columns.chunks(chunk_len)`; reached from create_proof, /root/reference/aggregator/src/wrapper.rs:129).  `values[c]` / `sigmas[c]`
 * are the Lagrange values of permutation column c and of its sigma polynomial (2^log_n rows each); set s holds columns
 * [s chunk_len, min((s + 1) chunk_len, n_columns)); `usable_rows` = n - (blinding_factors + 1), `delta` = Fr::DELTA, `omega` the domain's
 * generator.  z is [ceil(n_columns / chunk_len)][2^log_n], dense:
 *     z_0[0] = 1,  z_s[0] = z_(s-1)[usable_rows],  z_s[i + 1] = z_s[i] prod_j (v_j[i] + beta delta^c omega^i + gamma) / (v_j[i] + beta sigma_j[i] + gamma)
 * for i < usable_rows; the rows after usable_rows repeat z_s[usable_rows] (the caller overwrites them with its blinding scalars, as the
 * reference does).  With usable_rows = 2^log_n there is no row z_(s-1)[usable_rows]: a later set then starts from the product over all 2^log_n
 * rows of the earlier sets.  Zero denominators count as zero, like BatchInvert.  A handful of launches whatever the number of sets: the chained
 * products of all sets are one prefix product over the [sets][n] array. */
int zkhip_permutation_products(const uint64_t *const *values, const uint64_t *const *sigmas, uint32_t n_columns, uint32_t chunk_len, uint32_t log_n,
                               size_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4], const uint64_t omega[4],
                               uint64_t *z);
int zkhip_permutation_products_device(const void *const *d_values, const void *const *d_sigmas, uint32_t n_columns, uint32_t chunk_len, uint32_t log_n,
                                      size_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4],
                                      const uint64_t omega[4], void *d_z, void *stream);

/* `permute_expression_pair` of the lookup argument [DEP plonk/lookup/prover.rs]: the first `usable_rows` rows of `input` sorted by
 * canonical value into permuted_input; permuted_table holds, at the first row of every run of equal input values, that value, and at
 * the other rows the table values not consumed this way, ascending, handed out from the last such row backwards (the reference's
 * BTreeMap iteration + Vec::pop).  Rows >= usable_rows of the outputs (the blinding rows) are not written.  ZKHIP_EINVAL when an
 * input value does not occur in the table (the reference's Error::ConstraintSystemFailure).  Outputs must not alias the inputs. */
int zkhip_lookup_permute(const uint64_t *input, const uint64_t *table, size_t usable_rows, uint64_t *permuted_input, uint64_t *permuted_table);
int zkhip_lookup_permute_device(const void *d_input, const void *d_table, size_t usable_rows, void *d_permuted_input, void *d_permuted_table,
                                void *stream);
/* The lookup argument of EVERY lookup of a circuit, one call per transcript phase (A' and S' are committed before beta and gamma exist).  The
 * launches of a call do not grow with n_lookups, and the call waits for the stream once, for its status.
 * permute_expression_pair of n_lookups lookups at once. d_inputs[l] / d_tables[l]: the compressed input / table expression of lookup l
 * (device, >= usable_rows elements; equal table addresses are one table and are sorted once). d_permuted_inputs / d_permuted_tables:
 * [n_lookups][2^log_n] dense; rows < usable_rows of every column are written, rows >= usable_rows are not touched.  An input value missing
 * from its table: ZKHIP_EINVAL, zkhip_last_error names the lowest failing lookup index and the outputs are unspecified.  n_lookups == 0 or
 * usable_rows == 0: ZKHIP_OK, nothing written. */
int zkhip_lookup_permute_many_device(const void *const *d_inputs, const void *const *d_tables, uint32_t n_lookups, uint32_t log_n, size_t usable_rows,
                                     void *d_permuted_inputs, void *d_permuted_tables, void *stream);
/* z[l][0] = 1, z[l][i+1] = z[l][i] (a_l[i] + beta)(s_l[i] + gamma) / ((a'_l[i] + beta)(s'_l[i] + gamma)) for i < usable_rows; the rows after
 * usable_rows repeat z[l][usable_rows] (the caller overwrites them, as with zkhip_permutation_products). Zero denominators count as zero.
 * d_permuted_inputs / d_permuted_tables / d_z: [n_lookups][2^log_n] dense; rows >= usable_rows of the permuted columns are not read.
 * n_lookups == 0 or usable_rows == 0: ZKHIP_OK, nothing written. */
int zkhip_lookup_products_device(const void *const *d_inputs, const void *const *d_tables, const void *d_permuted_inputs, const void *d_permuted_tables,
                                 uint32_t n_lookups, uint32_t log_n, size_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], void *d_z,
                                 void *stream);

/* ---- witness checks: does this witness satisfy its circuit, and if not, where (MockProver) -----------------------------------------
 * The reference never proves an unchecked witness: `gen_proof` runs `MockProver::run(k, &circuit, instances).assert_satisfied()` first
 * (/root/reference/aggregator/src/wrapper.rs:117-123).  These three calls answer the same three questions -- every gate polynomial is zero
 * on every usable row, every copy constraint holds, every lookup input occurs in its table -- as read-only passes over columns that are
 * already in HBM for the proof.  Each question is reduced on the device to one record per item list:
 *   failures  the number of failing items
 *   first     the lowest failing index, UINT64_MAX when there is none
 * a count and a minimum, so both are exact and do not depend on the launch geometry.  All three calls are asynchronous on `stream`,
 * initialise their records themselves, read their columns only, wait for nothing on the host and return ZKHIP_OK when the check RAN,
 * whatever it found: the caller reads the records back (zkhip_stream_sync + zkhip_download).  A satisfied witness costs no atomic.
 * Argument errors are ZKHIP_EINVAL with nothing enqueued and the records untouched.  Records are 8-byte aligned device memory.
 * Not covered: halo2's unassigned-cell (`Poison`) diagnostics, selector / region bookkeeping, row-shard sets, devices other than the stream's. */
typedef struct zkhip_check_report { uint64_t failures; uint64_t first; } zkhip_check_report;   /* 16 bytes */
/* Gates.  `n_progs` row programs (1 .. 65535), one per gate polynomial, rot_scale = 1, over the same whole-domain columns (2^log_rows
 * elements each), side by side in ONE launch of the interpreter (one grid row per program; never the run-time compiler).  d_reports[p]
 * counts the rows r in [row0, row0 + count) where program p's result is not zero; `first` is the lowest such row of the domain.  Rotations
 * wrap modulo 2^log_rows as in the evaluator, ZKHIP_SRC_PREV reads 0, ZKHIP_SRC_ROWPOW is omega^r (programs that read it name one omega).
 * ZKHIP_EINVAL: count == 0, row0 + count > 2^log_rows, n_progs == 0 or > 65535, a null pointer, a program zkhip_fr_eval_rows_device rejects. */
int zkhip_check_rows_device(const zkhip_vm_program *progs, uint32_t n_progs, const void *const *d_columns, uint32_t n_columns,
                            uint32_t log_rows, uint64_t row0, uint64_t count, void *d_reports, void *stream);
/* Copy constraints.  d_map_col / d_map_row: [n_columns][2^log_n] u32 each (device), the permutation as `Assembly` keeps it: cell (c, r)
 * maps to cell (map_col[c][r], map_row[c][r]).  A cell fails when its 32 bytes differ from those of the cell it maps to; item index
 * c 2^log_n + r.  Map entries are reduced modulo n_columns / 2^log_n, not trusted (as in zkhip_fr_gather_mul_device).  One record.
 * ZKHIP_EINVAL: n_columns == 0 or > 4096, log_n > 28, n_columns 2^log_n >= 2^39, a null pointer. */
int zkhip_check_copies_device(const void *const *d_columns, uint32_t n_columns, uint32_t log_n, const void *d_map_col, const void *d_map_row,
                              void *d_report, void *stream);
/* Lookup membership, arguments as zkhip_lookup_permute_many_device: compressed input / table columns, equal table addresses are one table
 * and are sorted once, only rows < usable_rows of either side count.  Row i of lookup l fails when input_l[i] equals no table_l[j],
 * j < usable_rows; d_reports[l].  n_lookups == 0 or usable_rows == 0: ZKHIP_OK, the n_lookups records say "no failure".
 * ZKHIP_EINVAL: n_lookups > 1365, log_n > 28, usable_rows > 2^log_n, a null pointer. */
int zkhip_check_lookups_device(const void *const *d_inputs, const void *const *d_tables, uint32_t n_lookups, uint32_t log_n,
                               size_t usable_rows, void *d_reports, void *stream);

/* ---- random field elements: blinding rows and the vanishing argument's random polynomial, drawn in HBM ---------------------------
 * A cryptographic, reproducible stream of Fr elements addressed by index.  THE STREAM (normative): element i of stream (seed, stream_id) is
 *   1. one ChaCha20 block of 20 rounds in the original layout with a 64-bit block counter: words 0..3 are "expand 32-byte k" (0x61707865,
 *      0x3320646e, 0x79622d32, 0x6b206574); words 4..11 are the 32 seed bytes as little-endian u32; word 12 is the low half of i, word 13
 *      its high half; word 14 is the low half of stream_id, word 15 its high half;
 *   2. its 64 output bytes (the 16 output words, little-endian, word 0 first) read as a little-endian 512-bit integer;
 *   3. that integer mod r,
 * stored in the external format (4 x u64 Montgomery-256, canonical).  One block gives exactly one element, so an element depends on (seed,
 * stream_id, i) alone: every launch geometry, every split of a range into calls and every device produce the same column, and a host can
 * restate it.  (Design intent, not pinned by any test: the i-th `Fr::random` of a `ChaCha20Rng::from_seed(seed)` after `set_stream(stream_id)`.)
 * Pin: seed bytes 00 01 .. 1f, stream_id 0x4a000000, i = 0x0900000000000001 is the block of RFC 8439 section 2.3.2; its element is
 * 0x099d737c79bea952e4c9671a82baa6de853af4f7694e36c4e5577d4ae6d300c5, stored as the 256-bit number
 * 0x25312d9be543d4c7a1d921e13f01589a414c389165c4cad2b5e970bf8f628f64.
 * CONTRACT: the library holds no entropy -- the caller draws the seed from its own generator; blinding is exactly as secret as the seed; a
 * (seed, stream_id, index) triple is never reused across proofs.
 * zkhip_fr_random_device writes elements first .. first + n - 1 to d_out.  zkhip_fr_random is its host-buffer form.
 * zkhip_fr_random_rows_device writes element first + c * count + j to row row0 + j of column c (d_cols: host array of n_cols device pointers,
 * every column holding at least row0 + count elements) in one launch whatever n_cols is, and touches no other row: the blinding tails of all
 * columns of a phase in one call.  n_cols * count is at most 2^30.
 * Both `_device` forms are asynchronous on `stream`; the seed and the pointer array are consumed before the call returns.  n == 0, n_cols == 0
 * and count == 0 are ZKHIP_OK and do nothing.  ZKHIP_EINVAL with nothing written: a null pointer (a null column included), first + the number
 * of elements above 2^64, more than 2^30 elements in the rows form. */
int zkhip_fr_random_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, size_t n, void *d_out, void *stream);
int zkhip_fr_random(const uint8_t seed[32], uint64_t stream_id, uint64_t first, size_t n, uint64_t *out);
int zkhip_fr_random_rows_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, const void *const *d_cols,
                                uint32_t n_cols, size_t row0, size_t count, void *stream);

/* ---- device buffers for a host that does not link HIP itself (handles instead of host slices) ---- */
/* The `_device` entry points below take HIP device pointers so that polynomials stay in HBM from iNTT through commit, extended
 * NTT, quotient and back (PCIe is 8x slower than the NTT kernel: DESIGN.md section 5).  A Rust / C host obtains such pointers
 * here.  Copies run on HIP's default stream (the one the `_device` entry points use when `stream` is NULL) and block:
 * zkhip_download returns when the data is in `dst`, zkhip_upload when `src` may be reused. */
int zkhip_alloc(size_t bytes, void **d_ptr);
int zkhip_free(void *d_ptr);
int zkhip_upload(void *d_dst, const void *src, size_t bytes);
int zkhip_download(void *dst, const void *d_src, size_t bytes);
/* wait for everything this process has queued on the device */
int zkhip_sync(void);
/* wait for the work queued on one stream.  zkhip_upload / zkhip_download are blocking copies on HIP's legacy default stream: a stream
 * created with hipStreamNonBlocking (every library-owned stream, every torch side stream) is NOT ordered against them, so a host that
 * enqueues `_device` calls on such a stream calls this before it reads their results back. */
int zkhip_stream_sync(void *stream);

/* ---- device-resident variants (pointers are HIP device pointers; stream is a hipStream_t; NULL = HIP's default stream 0, ordered
 * with the caller's other default-stream work -- e.g. what torch.cuda.current_stream().cuda_stream is when no stream was set) --- */
/* Used by the pipeline / bench so that polynomials and scalars stay in HBM between calls. */
int zkhip_msm_g1_device(const void *d_scalars, const void *d_bases, size_t n, void *d_out_xyz, void *stream);
int zkhip_msm_g2_device(const void *d_scalars, const void *d_bases, size_t n, void *d_out_xyz, void *stream);
/* prepared (fixed-base) path for device-resident bases: the handle owns the table until released */
int zkhip_prepare_bases_device(const void *d_bases, size_t n, uint64_t *handle);
/* same with an explicit window size (2..20; 0 = automatic) -- experiments and tests of the wide-window path */
int zkhip_prepare_bases_device_c(const void *d_bases, size_t n, int window_bits, uint64_t *handle);
int zkhip_release_bases(uint64_t handle);
/* window size (bits) the handle's table was built for; <= 0 for an unknown handle */
int zkhip_prepared_window_bits(uint64_t handle);
int zkhip_msm_g1_prepared_device(uint64_t handle, size_t offset, const void *d_scalars, size_t n, void *d_out_xyz, void *stream);
/* Device-resident scalars against an array pinned with zkhip_register_bases: `bases` is the HOST pointer the caller would pass to
 * zkhip_msm_g1 (any sub-range of a registered array), the scalars and the result live in HBM.  This is `params.commit(&poly)` for a
 * polynomial that never left the device, against the same tables the host-buffer calls use.  A range that spans several shards (several
 * devices named in zkhip_init, or virtual shards) fans out like the host-buffer call: every secondary device pulls its slice of the scalars
 * from the primary device's HBM (peer copy over xGMI), runs its shard on a stream of its own and returns its 96-byte partial; the fold runs
 * on `stream`, which is the only stream the caller has to wait for (SURVEY.md section 8(e) with the scalars resident in HBM).
 * ZKHIP_EINVAL when the range is not inside a registered array. */
int zkhip_msm_g1_registered_device(const uint64_t *bases, const void *d_scalars, size_t n, void *d_out_xyz, void *stream);
/* `batch` device-resident scalar vectors (vector k at d_scalars + k * scalar_stride elements) against the same registered range, e.g. all
 * advice columns of a circuit; d_out_xyz: batch Jacobian results.  Vectors share launch sets per shard when the shard's table has
 * windows of <= 16 bits. */
int zkhip_msm_g1_registered_batch_device(const uint64_t *bases, const void *d_scalars, size_t n, size_t batch, size_t scalar_stride, void *d_out_xyz,
                                         void *stream);
/* `batch` scalar vectors (vector k at d_scalars + k * scalar_stride elements) against the same prepared bases in one launch
 * set -- e.g. all advice columns of a circuit: small MSMs (k = 13..17) then run at large-MSM throughput.  d_out_xyz: batch
 * Jacobian results, 96 bytes each.  Tables with wide windows (n >= 2^20) do not share a launch set; their vectors run alternately
 * on `stream` and on a high-priority stream the library owns (forked from and joined to `stream` with events), so that one MSM's
 * latency-bound sort and reduction tail run under the next one's accumulation: all results are complete once `stream` has
 * drained, as for any other `_device` call. */
int zkhip_msm_g1_prepared_batch_device(uint64_t handle, size_t offset, const void *d_scalars, size_t n, size_t batch, size_t scalar_stride,
                                       void *d_out_xyz, void *stream);
/* window-size override for experiments (0 = automatic) */
int zkhip_msm_g1_device_c(const void *d_scalars, const void *d_bases, size_t n, void *d_out_xyz, int window_bits, void *stream);
int zkhip_ntt_fr_device(void *d_a, const uint64_t omega[4], uint32_t log_n, void *stream);
int zkhip_ifft_scaled_device(void *d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], void *stream);
int zkhip_mul_periodic_device(void *d_a, size_t n, const void *d_table, uint32_t period, void *stream);
/* coset transforms on device-resident polynomials, `batch` of them per launch set (polynomial b at base + b * stride elements;
 * d_out must not overlap d_a).  coeff_to_extended reads 2^k coefficients and writes 2^ext_k evaluations per polynomial;
 * extended_to_coeff reads 2^ext_k evaluations and writes out_len coefficients per polynomial. */
int zkhip_coeff_to_extended_device(const void *d_a, size_t a_stride, uint32_t k, void *d_out, size_t out_stride, uint32_t ext_k, uint32_t batch,
                                   const uint64_t ext_omega[4], const uint64_t zeta[4], void *stream);
int zkhip_extended_to_coeff_device(const void *d_a, size_t a_stride, uint32_t ext_k, const uint64_t ext_omega_inv[4], const uint64_t ext_divisor[4],
                                   const uint64_t zeta[4], void *d_out, size_t out_stride, size_t out_len, uint32_t batch, void *stream);
/* `batch` polynomials of 2^log_n elements, polynomial b at d_a + b * stride elements (stride >= 2^log_n), one launch set:
 * many small transforms (voter / state-transition columns at k = 13..17) run at large-transform throughput */
int zkhip_ntt_fr_batch_device(void *d_a, const uint64_t omega[4], uint32_t log_n, uint32_t batch, size_t stride, void *stream);
int zkhip_ifft_scaled_batch_device(void *d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], uint32_t batch,
                                   size_t stride, void *stream);
/* out = sum of m Jacobian points (multi-GPU: fold of the gathered per-rank partial sums) */
int zkhip_g1_sum_device(const void *d_points_xyz, int m, void *d_out_xyz, void *stream);
int zkhip_g1_sum(const uint64_t *points_xyz, int m, uint64_t out_xyz[12]);
int zkhip_msm_window_bits(size_t n);

/* ---- synthetic inputs + per-phase timing (bench / large tests) ------------------------------------- */
/* d_out[i] = (t0 + i*d) * G as G1Affine, i < n, written to device memory: a seeded stand-in for an SRS whose
 * discrete logs are known, so MSM(a, out) = [sum a_i (t0 + i d)] G can be checked with one scalar multiplication.
 * t0, d: Fr in the usual Montgomery memory format. */
int zkhip_g1_gen_walk_device(const uint64_t t0[4], const uint64_t d[4], size_t n, void *d_out, void *stream);
/* `ParamsKZG::setup` [DEP poly/kzg/commitment.rs] building block: d_out[i] = scalars[i] * G as
 * G1Affine for the BN254 generator G = (1, 2), i < n -- g = [s^i] G and g_lagrange = [L_i(s)] G are two such calls on scalar vectors
 * the Fr primitives above produce on the device.  The first call builds a 32 MiB table of generator multiples. */
int zkhip_g1_fixed_base_mul_device(const void *d_scalars, size_t n, void *d_out, void *stream);
/* `best_fft::<G1>(a, omega, log_n)` [DEP arithmetic.rs: the FftGroup instance for curve points]: in place on 2^log_n Jacobian points
 * (96 B each, the memory of `G1`), natural order in and out, a[i] <- sum_j omega^(i j) a[j]; omega: Fr in Montgomery form.
 * Each butterfly holds one 254-bit scalar multiplication: ~1 s at log_n = 22.  log_n <= 26. */
int zkhip_g1_fft_device(void *d_points_xyz, const uint64_t omega[4], uint32_t log_n, void *stream);
/* `g_to_lagrange(g, k)` [DEP poly/kzg/commitment.rs, used by ParamsKZG::setup / from_parts for an SRS whose trapdoor is not known]:
 * d_g_lagrange[i] = (1/n) sum_j omega_k^(-i j) d_g[j], both arrays 2^k G1Affine points (64 B); may not alias. */
int zkhip_g_to_lagrange_device(const void *d_g, uint32_t k, void *d_g_lagrange, void *stream);
/* host-buffer form with the memory of the reference's function: g_xyz = 2^k Jacobian points (`Vec<G1>`, 12 limbs each), g_lagrange = 2^k affine
 * points (`Vec<G1Affine>`, 8 limbs each); the inverse FFT over the points, the 1/n scaling and the batch normalisation in one call */
int zkhip_g_to_lagrange(const uint64_t *g_xyz, uint32_t k, uint64_t *g_lagrange);
/* `Curve::batch_normalize` [DEP group / halo2curves; create_proof normalises its commitments before they enter the transcript, and
 * keygen stores `to_affine()` of the fixed / permutation commitments in the verifying key]: n Jacobian points (12 limbs each) -> n
 * affine points (8 limbs each, canonical Montgomery limbs; the identity becomes (0, 0)). */
int zkhip_g1_batch_normalize(const uint64_t *points_xyz, size_t n, uint64_t *out_affine);
int zkhip_g1_batch_normalize_device(const void *d_points_xyz, size_t n, void *d_out_affine, void *stream);
/* `G1Affine::read_raw`'s validity check [DEP halo2curves; run on every point by the SerdeFormat::RawBytes readers of SRS and key files:
 * ParamsKZG::read, VerifyingKey::read]: coordinates canonical Montgomery residues and (x, y) = (0, 0) or y^2 = x^3 + 3.  *first_bad =
 * index of the first point that fails, n when all pass (the XYZZ formulas never use b, so an off-curve point would otherwise give
 * garbage commitments without any error). */
int zkhip_g1_check_points(const uint64_t *points, size_t n, uint64_t *first_bad);
int zkhip_g1_check_points_device(const void *d_points, size_t n, uint64_t *first_bad, void *stream);
/* `GroupEncoding::{to_bytes, from_bytes}` of G1Affine [DEP halo2curves derive/curve.rs], one call per point in the reference's
 * `SerdeFormat::Processed` writers / readers (ParamsKZG::{write_custom, read_custom}, VerifyingKey / ProvingKey::{write, read}); the
 * reference itself writes RawBytesUnchecked (/root/reference/aggregator/src/wrapper.rs:971-988).  32 bytes per point: x canonical
 * little-endian plus flags in the last byte.  flag_layout 0 (halo2curves >= 0.3.2): bit 6 = lsb of canonical y, bit 7 = identity;
 * flag_layout 1 (earlier releases): bit 7 = lsb of canonical y, identity = 32 zero bytes.  Decompression is y = (x^3 + 3)^((q+1)/4)
 * per point, strict: *first_bad = index of the first encoding that is not canonical / not on the curve (its output point is (0, 0)),
 * n when all decode. */
int zkhip_g1_compress(const uint64_t *points, size_t n, uint8_t *out32, int flag_layout);
int zkhip_g1_compress_device(const void *d_points, size_t n, void *d_out32, int flag_layout, void *stream);
int zkhip_g1_decompress(const uint8_t *in32, size_t n, uint64_t *points, int flag_layout, uint64_t *first_bad);
int zkhip_g1_decompress_device(const void *d_in32, size_t n, void *d_points, int flag_layout, uint64_t *first_bad, void *stream);
/* ---- transcript: halo2's `Blake2bWrite` / `Blake2bRead` with `Challenge255` -- a proof written and read as bytes ------------------------
 * [DEP halo2-axiom transcript.rs; the benches prove with create_proof(SHPLONK, Blake2b): halo2-base `gen_proof`,
 * /root/reference/aggregator/benches/wrapper_circuit.rs:140.]  Restated from the published format, unpinned like everything at this boundary.
 * THE FORMAT (normative):
 *   state          Blake2b-512 (RFC 7693), no key, personalisation "Halo2-Transcript" (16 bytes), plus the proof byte stream: grown by a
 *                  writer, walked by a reader's cursor.
 *   common_point   absorb the byte 0x01, then x and y as 32-byte little-endian canonical integers.  The identity is ZKHIP_EINVAL (halo2:
 *                  "cannot write points at infinity to the transcript") and leaves the transcript untouched.
 *   common_scalar  absorb the byte 0x02, then the 32-byte little-endian canonical scalar.
 *   write_*        the common_* call, then 32 bytes appended to the proof: the point's GroupEncoding exactly as zkhip_g1_compress writes it
 *                  (flag_layout is fixed when the transcript is made) or the scalar's canonical repr.
 *   read_*         32 bytes from the proof, decoded STRICTLY, then the common_* call.  ZKHIP_EINVAL: x not canonical, x^3 + 3 not a square,
 *                  an identity encoding, a scalar >= r, fewer than 32 n bytes left.  zkhip_last_error() names the index of the first bad
 *                  element; the hash state and the cursor are as before the call.
 *   squeeze        absorb the byte 0x00; finalise A COPY of the state to 64 bytes (the running state goes on, the 0x00 included); the
 *                  challenge is those 64 bytes as a little-endian 512-bit integer mod r (`from_uniform_bytes`), returned as 4 Montgomery
 *                  words like every other Fr here.
 * Pin: the first squeeze of a fresh transcript is 0x0e89c2c9ef365f095ec7aa36500bb0ba58bf7d5e17194055afb5a1c746f1786a (canonical).
 * Batches: a call over n elements is n calls over one, in order; a failing call absorbs and appends NOTHING (all n are checked first).
 * Where things run.  The hash runs on the host, inside the library (a serial chain of 128-byte blocks).  The calls marked "host" touch no
 * GPU and work in a process that never initialises HIP: Montgomery <-> canonical and the 512-bit reduction are host arithmetic.  The
 * `_device` calls take what the prover has in HBM: write_points_device takes n Jacobian commitments exactly as the MSM calls leave them (12
 * words each) and costs ONE launch (shared inversion of the z's, canonical x and y, the encoding: 96 bytes per point) behind a 4-byte upload that
 * clears the call's identity count, one copy into a pinned block the transcript owns and one wait on `stream`; write_scalars_device the same for n Montgomery Fr (e.g. the buffer
 * zkhip_fr_eval_polynomial_batch_device filled).  read_points_device uploads n encodings, decompresses them (zkhip_g1_decompress's kernel)
 * and leaves the n affine Montgomery points (8 words each) at d_affine for the verifier's MSMs.  The forms without `_device` take / fill host
 * buffers and borrow a lane like every host-buffer call.  Device pointers must be 16-byte aligned.  After a failed `_device` call nothing of
 * it is left queued on `stream`.
 * A transcript object is used by one thread at a time; different objects may be used concurrently: no library lock is held while a call
 * waits for its stream or hashes.  A writer refuses read_*, a reader
 * refuses write_*; common_* and squeeze work on both. */
typedef struct zkhip_transcript zkhip_transcript;
zkhip_transcript *zkhip_transcript_new(int flag_layout);                                                /* a writer; NULL on a bad layout */
zkhip_transcript *zkhip_transcript_new_reader(const uint8_t *proof, size_t len, int flag_layout);       /* the bytes are copied */
void zkhip_transcript_free(zkhip_transcript *t);
int zkhip_transcript_common_scalars(zkhip_transcript *t, const uint64_t *fr_mont, size_t n);            /* host */
int zkhip_transcript_common_points(zkhip_transcript *t, const uint64_t *affine_mont, size_t n);         /* host; 8 words per point */
int zkhip_transcript_squeeze(zkhip_transcript *t, uint64_t out_fr_mont[4]);                             /* host */
int zkhip_transcript_write_scalars(zkhip_transcript *t, const uint64_t *fr_mont, size_t n);             /* host */
int zkhip_transcript_write_points_device(zkhip_transcript *t, const void *d_points_xyz, size_t n, void *stream);
int zkhip_transcript_write_scalars_device(zkhip_transcript *t, const void *d_fr, size_t n, void *stream);
int zkhip_transcript_write_points(zkhip_transcript *t, const uint64_t *points_xyz, size_t n);           /* host buffer: upload, then the device form */
int zkhip_transcript_read_scalars(zkhip_transcript *t, size_t n, uint64_t *fr_mont);                    /* host */
int zkhip_transcript_read_points_device(zkhip_transcript *t, size_t n, void *d_affine, void *stream);
int zkhip_transcript_read_points(zkhip_transcript *t, size_t n, uint64_t *affine_mont);                 /* host buffer */
/* the proof: everything written so far (a writer) or the bytes given (a reader).  *len = its length; buf may be NULL to ask for the length,
 * otherwise cap must be at least that (ZKHIP_EINVAL, *len still set). */
int zkhip_transcript_proof(const zkhip_transcript *t, uint8_t *buf, size_t cap, size_t *len);
/* The same object over the Poseidon sponge of the section "Poseidon" below: snark-verifier's halo2 `PoseidonTranscript<G1Affine, NativeLoader, _>`,
 * the transcript of the reference's `gen_snark` (/root/reference/aggregator/src/wrapper.rs:111-158).  Every zkhip_transcript_* call above works on
 * it and dispatches on the object's hash; what differs (normative):
 *   no prefix bytes anywhere.
 *   common_scalar  appends the scalar to the sponge's buffer.
 *   common_point   appends x mod r, then y mod r: the canonical Fq coordinates read as integers (q < 2 r: one conditional subtraction).  The
 *                  identity is ZKHIP_EINVAL and leaves the transcript untouched.
 *   squeeze        the sponge's squeeze; the challenge is that full Fr value.
 *   write_*        the common_* call, then the SAME 32 bytes the Blake2b transcript appends: a proof's bytes do not depend on the hash, only
 *                  its challenges do.  read_*: the same strict decoding, then the common_* call.  Atomicity and batches as above.
 * The `_device` calls launch the same kernels and move the same 96 / 32 / 64-byte records; only what the host does with a record differs.
 * The chain of permutations is serial and runs on the host inside the library: one permutation, 13 microseconds, per two absorbed elements
 * (profiles/r15_poseidon.txt).  Pins: the first squeeze of a fresh Poseidon transcript is the fresh-sponge pin below; after common_point((1, 2))
 * it is hash(1, 2). */
zkhip_transcript *zkhip_transcript_new_poseidon(int flag_layout);                                       /* a writer; NULL on a bad layout */
zkhip_transcript *zkhip_transcript_new_poseidon_reader(const uint8_t *proof, size_t len, int flag_layout);
/* Per-phase timing with HIP events on the stream the kernels run on.  enable(1), run one call, then
 * zkhip_profile_read synchronises and returns the number of phases of the last profiled call, writing up to
 * `max` durations (milliseconds) and names (63 chars + NUL each). */
int zkhip_profile_enable(int on);
int zkhip_profile_read(double *ms, char (*names)[64], int max);
/* enable(2): every following call APPENDS its phases (no read-back between calls: a loop of calls runs back to back as it does
 * unprofiled); zkhip_profile_read_calls then synchronises and returns all recorded phases in call order, call_of[i] = index of the
 * call phase i belongs to.  The pool holds 2048 events (about 100 MSM calls); calls beyond it record nothing. */
int zkhip_profile_read_calls(double *ms, char (*names)[64], int *call_of, int max);

/* ---- Poseidon over Fr: T = 3, RATE = 2, R_F = 8, R_P = 57, x^5 (`SECURE_MDS = 0`) -- Merkle trees and the sponge of the Poseidon transcript ----
 * [DEP pse_poseidon / snark-verifier `hash::Poseidon`; the reference's trees: /root/reference/voter/src/merkletree/native.rs:30-49, its
 * `gen_snark` transcript: aggregator/src/wrapper.rs:111-158.]  Restated from the Poseidon paper.  The PERMUTATION is pinned by the published
 * `poseidonperm_x5_254_3` vector and circomlib's poseidon([1, 2]); the FRAMING (sponge, tree, transcript) is pinned only as these lines word
 * it, not against the crates: its parity with them is unpinned like the rest of this boundary.
 * THE DEFINITION (normative):
 *   Grain        an 80-bit state, initialised most-significant bit first from: field = 1 (2 bits), sbox = 0 (4), n = 254 (12), t = 3 (12),
 *                R_F = 8 (10), R_P = 57 (10), thirty 1 bits.  A step: new = b62 ^ b51 ^ b38 ^ b23 ^ b13 ^ b0; b0 leaves, `new` is appended.
 *                The first 160 new bits are discarded.  Output bits come from PAIRS of new bits: first = 1 emits the second, else nothing.
 *   constants    round constants: (R_F + R_P) T = 195 elements in round order, then word order; each is 254 output bits as a big-endian
 *                integer, redrawn while it is >= r.  Then 2 T more elements, 254 bits each reduced mod r WITHOUT rejection: xs the first T,
 *                ys the next T, M[i][j] = (xs[i] + ys[j])^-1.  The library runs Grain itself, once per process; nothing is a pasted table.
 *   permutation  65 rounds, each: add the round's three constants; x^5 on all three words in rounds 0-3 and 61-64, on word 0 only in
 *                rounds 4-60; state'[i] = sum_j M[i][j] state[j].
 *   sponge       a fresh state is (2^64, 0, 0) with an empty buffer; update appends to the buffer; squeeze takes the buffer and (1) for each
 *                full chunk of 2 adds the chunk into words 1 and 2 and permutes, (2) adds the remaining 0 or 1 elements followed by a single
 *                1 into words 1.. and permutes, (3) returns word 1.  The state carries on after a squeeze; the buffer is empty.
 *   hash         a fresh sponge, one update, one squeeze.
 *   Merkle tree  a power of two of leaves >= 1; node = hash(left, right); level 0 is the leaves; one leaf: the root is the leaf.
 * Pins (canonical integers):
 *   permute(0, 1, 2) = (0x115cc0f5e7d690413df64c6b9662e9cf2a3617f2743245519e19607a4417189a,
 *                       0x0fca49b798923ab0239de1c9e7a4a9a2210312b6a2f616d18b5a87f9b628ae29,
 *                       0x0e7ae82e40091e63cbd4f16a6d16310b3729d4b6e138fcf54110e2867045a30c)
 *   constant [0][0] = 0x0ee9a592ba9a9518d05986d656f40c2114c4993c11bb29938d21d47304cd8e6e, M[0][0] = 0x109b7f411ba0e4c9b2b70caf5c36a7b194be7c11ad24378bfedb68592ba8118b
 *   squeeze of a fresh sponge = 0x14b2e5484b232721d64f405caa487febbce835dd07c5de940f2a775dc9aa0da6
 *   hash(1, 2) = 0x305df2f9f9f1c0b591427aa9fd8ff8b8b8ad8a16953065fca066cb6a69deff53
 *   root of the leaves (1, 2, 3, 4) = 0x2c01ebd821c7ffc51531dc18169a856bfa0e54c4f5ff99b94f328a38d57d2194
 * Elements are 4 Montgomery words like every other Fr here.  The calls marked "host" touch no GPU and work in a process that never initialises
 * HIP.  The kernels run one lane per message or node (csrc/poseidon.hip). */
#define ZKHIP_POSEIDON_MAX_WIDTH 16   /* the most elements of one message of zkhip_poseidon_hash_many_device */
#define ZKHIP_POSEIDON_SUBTREE 256    /* elements of a level one workgroup of zkhip_poseidon_merkle_device folds: tree sizes around it take different paths */
int zkhip_poseidon_permute(uint64_t *states, size_t n);                                                 /* host; n states of 12 words, in place */
int zkhip_poseidon_hash(const uint64_t *fr, size_t n, uint64_t out[4]);                                 /* host; a fresh sponge over n elements */
/* the table the permutation runs on, canonical integers (not Montgomery): 195 round constants, then the 9 matrix entries row-major (host) */
int zkhip_poseidon_constants(uint64_t out[204 * 4]);
/* n messages of `width` elements each, row-major at d_in; d_out[i] = hash of message i (a fresh sponge each).  1 <= width <=
 * ZKHIP_POSEIDON_MAX_WIDTH, else ZKHIP_EINVAL.  One launch, no host wait (the FIRST Poseidon `_device` call of a process uploads the table and
 * waits for that).  d_in and d_out 16-byte aligned; they must not overlap. */
int zkhip_poseidon_hash_many_device(const void *d_in, size_t n, uint32_t width, void *d_out, void *stream);
/* n secp256k1 points as the PLUME calls hold them (8 little-endian 64-bit words, canonical x then y; ANY 256-bit values are taken) packed and
 * hashed where they lie: d_out[i] = what zkhip_poseidon_hash_many_device gives over the packed message of point i.  layout 0 (nullifier,
 * `compress_native_nullifier`): (2 + (y & 1), x bytes 0..10, 11..21, 22..31 as little-endian integers), width 4.  layout 1 (member, the
 * members tree's leaf): the three chunks of x, then those of y, width 6.  One launch, one lane per point, no host wait (the first Poseidon
 * `_device` call uploads the table).  ZKHIP_EINVAL, nothing enqueued: another layout, a null or non-16-byte-aligned pointer, n above 2^30,
 * d_out overlapping d_points.  n == 0 succeeds and writes nothing. */
int zkhip_poseidon_hash_points_device(const void *d_points, size_t n, uint32_t layout, void *d_out, void *stream);
/* The n_leaves - 1 inner nodes of the tree over d_leaves, level 1 (n_leaves / 2 nodes) first, the root last: level L starts at node
 * n_leaves - (n_leaves >> (L - 1)).  One launch behind one small memset, no host wait.  n_leaves = 1 writes nothing (the root is the leaf).
 * ZKHIP_EINVAL, nothing enqueued: n_leaves not a power of two, 0, or above 2^30; a null or misaligned pointer.  d_nodes must not overlap d_leaves. */
int zkhip_poseidon_merkle_device(const void *d_leaves, size_t n_leaves, void *d_nodes, void *stream);

/* ---- indexed Merkle tree: the nullifier tree of the state-transition circuit, a BATCH of insertions in one device call ----
 * [DEP indexed_merkle_tree_halo2 `IndexedMerkleTree` / `IMTLeaf`; the reference: `generate_state_transition_circuit_inputs` and `update_idx_leaf`,
 * /root/reference/aggregator/src/utils.rs:101-197, which scans for the low leaf and rebuilds the whole tree twice per vote; the witness is the
 * argument list of `IndexedMerkleTreeInput::new`, aggregator/src/state_transition.rs:44-70.]  The hash is the Poseidon of the section above.
 * The FRAMING below is pinned only as these lines word it: the `indexed_merkle_tree_halo2` crate is not vendored with the reference and could
 * not be built, so parity with it is unpinned, like the Poseidon framing.
 * THE DEFINITION (normative):
 *   tree        2^depth leaves.  A leaf has a preimage (val, next_val, next_idx) of three Fr; its value in the tree is hash(val, next_val,
 *               next_idx), the width-3 sponge (two permutations); an inner node is hash(left, right).
 *   empty tree  every preimage is (0, 0, 0).  Leaf 0 is the permanent head of the sorted list; the first free index is 1 (the reference
 *               inserts round r at index r, rounds counted from 1).  `used` counts the head: it is the first free index.
 *   insert v    at the first free index j, values compared as canonical integers: the low leaf l is the used leaf with the greatest val < v
 *               (it exists, and next_val[l] == 0 or next_val[l] > v).  The new leaf becomes (v, next_val[l], next_idx[l]); the low leaf becomes
 *               (val[l], v, j), next_idx held as the field element j.  (`update_idx_leaf`, whose special case for the first insertion is
 *               this rule.)
 *   refusals    v == 0; v equal to a val already in the tree; v equal to an earlier value of the same batch; a value that finds no free
 *               leaf; four words that are not a reduced Montgomery element.  The call returns ZKHIP_EINVAL, *first_bad = the index of the
 *               first such value, nothing is enqueued and the tree is unchanged.  (*first_bad = (size_t)-1 on every other outcome.)
 *   witness of insertion i of a batch:
 *     old_root = roots[i], the root before the insertion; new_root = roots[i + 1], the root after both leaf updates;
 *     low_leaf = the low leaf's preimage BEFORE the insertion, low index = l;
 *     low_leaf_proof = the siblings of the low leaf's path in the tree before the insertion, from the leaf level up;
 *     new_leaf = the new leaf's preimage, new_leaf_index = used-before-the-batch + i;
 *     new_leaf_proof = the siblings of the new leaf's path AFTER the low leaf's update (and before its own);
 *     is_new_leaf_largest = (new_leaf.next_val == 0); the proof helpers are 1 where the path node is a left child (bit L of the index clear).
 * How it runs: the host links the batch over an ordered index of the used values (no scan); the device computes all 2 n_new leaf updates level
 * by level, one lane per update and depth + 2 launches per batch (csrc/imt.hip).  One insertion alone is better served by
 * the host hash: see DESIGN.md section 9 for the batch size from which the device wins.  Not built: removal of leaves, trees sharded over
 * devices.
 * The object lives on the primary device and owns the leaves, inner nodes and preimages in device memory and the host index.  Calls on one
 * object come from one thread at a time and are ordered by the caller on ONE stream; the host index advances at call time.  Destroy it before
 * zkhip_shutdown. */
#define ZKHIP_IMT_MAX_DEPTH 24        /* 160 bytes of device memory per leaf: 2.5 GiB at the cap */
typedef struct zkhip_imt zkhip_imt;
/* where zkhip_imt_insert leaves the witnesses: device pointers the caller owns, 16-byte aligned (d_low_indices: 4-byte), 4 words per element */
typedef struct zkhip_imt_witness {
  void *d_roots;        /* (n_new + 1) x 4 words: entry i the old_root of insertion i, entry i + 1 its new_root */
  void *d_low_leaves;   /* n_new x 12 words */
  void *d_new_leaves;   /* n_new x 12 words */
  void *d_low_indices;  /* n_new uint32 */
  void *d_low_proofs;   /* n_new x depth x 4 words */
  void *d_new_proofs;   /* n_new x depth x 4 words */
} zkhip_imt_witness;
int zkhip_imt_create(uint32_t depth, zkhip_imt **t);             /* 1 <= depth <= ZKHIP_IMT_MAX_DEPTH; the empty tree from depth + 1 host hashes and fills; waits */
int zkhip_imt_destroy(zkhip_imt *t);                              /* NULL is ZKHIP_OK */
/* values: n_new x 4 Montgomery words on the HOST, in insertion order (the linking is host work).  out may be NULL: the call only updates the
 * tree.  No host wait after the uploads.  n_new == 0 is ZKHIP_OK and does nothing.  A null or misaligned pointer is ZKHIP_EINVAL, nothing enqueued. */
int zkhip_imt_insert(zkhip_imt *t, const uint64_t *values, size_t n_new, const zkhip_imt_witness *out, size_t *first_bad, void *stream);
/* host results, read behind the stream of the object's last insert, which they wait for: the root; leaf `index`'s preimage; the depth siblings
 * of its path from the leaf level up.  index >= 2^depth is ZKHIP_EINVAL. */
int zkhip_imt_root(zkhip_imt *t, uint64_t out[4]);
int zkhip_imt_leaf(zkhip_imt *t, uint32_t index, uint64_t out[12]);
int zkhip_imt_proof(zkhip_imt *t, uint32_t index, uint64_t *out /* depth x 4 words */);
int zkhip_imt_size(const zkhip_imt *t, uint32_t *depth, uint32_t *used);                                /* host; either pointer may be NULL */
/* device-to-device copies on `stream`, no host wait: 2^depth leaves, the 2^depth - 1 inner nodes in zkhip_poseidon_merkle_device's order,
 * 2^depth preimages of 12 words */
int zkhip_imt_export_device(zkhip_imt *t, void *d_leaves, void *d_nodes, void *d_preimages, void *stream);
/* The linking alone (host; touches no GPU and works in a process that never initialises HIP; the code the object runs).  used_vals: the vals of
 * leaves 0 .. n_used - 1 in index order, leaf 0 the head with val 0 (n_used == 0 stands for the empty tree).  low_index_out[i] = the low leaf of
 * new value i, inserted at leaf max(n_used, 1) + i.  Refusals as above, except that any number of leaves is free. */
int zkhip_imt_link(const uint64_t *used_vals, size_t n_used, const uint64_t *new_vals, size_t n_new, uint32_t *low_index_out, size_t *first_bad);

/* ---- Paillier tally: the running homomorphic sum of a batch of ballots in one device call ----
 * [DEP paillier_chip `paillier_enc_native` / `paillier_add_native`; the reference: `generate_wrapper_circuit_input`,
 * /root/reference/aggregator/src/utils.rs:298-341, which encrypts every vote and folds the ballots one at a time into `prev_vote`, the argument
 * of `StateTransitionInput::new`, aggregator/src/state_transition.rs:81.]  The `paillier_chip` crate is not vendored with the reference and
 * could not be built, so parity with it is unpinned; only the two textbook formulas are restated here.
 * THE DEFINITION (normative), over non-negative integers, N = n^2:
 *   enc(n, g, m, r) = g^m * r^n mod N                 (`paillier_enc_native`)
 *   add(n, a, b)    = a * b mod N                     (`paillier_add_native`: the product of two ciphertexts encrypts the sum of their votes)
 *   pinned   n = 0x1ef95 (293 * 433), g = n + 1:  enc(m = 42, r = 23) = 0x13a7c1d25,  enc(m = 58, r = 101) = 0x32a4da219,  their add = 0x1b5145505
 *   pinned   n = 2^175 + 2^88 + 1, g = n + 1:  enc(m = 2^253 + 5, r = 2^100 + 7) =
 *            0xd46573adf90cb6f703909e88c21470d8d54038324d18ed3723a3b62fae6bca752ac6bc47b0d61531e9c8199,
 *            enc(m = 1, r = n - 1) = 0x400000000000000000000100000000000000000000018000000000000000000000ffffffffffffffffffffff,
 *            their add = 0x695b9b430ba3fb1445f14b6f5912adac3d5d33a7d5d0877d0cb74a94285556ccd43275cac8214d40c0c624a   (Python `pow`)
 * Formats: a ciphertext is ZKHIP_PAILLIER_WORDS little-endian 64-bit words holding the canonical integer -- NOT Montgomery: the modulus is the
 * caller's, and the Montgomery form mod N is internal to a call.  n is 3 words (at most ZKHIP_PAILLIER_MAX_N_BITS bits), on the HOST, read
 * before the call returns; the modulus is always n^2.  An input >= N is taken mod N, as `BigUint %` would; every output is < N.
 * Every call is asynchronous on `stream` with no host wait; scratch is the stream's workspace; at most 2^32 ciphertexts per call.
 * ZKHIP_EINVAL, nothing enqueued (decided before the device is touched): n even (the arithmetic is Montgomery's and needs an odd modulus;
 * every n = p q of a real key is odd) or n < 3; a null or non-8-byte-aligned pointer with a non-zero count; n_cols == 0; the overlaps named
 * below.  Not built: moduli wider than 384 bits, decryption, a tally sharded over devices. */
#define ZKHIP_PAILLIER_WORDS 6        /* 64-bit words of a ciphertext: an integer below n^2 < 2^384 */
#define ZKHIP_PAILLIER_MAX_N_BITS 192 /* n fits three 64-bit words */
/* d_out[i] = d_a[i] * d_b[i] mod n^2, i < count: `paillier_add_native` over arrays.  d_out may be d_a or d_b; any other overlap is refused. */
int zkhip_paillier_mul_device(const uint64_t n[3], const void *d_a, const void *d_b, size_t count, void *d_out, void *stream);
/* d_ballots: [n_ballots][n_cols] ciphertexts, ballot-major (one ballot contiguous, as it arrives).  d_init: n_cols ciphertexts, the
 * reference's prev_vote at round 0; NULL starts every column from 1.  d_running: [n_ballots + 1][n_cols]: row 0 = init mod n^2, row i + 1 =
 * row i * ballot i mod n^2 column by column -- row i is the prev_vote of round i, the last row the tally.  n_ballots == 0 writes row 0 only.
 * A chunked scan per column, 2 ceil(log_16 n_ballots) - 1 launches above 16 ballots and one below (csrc/paillier.hip).  d_running must not overlap d_ballots or d_init. */
int zkhip_paillier_tally_device(const uint64_t n[3], const void *d_ballots, size_t n_ballots, uint32_t n_cols, const void *d_init, void *d_running, void *stream);
/* d_out[i] = g^m[i] * r[i]^n mod n^2, i < count.  g: 6 words on the host; d_m: 4 words per ciphertext (a vote is `fe_to_biguint` of an Fr);
 * d_r: 3 words per ciphertext (any value; r >= n is not refused).  m = 0 gives g^0 = 1 whatever g is.  One lane per ciphertext, both powers by
 * the plain left-to-right ladder.  d_out must not overlap d_m or d_r. */
int zkhip_paillier_encrypt_device(const uint64_t n[3], const uint64_t g[6], const void *d_m, const void *d_r, size_t count, void *d_out, void *stream);

/* ---- PLUME nullifiers on secp256k1: a batch of nullifiers verified, or signed, in one device call ----
 * [DEP k256 `hash_from_bytes::<ExpandMsgXmd<Sha256>>`, halo2curves secp256k1; the reference: `verify_nullifier`, `compress_point`, `hash_to_curve`
 * and `gen_test_nullifier`, voter_tests/src/lib.rs:25-119, called for every round by `generate_wrapper_circuit_input`,
 * aggregator/src/utils.rs:289-290.]  The crates are not vendored with the reference and could not be built: parity with `k256` / `plume-halo2` is
 * pinned by the two RFC 9380 vectors below and no further; the PLUME vector pins the next restatement against this one.
 * THE DEFINITION (normative).
 *   Curve     secp256k1: y^2 = x^3 + 7 over p = 2^256 - 2^32 - 977, group order
 *             n = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141, generator G as in SEC 2.
 *   compress(P) = the 33 bytes 02|03 || x big-endian, 03 for an odd y (`compress_point`).  The identity is the affine pair (0, 0), as
 *             halo2curves' `to_affine` gives it, and so compresses to 02 || 00..00 (restated, not pinned).
 *   H(msg, pk) = hash_to_curve(msg || compress(pk)) of RFC 9380, suite secp256k1_XMD:SHA-256_SSWU_RO_, with the DST
 *             "QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_": expand_message_xmd to 96 bytes, two 48-byte big-endian values mod p,
 *             simplified SWU on E': y^2 = x^3 + A'x + B' with Z = -11 (the exceptional cases of section 6.6.2 included), the 3-isogeny to
 *             secp256k1 (a zero denominator gives the identity), the sum of the two images.  A', B' and the isogeny's coefficients are those
 *             of RFC 9380 section 8.7 and appendix E.1 (csrc/secp256k1_h2c.hpp).
 *   pinned    (RFC 9380 J.8.1) hash_to_curve(""):    x = 0xc1cae290e291aee617ebaef1be6d73861479c48b841eaba9b7b5852ddfeb1346
 *                                                    y = 0x64fa678e07ae116126f08b022a94af6de15985c996c3a91b64c406a960e51067
 *                              hash_to_curve("abc"): x = 0x3377e01eab42db296b512293120c6cee72b6ecf9f9205760bd9ff11fb3cb2c4b
 *                                                    y = 0x7f95890f33efebd1044d382a01b1bee0900fb6116f94688d487c6c7b9c8371f6
 *   verify(msg, N, pk, s, c) (`verify_nullifier`), with H = H(msg, pk):  A = s G - c pk,  B = s H - c N,
 *             d = SHA-256(compress(G) || compress(pk) || compress(H) || compress(N) || compress(A) || compress(B))   (198 bytes);
 *             accept iff the big-endian integer of d equals c.  d is not reduced: the reference's `from_bytes_le` panics on a digest >= n, and
 *             here such a digest never equals a c < n.
 *   verdict   0 accepted; 1 well-formed but d != c; 2 malformed: a coordinate >= p, a point off the curve (the pair (0, 0) included), or s or
 *             c >= n.  A malformed voter is a verdict, never a failed call.
 *   pinned    msg = 01 00, sk = SHA-256("sk") mod n, r = SHA-256("r") mod n, `gen_test_nullifier` with that r:
 *             pk = (0x020f475341bdcaa86307f6bc73482e9f97de1eb143c4d377882338e41bd3816c, 0xd9b0bc73ac2ef11aa0d9c7e597a2247fae84397fbcf7c5545ca569c392a43d9d)
 *             H  = (0xfc8ad938310804a146d15e27c45dd085890d059a4fe75efb792557945cd4e555, 0x5dff9477353e60cd4f45ced0dadf3646df67bc09aacc29b645ff2338763b8509)
 *             N  = (0x022e80224208f61d2bd0db01ee45f1ad280afed208073f8cadfea796b62ec66e, 0xeb2167a30ea8a02d40c3a86c93961b7f02664aac622d11d34b9f120eed108c73)
 *             s  = 0x2dd6d3be74b08a383e981dac34dda120b5f0d32f9a1e245ab034d00b4d1149a3, c = 0x31c5e6a7886d3802ee2e0bc16993e6dda5f9992597c67ee4bfb5acba7bf07535
 *             verify -> 0; with c + 1 -> 1; with msg = 02 00 -> 1.
 *   sign(msg, sk, r) (`gen_test_nullifier`, r in place of `Fq::random`), sk and r in [1, n):  pk = sk G,  H = H(msg, pk),  N = sk H,
 *             d = SHA-256(compress(G) || compress(pk) || compress(H) || compress(N) || compress(r G) || compress(r H)),
 *             c = the big-endian integer of d, taken mod n (the reference panics on a digest >= n; probability 2^-128),  s = r + sk c mod n.
 *             status 0, or 2 and zeros in every output where sk or r is 0 or >= n.  The pinned vector above is sign(01 00, sk, r).
 *             The ladders are branch-free, but nothing here is audited for side channels: the call is meant for generated populations
 *             (tests, probes, simulations), not for a voter's wallet.
 * Formats: a point is 8 little-endian 64-bit words, x then y, each the canonical integer (NOT Montgomery); a scalar is 4 words.  A verdict or
 * status is a uint32.  msg is on the HOST, read before the call returns, at most ZKHIP_PLUME_MAX_MSG bytes, and shared by the batch (the proposal).
 * The `_device` calls are asynchronous on `stream` with no host wait; at most 2^30 elements per call.
 * ZKHIP_EINVAL, nothing enqueued (decided on the host before the device is touched): a null pointer where none is allowed (msg may be null when
 * msg_len is 0; d_h_out may be null; every array may be null when count is 0, d_report never), msg_len > ZKHIP_PLUME_MAX_MSG, a pointer that is
 * not 8-byte aligned, an output that overlaps an input or another output.  count == 0 succeeds; the verify call then writes only a zeroed report.
 * Not built: a fixed-base table for G, batch verification by a random linear combination, sharding over devices, PLUME v2, constant-time
 * guarantees. */
#define ZKHIP_PLUME_MAX_MSG 64
/* d_out[i] = a[i] P[i] + b[i] Q[i], affine, identity as (0, 0); scalars are any 256-bit integers; a malformed P or Q gives status 2 and (0, 0) */
int zkhip_secp256k1_lincomb_device(const void *d_a, const void *d_p, const void *d_b, const void *d_q, size_t count, void *d_out, void *d_status, void *stream);
/* d_out[i] = H(msg, pk[i]); msg on the host, shared by the batch (the proposal); a malformed pk gives status 2 and (0, 0) */
int zkhip_secp256k1_hash_to_curve_device(const uint8_t *msg, size_t msg_len, const void *d_pk, size_t count, void *d_out, void *d_status, void *stream);
/* d_status[i] (uint32) = the verdict above; d_report: one zkhip_check_report -- voters with a non-zero verdict, lowest such index; d_h_out optional
 * (NULL or count points): H of every voter, (0, 0) where pk is malformed.  Two lanes per voter (csrc/plume.hip). */
int zkhip_plume_verify_device(const uint8_t *msg, size_t msg_len, const void *d_pk, const void *d_nullifier, const void *d_s, const void *d_c, size_t count, void *d_status, void *d_report, void *d_h_out, void *stream);
/* sign of every voter: d_sk, d_r count scalars in; d_pk, d_nullifier count points, d_s, d_c count scalars, d_status count uint32 out; d_h_out
 * optional (NULL or count points): H of every voter.  A malformed sk or r gives status 2 and zeros in every output of that voter.  One launch, two
 * lanes per voter (csrc/plume_sign.hip); count == 0 succeeds and writes nothing. */
int zkhip_plume_sign_device(const uint8_t *msg, size_t msg_len, const void *d_sk, const void *d_r, size_t count, void *d_pk, void *d_nullifier, void *d_s, void *d_c, void *d_status, void *d_h_out, void *stream);
/* The same for one voter on the host, over the same headers; no GPU is touched.  out = H(msg, pk) and *status 0, or (0, 0) and 2 for a malformed pk. */
int zkhip_secp256k1_hash_to_curve(const uint8_t *msg, size_t msg_len, const uint64_t pk[8], uint64_t out[8], uint32_t *status);
/* *verdict as above; h_out optional: H(msg, pk), (0, 0) where pk is malformed */
int zkhip_plume_verify(const uint8_t *msg, size_t msg_len, const uint64_t pk[8], const uint64_t nullifier[8], const uint64_t s[4], const uint64_t c[4], uint32_t *verdict, uint64_t h_out[8]);
/* *status 0 and the signature, or 2 and zeros; h_out optional: H(msg, pk) */
int zkhip_plume_sign(const uint8_t *msg, size_t msg_len, const uint64_t sk[4], const uint64_t r[4], uint64_t pk[8], uint64_t nullifier[8], uint64_t s[4], uint64_t c[4], uint32_t *status, uint64_t h_out[8]);

/* ---- the quotient identity at x: the scalar half of `verify_proof`, a batch of proofs in one call -------------------------------------
 * [DEP] halo2-axiom plonk/verifier.rs recomputes the expected quotient evaluation from the gate, permutation and lookup expressions at the
 * challenge x and compares it with h(x) (x^n - 1); the reference's aggregator does so for the voter proof of every ballot
 * (/root/reference/aggregator/src/wrapper.rs:140-155).  One proof is a few thousand field products, so the unit of work is the batch: every
 * proof of one circuit is a ROW of one row program (an ordinary zkhip_vm_program), run by the interpreter of zkhip_fr_eval_rows_device (never
 * the run-time compiler).  Both calls are asynchronous on `stream`, wait for nothing on the host, take their scratch from the stream's
 * scratch set and return ZKHIP_OK when the check RAN, whatever it found (as the witness checks above).  All elements are in the external Fr
 * format (4 x u64 Montgomery-256, canonical); device arrays of elements are 16-byte aligned.  Argument errors are ZKHIP_EINVAL, decided on the
 * host before the device is touched, with nothing enqueued.
 *
 * Domain values.  n = 2^k rows; rows 0 .. usable_rows - 1 are usable, row u = usable_rows carries l_last and the n - u - 1 rows behind it are
 * blinding rows.  With l_i(x) = omega^i (x^n - 1) / (n (x - omega^i)):  l_last = l_u,  l_active = 1 - l_last - sum_{i > u} l_i.
 * zkhip_fr_domain_points_device: one lane per point; d_out is [4][n_points]: x^n, l_0(x), l_last(x), l_active(x).  A point OF the domain
 * (x^n = 1) has no closed form: its four values are written as zero, which no other point produces (x^n = 0 only at x = 0, where l_0 = 1 / n).
 * ZKHIP_EINVAL unless k <= 28, 1 <= usable_rows < 2^k, 2^k - usable_rows <= 64 (the per-lane loop; halo2 circuits have 5 to 10 blinding
 * rows), n_points >= 1 (at most 2^30), omega canonical, no null or misaligned pointer.
 *
 * zkhip_verify_identity_device.  d_evals: [n_proofs][n_evals], one record per proof as it comes off that proof's transcript; d_challenges:
 * [n_proofs][5] = theta, beta, gamma, y, x.  COLUMNS OF THE PROGRAM (normative): column j < n_evals is evaluation j of the record;
 * columns n_evals + 0 .. 4 are theta, beta, gamma, y, x; columns n_evals + 5 .. 8 are x^n, l_0(x), l_last(x), l_active(x).  The program's
 * result must be zero exactly when the identity holds (evaluation.py identity_program builds it from the terms of the prover's quotient).
 * d_status: int32[n_proofs] -- 0 the identity holds; 1 it does not; 2 x lies in the domain (x^n = 1), so nothing was divided: a verdict,
 * never a failed call.  d_report: one zkhip_check_report -- `failures` the number of proofs with a status other than 0, `first` the lowest
 * such index, UINT64_MAX when there is none.  n_proofs == 0: ZKHIP_OK, the report says "no failure", nothing else is written.
 * ZKHIP_EINVAL: a program zkhip_fr_eval_rows_device rejects over n_evals + 9 columns (a column >= n_evals + 9 included), or one whose
 * rotation table holds a non-zero rotation, or that reads ZKHIP_SRC_PREV or ZKHIP_SRC_ROWPOW; n_evals == 0 or n_evals + 9 > 65536;
 * n_proofs > 2^24; the domain arguments as above; a null pointer, d_evals / d_challenges not 16-byte aligned, d_status not 4-byte or d_report
 * not 8-byte aligned (with n_proofs == 0 the three arrays may be null, d_report never).
 *
 * Instance columns (public inputs).  With halo2's KZG scheme an instance polynomial is neither committed nor opened: the verifier evaluates it
 * at x omega^rot from the public inputs.  A circuit has n_columns instance columns, column c of column_lens[c] values (zeros behind them);
 * d_instances: [n_proofs][total_len] elements, total_len = the sum of column_lens, column c's values at offset sum_{c' < c} column_lens[c'].
 * A QUERY q is a pair (query_columns[q], query_rotations[q]), the rotation reduced mod 2^k as an unsigned value (rotation -1 is 2^k - 1):
 *   e[q][p] = sum_{i < len_c} v[p][c][i] l_((i - rot) mod n)(x_p)          (len_c = 0 gives 0; x_p in the domain gives 0, nothing is divided)
 * The three host arrays are consumed before a call returns.
 * zkhip_fr_instance_evals_device: d_x [n_proofs] points, d_out [n_queries][n_proofs] (the layout of zkhip_fr_domain_points_device); a group of
 * lanes per (query, proof), one inversion per group.  n_proofs == 0 or n_queries == 0: ZKHIP_OK, nothing is written.  ZKHIP_EINVAL: k == 0 or
 * k > 28, omega null or not canonical, n_columns or n_queries above 64, a null host array that is not empty, a query column >= n_columns, a
 * rotation >= 2^k, column_lens[c] > 2^k, n_proofs > 2^24, d_x or d_out null or misaligned where there is something to write, d_instances
 * null or misaligned where total_len * n_proofs > 0.
 * zkhip_verify_identity_instances_device: zkhip_verify_identity_device for a circuit with instance columns.  COLUMNS OF THE PROGRAM
 * (normative): columns 0 .. n_evals + 8 as above; column n_evals + 9 + q is query q, evaluated at the record's x; the program is validated
 * over n_evals + 9 + n_queries columns.  With n_queries == 0 it does what zkhip_verify_identity_device does.  Status 2 is unchanged (the
 * instance columns of such a proof are zero).  ZKHIP_EINVAL: the conditions of zkhip_verify_identity_device; n_columns or n_queries above 64;
 * a query column >= n_columns; a rotation >= 2^k; column_lens[c] > usable_rows (halo2's `InstanceTooLarge`); d_instances null or misaligned
 * where total_len * n_proofs > 0.
 * Not built: committed instance columns (`QUERY_INSTANCE = true`, the IPA scheme), multi-phase challenges -- DESIGN.md section 10. */
int zkhip_fr_domain_points_device(uint32_t k, uint32_t usable_rows, const uint64_t omega[4], const void *d_x, size_t n_points, void *d_out, void *stream);
int zkhip_verify_identity_device(const zkhip_vm_program *prog, const void *d_evals, uint32_t n_evals, const void *d_challenges, uint32_t k,
                                 uint32_t usable_rows, const uint64_t omega[4], size_t n_proofs, void *d_status, void *d_report, void *stream);
int zkhip_fr_instance_evals_device(uint32_t k, const uint64_t omega[4], const void *d_x, const void *d_instances, const uint32_t *column_lens, uint32_t n_columns,
                                   const uint32_t *query_columns, const uint32_t *query_rotations, uint32_t n_queries, size_t n_proofs, void *d_out, void *stream);
int zkhip_verify_identity_instances_device(const zkhip_vm_program *prog, const void *d_evals, uint32_t n_evals, const void *d_challenges, uint32_t k,
                                           uint32_t usable_rows, const uint64_t omega[4], const void *d_instances, const uint32_t *column_lens, uint32_t n_columns,
                                           const uint32_t *query_columns, const uint32_t *query_rotations, uint32_t n_queries, size_t n_proofs,
                                           void *d_status, void *d_report, void *stream);

/* ---- parity hooks for the field / curve layer (rows a1/a2 of SURVEY.md section 8) ------------------ */
/* field: 0 = Fq, 1 = Fr.  op: 0 mul, 1 add, 2 sub, 3 square (b ignored).  Elementwise on n elements.
 * The shapes the MSM / NTT kernels instantiate: 4 = mul and 5 = square as single-chain product columns (the asm blocks of mac_blocks.hpp; same
 * values as 0 and 3), 6 = fe_mul_add in the compiler's shape and 7 = in the chain shape: out[i] = a[i] b[i] + a[i ^ 1] b[i ^ 1], two products
 * under one Montgomery reduction (n must be even, else ZKHIP_EINVAL).
 * op + 256, for op 4 .. 7: the same operation with every operand first replaced by the largest representative of its residue that the
 * operation's documented limb / value bounds allow (csrc/fe_lift.hpp); the outputs are those of the plain op. */
int zkhip_test_field_op(int field, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n);
/* op: 0 = affine a[i] + affine b[i], 1 = 2 * a[i], 2 = a[i] + (-b[i]); with the quad-cooperative formulas of the reduction tail:
 * 3 = 2 a[i] + 2 b[i], 4 = 4 a[i]; through the bucket kernels' mixed addition xyzz_madd<true> (Y3 as one fused product pair), twice:
 * 5 = a[i] + b[i], 6 = a[i] + (-b[i]).  5 + 256, 6 + 256: the same with the loaded coordinates lifted to the top of 64p and the accumulator,
 * after the first addition, to the top of the stored-point invariant of csrc/ec.hpp.  out: n Jacobian points. */
int zkhip_test_g1_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out_xyz, size_t n);

/* G2 (Fq2 + twist curve arithmetic): op 0 = a[i] + b[i], 1 = 2 a[i], 2 = a[i] - b[i]; with the quad-cooperative formulas of the MSM's
 * latency-bound end: 3 = 2 a[i] + b[i], 4 = 4 a[i]; with their lazy forms chained as in the window fold: 5 = 4 a[i] + b[i], 6 = 16 a[i].
 * The lazy Fq2 layer of the bucket kernels (csrc/ec2.hpp), coordinates unpacked without a multiplication as the accumulation does:
 * 7 = a[i] + b[i] and 8 = a[i] - b[i] (the negated load) through xyzz2_madd_lazy<true> twice, then xyzz2_to_std; 9 = 2 a[i] + b[i] through
 * xyzz2_add_lazy<true>; 10 = the same sum with both operands stored as 288-byte work points: even rows through xyzz2_add_lazy_mem<true>, odd rows
 * through xyzz2_add_lazy_regmem<true>; 11 = xyzz2_add_lazy<true>(2 a[i], 2 a[i]), the doubling inside the general addition.
 * op + 256, for op 5 .. 11: the same with every operand of the formula under test (for 5 and 6: the lazy quad point between the links of
 * the chain) lifted to the top of its documented magnitude bound (csrc/fe_lift.hpp); the outputs are those of the plain op.
 * No op checks that a point is on the curve: the formulas never use the curve constant.
 * a, b: n G2Affine points, out: n G2 Jacobian points */
int zkhip_test_g2_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out_xyz, size_t n);

/* the transcript's challenge reduction on its own: 64 bytes as a little-endian 512-bit integer mod r, 4 Montgomery words (host, no GPU) */
int zkhip_test_reduce512(const uint8_t in64[64], uint64_t out_fr_mont[4]);
/* how many points share one inversion when zkhip_transcript_write_points_device runs over n points (the kernel's launch shape; host, no GPU) */
uint32_t zkhip_test_transcript_chunk(size_t n);

/* ---- pairing check (`multi_miller_loop` + `final_exponentiation` + `is_identity` [DEP halo2curves bn256], under `verify_proof` and the decider) ---- */
#define ZKHIP_MAX_PAIRS 64
/* *ok = 1 when prod_i e(g1[i], g2[i]) is the identity of Gt, else 0.  g1: n x 8 words (G1Affine, Montgomery, (0,0) = identity),
   g2: n x 16 words (G2Affine as zkhip_msm_g2 takes it).  A pair with either point the identity contributes 1; n = 0 gives 1.
   Points are NOT checked to be on the curve or in the subgroup (as halo2curves' multi_miller_loop does not): callers that
   read them from a file check them first.  n > ZKHIP_MAX_PAIRS or a null pointer with n > 0: ZKHIP_EINVAL, nothing enqueued.
   The Gt value itself is not an interface: only the verdict leaves the device.  `_device`: asynchronous on `stream`, no host wait;
   d_g1 and d_g2 must be 16-byte aligned (the pairs are read with vector loads; any zkhip_alloc'd block is) and d_ok 4-byte aligned, else ZKHIP_EINVAL. */
int zkhip_pairing_check(const uint64_t *g1, const uint64_t *g2, size_t n, int *ok);
int zkhip_pairing_check_device(const void *d_g1, const void *d_g2, size_t n, void *d_ok /* one uint32 */, void *stream);
/* One operation of the Fq12 tower (csrc/pairing.hpp) on the device, so that a wrong verdict can be located.  a, b: 48 words each (the 12 Fq
 * coefficients c0.c0.c0, c0.c0.c1, c0.c1.c0 .. c1.c2.c1, Montgomery); out: 2 x 48 words, canonical: first through the quad policy in one quad,
 * then through the single-lane policy in one lane.  op: 0 mul, 1 sqr, 2 inverse, 3 / 4 / 5 Frobenius q / q^2 / q^3, 6 cyclotomic square (a in
 * the cyclotomic subgroup), 7 a times the sparse line x + y w + z w^3 with (x, y, z) the first three Fq2 of b, 8 the Miller value of the one
 * pair a = G1Affine (8 words) | G2Affine (16 words), 9 the final exponentiation, 10 conjugation, 11 the verdict (out word 0) of the two pairs
 * a = 2 G1Affine | 2 G2Affine run as one serial chain.  op + 256: quad policy only, op + 512: single-lane policy only (the other half of out
 * is left as it was). */
int zkhip_test_fq12_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out);

/* ---- the batch verifier: the opening checks of a batch folded into one pairing check ---------------------------------------------------------
 * The openings of proof i accept exactly when e(A_i, g2) e(-C_i, [s]g2) = 1, A_i and C_i linear combinations of the proof's commitments, the
 * key's commitments and G.  With random r_i the batch accepts, except with probability about 1 / r, exactly when
 * e(sum r_i A_i, g2) e(-sum r_i C_i, [s]g2) = 1: two MSMs and one pairing check (halo2's `BatchVerifier`; the reference's aggregator folds its
 * KZG accumulators the same way, `KzgAs<Bn256, Gwc19>`).  The calls below are the scalar side: the scalars of A_i and C_i of every proof for the
 * GWC multi-open and for the SHPLONK multi-open, and the scaling and folding of such ROWS of scalars by the r_i; multiopen.fold_check is the
 * sequence around them.  All are asynchronous on `stream`, wait for nothing on the host and take their scratch from the stream's scratch set.  Elements are in the
 * external Fr format (4 x u64 Montgomery-256, canonical); device arrays are 16-byte aligned.  Argument errors are ZKHIP_EINVAL, decided on the
 * host before the device is touched, with nothing enqueued.
 *
 * zkhip_gwc_plan: a key's opening plan as the GWC verifier groups it, fixed per key, host memory, consumed before the call returns.  Query q is
 * evaluation q of a proof's record.  n_sets point sets: set_rotation[i] is the rotation of set i reduced mod 2^k as an unsigned value, the
 * sets in order of first appearance among the queries (multiopen.construct_intermediate_sets grouped by rotation).  n_slots opened polynomials,
 * one slot each, the proof's own polynomials first and the key's behind them.  query_set[q], query_slot[q]: the set and the polynomial of
 * query q; query_pos[q]: its position inside its set, the exponent of v.  (A tagged struct: its ctypes mirror _lib.GwcPlan is checked by
 * tests/test_gwc_fold_host.py.)
 *
 * zkhip_gwc_scalars_device.  d_evals: [n_proofs][n_evals]; d_points: [n_proofs][3] = x, v, u.  COLUMNS OF A ROW OF d_rows_a (normative), with
 * n_cols = n_sets + n_slots + 1:
 *   column i < n_sets (witness W_i):          u^i x omega^set_rotation[i]
 *   column n_sets + p (polynomial slot p):    sum over the queries q with query_slot[q] = p of u^query_set[q] v^query_pos[q]
 *   column n_cols - 1 (G):                    - sum_q u^query_set[q] v^query_pos[q] evals[q]
 * d_rows_a is [n_proofs][n_cols]; d_rows_c is [n_proofs][n_sets], column j = u^j.  One workgroup per proof, one lane per column.
 * The plan is validated, marshalled (its CSR lists, omega^set_rotation[i]) and uploaded inside every call, in pieces of 32 KB through the
 * stream's ring of eight pinned slots: a plan above 256 KB of tables (2 n_evals + n_slots + 8 n_sets + 1 words of 4 bytes) waits on the host
 * for its own first pieces to be copied -- the one exception to "no host wait"; the plans of this project are at most 24 KB.
 * n_proofs == 0: ZKHIP_OK, nothing is written.  ZKHIP_EINVAL: a null plan or plan array; n_sets outside 1 .. 64; n_evals outside 1 .. 65527;
 * n_slots outside 1 .. 65536; k > 28; omega null or not canonical; set_rotation[i] >= 2^k; query_set[q] >= n_sets; query_pos[q] >= n_evals;
 * query_slot[q] >= n_slots; n_proofs > 2^24; with n_proofs > 0 a device pointer that is null or not 16-byte aligned.
 *
 * zkhip_fr_fold_rows_device.  d_rows: [n_rows][n_cols]; d_r: [n_rows]; negate: 0 or 1, the sign of every output.
 *   d_out_own    [n_rows][n_own]      out_own[i][j] = +- r_i rows[i][j]                          for j < n_own
 *   d_out_shared [n_cols - n_own]     out_shared[j] = +- sum_i r_i rows[i][n_own + j]            exact for every n_rows (a second level joins the
 *                                                                                                 workgroups' sums above 4096 rows)
 * n_own == 0, n_own == n_cols and n_rows == 0 are legal; with n_rows == 0 the shared part is written as zeros.  A sub-range of a batch is the
 * same call with offset pointers.  The outputs must not overlap the inputs.  ZKHIP_EINVAL: n_cols outside 1 .. 65536; n_own > n_cols; negate
 * other than 0 or 1; n_rows > 2^24 or n_rows n_cols > 2^32; a pointer that is read or written and is null or not 16-byte aligned (d_rows, d_r
 * and d_out_own only where n_rows > 0, d_out_own only where n_own > 0, d_out_shared only where n_own < n_cols).
 *
 * zkhip_shplonk_plan: a key's opening plan as the SHPLONK verifier groups it, fixed per key and k, host memory, consumed before the call returns.
 * n_points super points: point_rotation[t] is a distinct rotation of the plan reduced mod 2^k as an unsigned value.  n_sets rotation sets, the
 * opened polynomials grouped by their set of rotations, sets in order of first appearance (multiopen.construct_rotation_sets grouped by
 * rotation): set i holds the super points set_point[set_start[i] .. set_start[i + 1] - 1], at least one, none twice.  n_slots opened polynomials,
 * one slot each, the proof's own first and the key's behind them: slot_set[p] is the set of polynomial p (it has exactly one), slot_pos[p] its
 * position inside that set, the exponent of y.  Query q is evaluation q of a proof's record: polynomial query_slot[q] at super point
 * query_point[q]; every (polynomial, point of its set) pair is queried exactly once.  (A tagged struct: its ctypes mirror _lib.ShplonkPlan is
 * checked by tests/test_shplonk_fold_host.py.)
 *
 * zkhip_shplonk_scalars_device.  d_evals: [n_proofs][n_evals]; d_points: [n_proofs][4] = x, y, v, u; d_status: [n_proofs] uint32.  Per proof,
 * with w = omega (the 2^k-th root the rotations are powers of; taken as given) and d_t = u - x w^point_rotation[t]:
 *   Z_i = the product of d_t over the super points outside set i (the empty product is 1), Z_T = the product over all of them,
 *   w_i = v^i Z_i / Z_0,
 *   L_(i,a) = w_i prod_(b in set i, b != a) d_b / (x w^rot_a - x w^rot_b): w_i times the Lagrange basis of set i's points at u.
 * COLUMNS OF A ROW OF d_rows_a (normative), with n_cols = 2 + n_slots + 1, the layout [H', H | own polynomials | key polynomials | G]:
 *   column 0 (H'):                            u
 *   column 1 (H):                             - Z_T / Z_0
 *   column 2 + p (polynomial slot p):         w_slot_set[p] y^slot_pos[p]
 *   column n_cols - 1 (G):                    - sum_q L_(slot_set[query_slot[q]], query_point[q]) y^slot_pos[query_slot[q]] evals[q]
 * d_rows_a is [n_proofs][n_cols]; d_rows_c is [n_proofs][1], the column 1 (the scalar of H').  These are multiopen.shplonk_accumulate's scalars.
 * status 0: the rows are written.  status 1: x Z_0 = 0 -- x = 0, or u on a point outside set 0 --, the proof has no such row: both of its rows are
 * written as zeros, no other proof of the launch is affected, and the caller verifies that proof one by one.  u on a point of set 0 is status 0:
 * Z_T = 0 and the H column is an exact zero.  One workgroup per proof and one field inversion per proof; 1 / prod (w^rot_a - w^rot_b) is
 * computed on the host when the plan is marshalled.  The plan is validated, marshalled and uploaded inside every call, through the same ring
 * of pinned slots as the GWC plan (its tables: 8 + 8 n_points + 9 pairs + n_sets + 1 + n_slots + n_evals words of 4 bytes, pairs = set_start[n_sets]).
 * n_proofs == 0: ZKHIP_OK, nothing is written.  ZKHIP_EINVAL: a null plan or plan array; n_sets or n_points outside 1 .. 64; set_start not
 * starting at 0, a set without a point, more than 256 (set, point) pairs in all; n_evals outside 1 .. 65527; n_slots outside 1 .. 65536; k > 28;
 * omega null or not canonical; point_rotation[t] >= 2^k or repeated; set_point[j] >= n_points or repeated inside a set; slot_set[p] >= n_sets;
 * slot_pos[p] >= 2^16; query_slot[q] >= n_slots; query_point[q] >= n_points or not in the set of its slot; a (slot, point) pair queried twice
 * or not at all (n_evals is the sum over the slots of their sets' sizes); n_proofs > 2^24; with n_proofs > 0 a device pointer that is null or
 * not 16-byte aligned.
 * Not built: folding across different circuits or parameter sets, a batch sharded over devices. */
struct zkhip_gwc_plan {
  uint32_t n_evals, n_sets, n_slots, reserved;
  const uint32_t *set_rotation;     /* [n_sets] */
  const uint32_t *query_set;        /* [n_evals] */
  const uint32_t *query_pos;        /* [n_evals] */
  const uint32_t *query_slot;       /* [n_evals] */
};
typedef struct zkhip_gwc_plan zkhip_gwc_plan;
int zkhip_gwc_scalars_device(const zkhip_gwc_plan *plan, const void *d_evals, const void *d_points, uint32_t k, const uint64_t omega[4], size_t n_proofs,
                             void *d_rows_a, void *d_rows_c, void *stream);
int zkhip_fr_fold_rows_device(const void *d_rows, uint32_t n_cols, uint32_t n_own, const void *d_r, int negate, size_t n_rows, void *d_out_own,
                              void *d_out_shared, void *stream);
struct zkhip_shplonk_plan {
  uint32_t n_evals, n_sets, n_slots, n_points;
  const uint32_t *point_rotation;   /* [n_points]  distinct, < 2^k */
  const uint32_t *set_start;        /* [n_sets + 1] CSR over set_point */
  const uint32_t *set_point;        /* [set_start[n_sets]] indices into point_rotation; distinct inside a set */
  const uint32_t *slot_set;         /* [n_slots] */
  const uint32_t *slot_pos;         /* [n_slots]  < 2^16 */
  const uint32_t *query_slot;       /* [n_evals] */
  const uint32_t *query_point;      /* [n_evals]  index into point_rotation */
};
typedef struct zkhip_shplonk_plan zkhip_shplonk_plan;
int zkhip_shplonk_scalars_device(const zkhip_shplonk_plan *plan, const void *d_evals, const void *d_points, uint32_t k, const uint64_t omega[4], size_t n_proofs,
                                 void *d_rows_a, void *d_rows_c, void *d_status, void *stream);

/* ---- KZG accumulators -------------------------------------------------------------------------------------------------------------------
 * A KZG accumulator is a pair of G1 points (lhs, rhs) with e(lhs, g2) = e(rhs, [s] g2): what a proof's opening check leaves when the pairing
 * is not taken (`PlonkSuccinctVerifier::verify` of the reference, aggregator/src/wrapper.rs:433-536), what `KzgAs` folds, and what the
 * wrapper carries from round to round as 12 public inputs.  lhs is the A point of the batch verifier's rows above, rhs the C point.
 *
 * zkhip_g1_row_msm_device: n_rows independent small MSMs in one launch set (csrc/row_msm.hip),
 *     out[i] = sum_{j < n_own} rows[i][j] own[i][j]  +  sum_{n_own <= j < n_cols} rows[i][j] shared[j - n_own].
 *   d_rows           [n_rows][n_cols] Fr, 4 Montgomery words each, canonical (the rows of zkhip_gwc_scalars_device / zkhip_shplonk_scalars_device)
 *   d_own_points     row i's own points start at element i * own_stride: 64-byte affine points.  own_stride >= n_own lets the C side of a batch
 *                    read the first c own points of every row of the A side's array without a copy
 *   d_shared_points  [n_cols - n_own] affine points shared by every row
 *   d_out_xyz        [n_rows] 96-byte Jacobian points, the format the MSM calls leave: it goes straight into zkhip_g1_batch_normalize_device and
 *                    zkhip_transcript_write_points_device
 * The affine identity (0, 0) is a legal point anywhere; a zero scalar, two equal points in a row, P beside -P and a row that sums to the identity
 * give what the group law says.  One launch set of at most two launches (one for n_cols <= 64; wider rows are cut into chunks of 64 columns
 * whose partial sums meet in the second), no host wait, no allocation beyond the stream's scratch (144 bytes per chunk of a row, rows wider than
 * 64 columns only).  A lane runs a GLV joint ladder over its column, so the call's latency is that of ~128 dependent point doublings and
 * additions whatever n_rows is, until the chip is full.  n_rows == 0: ZKHIP_OK, nothing is written.  ZKHIP_EINVAL, decided before HIP is
 * touched and with nothing enqueued: n_cols == 0; n_own > n_cols; own_stride < n_own; n_rows * n_cols above 2^31; own points spread over more
 * than 2^40 elements ((n_rows - 1) * own_stride); with n_rows > 0 a pointer that is needed (d_rows, d_out_xyz, d_own_points where n_own > 0,
 * d_shared_points where n_own < n_cols) and is null or not 16-byte aligned; d_out_xyz overlapping an input.
 *
 * Limbs (csrc/kzg_limbs.hpp has the normative text and the arithmetic, for host and device): ZKHIP_KZG_LIMBS = 3 limbs of
 * ZKHIP_KZG_LIMB_BITS = 88 bits per coordinate.  A point becomes 6 Fr values: x's canonical integer cut little-endian into three 88-bit limbs,
 * then y's, each limb an Fr in Montgomery words; an accumulator is lhs then rhs, 12 values (`[lhs.x, lhs.y, rhs.x, rhs.y].flat_map(fe_to_limbs)`).
 * `affine`: n points of 8 words; `fr_out` / `fr_in`: n x 6 values of 4 words; `status`: n uint32.  Encode splits whatever canonical coordinates
 * it is given.  Decode is strict and never a failed call: status 0 accepted, 1 a limb >= 2^88 (or a value that is no canonical Fr), 2 a
 * coordinate >= q, 3 not on y^2 = x^3 + 3 -- (0, 0) gets status 3, as `from_xy` would refuse it; a refused point is written as (0, 0).
 * (1, 2) |-> [1, 0, 0, 2, 0, 0].  The host forms touch no GPU and work in a process that never initialises HIP.  ZKHIP_EINVAL: with n > 0 a null
 * pointer; for the device forms also a pointer that is not 16-byte aligned (d_status: 4-byte) and n > 2^31.
 * Not built: blinded `KzgAs` (the reference's keys have no zk), the in-circuit side of the accumulation, a batch sharded over devices. */
#define ZKHIP_KZG_LIMBS 3
#define ZKHIP_KZG_LIMB_BITS 88
int zkhip_g1_row_msm_device(const void *d_rows, size_t n_cols, const void *d_own_points, size_t n_own, size_t own_stride, const void *d_shared_points,
                            size_t n_rows, void *d_out_xyz, void *stream);
int zkhip_kzg_limbs_encode(const uint64_t *affine, size_t n, uint64_t *fr_out);
int zkhip_kzg_limbs_decode(const uint64_t *fr_in, size_t n, uint64_t *affine, uint32_t *status);
int zkhip_kzg_limbs_encode_device(const void *d_affine, size_t n, void *d_fr_out, void *stream);
int zkhip_kzg_limbs_decode_device(const void *d_fr_in, size_t n, void *d_affine, void *d_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_H */

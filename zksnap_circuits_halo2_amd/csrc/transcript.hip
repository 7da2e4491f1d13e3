// The field and curve work that feeds the transcript's hash (include/zkhip.h, "transcript"): what halo2's `TranscriptWrite::write_point` /
// `write_scalar` do per element before they hash -- `to_affine()`, `coordinates()`, `to_repr()`, `to_bytes()` [DEP halo2-axiom transcript.rs,
// halo2curves derive/curve.rs; reached from create_proof, /root/reference/aggregator/src/wrapper.rs:129] -- for a whole batch in one launch.
// The hash itself runs on the host (blake2b.hpp).
//
//   k_transcript_points   n Jacobian commitments as the MSM calls leave them (24 words) -> n records of 96 bytes: canonical x (32 bytes,
//                         little-endian) | canonical y | the 32-byte GroupEncoding of serde.hip's k_g1_compress.  The z's of a chunk of
//                         points share one inversion (Montgomery's trick, fe_inverse.hpp once per thread).  Identity inputs (z = 0) get a
//                         zero record and are COUNTED in *ident (zero before the launch): a transcript refuses them.
//   k_transcript_scalars  n Montgomery Fr -> n canonical 32-byte reprs.
//   k_transcript_affine   n affine Montgomery points (what k_g1_decompress wrote) -> n records of 64 bytes, canonical x | y: the read side's
//                         absorb.  The lowest index of a (0, 0) point -- an identity encoding, or one k_g1_decompress refused -- goes to *first_bad.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ec.hpp"
#include "fe_inverse.hpp"
#include "zkhip_internal.hpp"

namespace zkhip {

// Launch shape of k_transcript_points.  n runs from 1 to a few thousand and the kernel is one inversion deep whatever the chunk, so up to
// TR_SINGLE_MAX points every thread inverts its own z (16 workgroups at most); beyond that the chunk doubles until TR_CHUNK_MAX, which
// keeps the launch at 16 workgroups up to 8192 points.  tests/test_gpu_transcript.py names these sizes.
constexpr int TR_BLOCK = 64;
constexpr uint32_t TR_CHUNK_MAX = 8;
constexpr uint32_t TR_SINGLE_MAX = 1024;

uint32_t transcript_chunk(size_t n) {
  uint32_t ch = 1;
  while (ch < TR_CHUNK_MAX && (n + ch - 1) / ch > TR_SINGLE_MAX) ch <<= 1;
  return ch;
}

__device__ __forceinline__ void load_words6(const uint32_t* p, uint32_t (&x)[8], uint32_t (&y)[8], uint32_t (&z)[8]) {
  load_words(p, x);
  load_words(p + 8, y);
  load_words(p + 16, z);
}

__global__ void __launch_bounds__(TR_BLOCK) k_transcript_points(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out, uint32_t ch,
                                                                int layout, uint32_t* __restrict__ ident) {
  __shared__ uint32_t pref_lds[TR_CHUNK_MAX][NL][TR_BLOCK];          // prefix products of the thread's z's, a column per thread
  const uint32_t lo = (blockIdx.x * TR_BLOCK + threadIdx.x) * ch;
  if (lo >= n) return;                                               // no barrier below: the LDS columns are private
  const uint32_t cnt = min(ch, n - lo);
  const fe one = fe_one<Fq>();
  fe pref = one;
  uint32_t identities = 0;
  for (uint32_t i = 0; i < cnt; i++) {
    uint32_t zw[8];
    load_words(in + (size_t)(lo + i) * 24 + 16, zw);
#pragma unroll
    for (int l = 0; l < NL; l++) pref_lds[i][l][threadIdx.x] = pref.l[l];
    if (words_zero(zw)) { identities++; continue; }
    pref = fe_mul<Fq>(pref, fe_mul<Fq>(one, fe_from_ext_lazy(zw)));
  }
  if (identities) atomicAdd(ident, identities);
  fe inv = fe_inverse<Fq>(pref);
  for (uint32_t i = cnt; i-- > 0;) {
    uint32_t xw[8], yw[8], zw[8];
    load_words6(in + (size_t)(lo + i) * 24, xw, yw, zw);
    uint32_t* o = out + (size_t)(lo + i) * 24;
    uint32_t ox[8] = {0, 0, 0, 0, 0, 0, 0, 0}, oy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, oe[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!words_zero(zw)) {
      fe before;
#pragma unroll
      for (int l = 0; l < NL; l++) before.l[l] = pref_lds[i][l][threadIdx.x];
      const fe zinv = fe_mul<Fq>(inv, before);                                       // 1 / z_i
      inv = fe_mul<Fq>(inv, fe_mul<Fq>(one, fe_from_ext_lazy(zw)));
      const fe zi2 = fe_sqr<Fq>(zinv);
      const fe x = fq_plain(fe_mul<Fq>(zi2, fe_from_ext_lazy(xw)));                  // lazy loads are < 32p: 2 * 32 / 169 + 1 < 2p
      const fe y = fq_plain(fe_mul<Fq>(fe_mul<Fq>(zi2, zinv), fe_from_ext_lazy(yw)));
      fe_pack(x, ox);
      fe_pack(y, oy);
      g1_encoding_words(x, y, layout, oe);
    }
    store_words(o, ox);
    store_words(o + 8, oy);
    store_words(o + 16, oe);
  }
}

__global__ void __launch_bounds__(256) k_transcript_scalars(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  load_words(in + i * 8, w);
  fe_pack(fe_canon_lt2p<FrParams>(fe_mul<FrParams>(fe_const<FrParams>(FrParams::FROM_EXT_CANON), fe_unpack<0>(w))), w);   // s * 2^256 -> s
  store_words(out + i * 8, w);
}

__global__ void __launch_bounds__(256) k_transcript_affine(const uint32_t* __restrict__ pts, size_t n, uint32_t* __restrict__ out,
                                                           unsigned long long* __restrict__ first_bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const affine_words p = load_affine(pts, i);
  uint32_t ox[8] = {0, 0, 0, 0, 0, 0, 0, 0}, oy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (affine_is_identity(p)) {
    atomicMin(first_bad, (unsigned long long)i);
  } else {
    const fe from_ext = fe_const<Fq>(Fq::FROM_EXT_CANON);
    fe_pack(fe_canon_lt2p<Fq>(fe_mul<Fq>(from_ext, fe_unpack<0>(p.x))), ox);
    fe_pack(fe_canon_lt2p<Fq>(fe_mul<Fq>(from_ext, fe_unpack<0>(p.y))), oy);
  }
  store_words(out + i * 16, ox);
  store_words(out + i * 16 + 8, oy);
}

// d_ident: one uint32, zero before the launch, that the kernel adds the number of identity inputs to.  d_out: n x 24 words.  All pointers 16-byte aligned.
int transcript_points_device(const uint32_t* d_in, size_t n, uint32_t* d_out, int layout, uint32_t* d_ident, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  if (n > ((size_t)1 << 24)) { set_error("transcript: more than 2^24 points in one call"); return ZKHIP_EINVAL; }
  const uint32_t ch = transcript_chunk(n);
  const size_t threads = (n + ch - 1) / ch;
  hipLaunchKernelGGL(k_transcript_points, dim3((unsigned)((threads + TR_BLOCK - 1) / TR_BLOCK)), dim3(TR_BLOCK), 0, stream, d_in, (uint32_t)n, d_out, ch, layout,
                     d_ident);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

int transcript_scalars_device(const uint32_t* d_in, size_t n, uint32_t* d_out, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  if (n > ((size_t)1 << 26)) { set_error("transcript: more than 2^26 scalars in one call"); return ZKHIP_EINVAL; }
  hipLaunchKernelGGL(k_transcript_scalars, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_in, n, d_out);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

// d_first_bad must hold a value >= n before the launch
int transcript_affine_device(const uint32_t* d_points, size_t n, uint32_t* d_out, unsigned long long* d_first_bad, hipStream_t stream) {
  if (n == 0) return ZKHIP_OK;
  hipLaunchKernelGGL(k_transcript_affine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_points, n, d_out, d_first_bad);
  HIPCHK(hipGetLastError());
  return ZKHIP_OK;
}

}  // namespace zkhip

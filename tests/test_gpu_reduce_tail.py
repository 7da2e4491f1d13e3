"""GPU: the tail of the bucket reduction (csrc/msm.hip: msm_reduce_buckets, k_pyramid_pair_quad, k_reduce_finish; csrc/reduce_plan.hpp).

Up to 64 bucket sets are reduced by single-lane steps, then quad steps two levels per launch, then one workgroup per set that runs the last
levels in LDS, the weighted sum laid out by chain length, and the store.  The tables are forced to a window size with
`zkhip_prepare_bases_device_c`, so n stays at 2^10 + 3 points while the MSM still reduces all 2^(c-1) buckets, and every result is compared
as an affine point with the structured identity of the walk bases as bench.py computes it (`structured_point`: polynomial evaluations and
one fixed-base multiplication, no MSM kernel and no oracle).  Every case asserts that the expected point is not the identity."""
import ctypes as C

import numpy as np
import pytest

import bench
from zksnap_circuits_halo2_amd import _lib, fields as F

pytestmark = pytest.mark.gpu
D = 0x9E3779B97F4A7C15F39CC0605CEDC835
T0 = 0x5A4B534E41500002 + 2727
N = (1 << 10) + 3


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _walk(lib, torch, n, t0, d=D):
    bases = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    t0m, dm = F.fr_encode([t0])[0], F.fr_encode([d])[0]
    _lib.check(lib.zkhip_g1_gen_walk_device(t0m.ctypes.data, dm.ctypes.data, n, bases.data_ptr(), None))
    torch.cuda.synchronize()
    return bases


def _want(lib, torch, dsc, n, t0, d=D):
    want = bench.structured_point(lib, _lib, F, torch, dsc, n, t0 % F.R_MOD, d, _stream(torch), torch.device("cuda", torch.cuda.current_device()))
    assert want.any(), "the structured identity of these scalars is the point at infinity: the case checks nothing"
    return want


def _affine(lib, words):
    return bench.affine_words(lib, _lib, np.ascontiguousarray(words).view(np.uint64)[:12])[0]


class Tables:
    """tables of one base array, one per forced window size, built on first use and released together"""

    def __init__(self, lib, torch, t0, d):
        self.lib, self.t0, self.d, self.handles = lib, t0, d, {}
        self.bases = _walk(lib, torch, N, t0, d)

    def get(self, c):
        if c not in self.handles:
            h = C.c_uint64(0)
            _lib.check(self.lib.zkhip_prepare_bases_device_c(self.bases.data_ptr(), N, c, C.byref(h)))
            assert self.lib.zkhip_prepared_window_bits(h) == c
            self.handles[c] = h
        return self.handles[c]

    def release(self):
        for h in self.handles.values():
            _lib.check(self.lib.zkhip_release_bases(h))


@pytest.fixture(scope="module")
def walk_tables(lib):
    import torch

    t = Tables(lib, torch, T0, D)
    yield t
    t.release()


@pytest.fixture(scope="module")
def equal_tables(lib):
    """step d = 0: every base is the same point T0 G"""
    import torch

    t = Tables(lib, torch, T0, 0)
    yield t
    t.release()


def _check_prepared(lib, tables, c, sc):
    import torch

    dsc = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_msm_g1_prepared_device(tables.get(c), 0, dsc.data_ptr(), N, out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    want = _want(lib, torch, dsc, N, tables.t0, tables.d)
    assert np.array_equal(_affine(lib, out.cpu().numpy()), want)


def _sparse(values):
    """N scalars: the given integers first, zeros behind them"""
    sc = np.zeros((N, 4), dtype=np.uint64)
    sc[:len(values)] = F.fr_encode(list(values))
    return sc


@pytest.mark.parametrize("c", [20, 19, 17, 16, 13, 8, 5, 3, 2])
def test_window_sizes(lib, walk_tables, c):
    """c = 20: four single-lane steps, three quad steps, four pairs, the finish from step 16; 19: three pairs between quad steps (one left
    over behind them); 17 and 16: quad steps, then four pairs; 13: three pairs from the first step and one quad step left over; 8 and below:
    the finish kernel alone -- with 6, 3 and 1 levels, and with none at all (c = 2: two buckets, X0 + 2 X1)"""
    _check_prepared(lib, walk_tables, c, bench.synth_scalars(N, 0x27A0 + c))


@pytest.mark.parametrize("l", list(range(19)))
def test_one_bit_at_a_time(lib, walk_tables, l):
    """c = 20; every scalar is 2^l or 2^l + 1: window 0 alone has a non-zero digit, in buckets 2^l - 1 and 2^l, so the Z^l row (and for
    l = 18 the 2^nz X1 term) carries the result alone"""
    vals = [(1 << l) + (i & 1) for i in range(N)]
    _check_prepared(lib, walk_tables, 20, F.fr_encode(vals))


def test_top_bucket_and_bucket_zero(lib, walk_tables):
    """2^19 recodes to the digit -2^19 (the top bucket, negated) and a carry of 1 into window 1 (bucket 0); 1 is bucket 0 of window 0"""
    vals = [(1 << 19) if i % 3 else 1 for i in range(N)]
    _check_prepared(lib, walk_tables, 20, F.fr_encode(vals))


# Buckets k and k + 1 with k + 1 = 2^m (odd multiple) hold the two halves of one X addition of step m + 1.  At c = 20: step 1 is a
# single-lane step, 5 a quad step, 8 / 9 the first / second addition of a pair launch, 13 and 14 the second addition of one pair and the
# first of the next, 16 and 18 the first and the last level of the finish kernel.
MERGE_STEPS = [1, 5, 8, 9, 13, 14, 16, 18]


@pytest.mark.parametrize("step", MERGE_STEPS)
def test_equal_operands_take_the_doubling_branch(lib, equal_tables, step):
    """all bases equal, one scalar 2^m and one 2^m + 1 (m = step - 1): buckets 2^m - 1 and 2^m both hold the base point"""
    m = step - 1
    _check_prepared(lib, equal_tables, 20, _sparse([1 << m, (1 << m) + 1]))


@pytest.mark.parametrize("step", MERGE_STEPS)
def test_opposite_operands_give_the_identity(lib, equal_tables, step):
    """all bases equal: 2^m puts the base point P into bucket 2^m - 1, and 2^20 - (2^m + 1) recodes to the digit -(2^m + 1) -- -P in bucket
    2^m -- with a carry into window 1 (2^20 P in bucket 0): the X addition of step m + 1 is P + (-P) (at step 1, where bucket 0 is one of the
    two, it is (P + 2^20 P) + (-P))"""
    m = step - 1
    _check_prepared(lib, equal_tables, 20, _sparse([1 << m, (1 << 20) - ((1 << m) + 1)]))


@pytest.mark.parametrize("k", [0, 1 << 12, 1 << 18])
def test_adjacent_and_negated_scalars(lib, equal_tables, k):
    """all bases equal, scalars k + 1 and k + 2 (adjacent buckets), then k + 1 and r - (k + 2) (the sum is -P)"""
    _check_prepared(lib, equal_tables, 20, _sparse([k + 1, k + 2]))
    _check_prepared(lib, equal_tables, 20, _sparse([k + 1, F.R_MOD - (k + 2)]))


def test_general_path(lib):
    """unregistered bases: GLV, a bucket set per window (WB = W sets in the finish kernel's grid), then k_fold"""
    import torch

    bases = _walk(lib, torch, N, T0 + 1)
    dsc = torch.from_numpy(bench.synth_scalars(N, 0x27B0).view(np.int64)).cuda()
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_msm_g1_device(dsc.data_ptr(), bases.data_ptr(), N, out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    assert np.array_equal(_affine(lib, out.cpu().numpy()), _want(lib, torch, dsc, N, T0 + 1))


def _check_batch(lib, tables, c, batch, seed):
    import torch

    stride = N + 5
    dsc = torch.from_numpy(bench.synth_scalars(stride * batch, seed).view(np.int64)).cuda().reshape(-1)
    out = torch.zeros(12 * batch, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_msm_g1_prepared_batch_device(tables.get(c), 0, dsc.data_ptr(), N, batch, stride, out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    got = bench.affine_words(lib, _lib, out.cpu().numpy().view(np.uint64).reshape(batch, 12))
    for b in range(batch):
        want = _want(lib, torch, dsc[b * stride * 4:(b * stride + N) * 4], N, tables.t0)
        assert np.array_equal(got[b], want), b


def test_batched_prepared_call(lib, walk_tables):
    """5 vectors at c = 13: five bucket sets in every launch's grid (a quad step, three pairs, the finish)"""
    _check_batch(lib, walk_tables, 13, 5, 0x27B1)


@pytest.mark.parametrize("batch", [64, 65])
def test_bucket_sets_at_the_bound_of_the_finish_kernel(lib, walk_tables, batch):
    """64 sets: the finish kernel alone (c = 8); 65: a launch per level and the weighted-sum kernel, as before"""
    _check_batch(lib, walk_tables, 8, batch, 0x27B2 + batch)


def test_more_bucket_sets_than_the_quad_weighted_sum_takes(lib):
    """2049 vectors at c = 7, (B, WB) = (64, 2049): steps 1 and 2 are single-lane steps (48 x 2049 and 32 x 2049 additions exceed 65536),
    steps 3 - 5 quad steps, then the single-lane k_window_horner and k_store_results, every launch with 2049 grid rows.  The table has its
    own walk of 2^6 + 3 bases, so the sort sees about 5 M entries.  Rows 0, 1024, 2047 and 2048 carry vectors of their own; every other
    row carries one shared vector, checked once against its identity and compared with the rest for equality."""
    import torch

    n, c, batch, t0 = (1 << 6) + 3, 7, 2049, T0 + 3
    own = [0, 1024, 2047, 2048]
    sc = np.broadcast_to(bench.synth_scalars(n, 0x27C0), (batch, n, 4)).copy()
    for i, b in enumerate(own):
        sc[b] = bench.synth_scalars(n, 0x27C1 + i)
    bases = _walk(lib, torch, n, t0)
    dsc = torch.from_numpy(sc.view(np.int64)).cuda().reshape(-1)
    out = torch.zeros(12 * batch, dtype=torch.int64, device="cuda")
    h = C.c_uint64(0)
    _lib.check(lib.zkhip_prepare_bases_device_c(bases.data_ptr(), n, c, C.byref(h)))
    try:
        assert lib.zkhip_prepared_window_bits(h) == c
        _lib.check(lib.zkhip_msm_g1_prepared_batch_device(h, 0, dsc.data_ptr(), n, batch, n, out.data_ptr(), _stream(torch)))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.zkhip_release_bases(h))
    got = bench.affine_words(lib, _lib, out.cpu().numpy().view(np.uint64).reshape(batch, 12))
    for b in own + [1]:                                  # row 1 stands for the shared vector
        assert np.array_equal(got[b], _want(lib, torch, dsc[b * n * 4:(b + 1) * n * 4], n, t0)), b
    rest = np.delete(got, own, axis=0)
    assert rest.shape[0] == batch - len(own) and (rest == rest[0]).all()


def test_chunked_host_buffer_call(lib):
    """zkhip_msm_g1 on registered bases at 2^21 scalars: two pieces accumulated into one bucket set, reduced once (msm_chunk_finish)"""
    import torch

    n = 1 << 21
    bases = np.ascontiguousarray(_walk(lib, torch, n, T0 + 2).cpu().numpy().view(np.uint64).reshape(n, 8))
    sc = bench.synth_scalars(n, 0x27B3)
    out = np.zeros(12, dtype=np.uint64)
    _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
    try:
        _lib.check(lib.zkhip_msm_g1(sc.ctypes.data, bases.ctypes.data, n, out.ctypes.data))
    finally:
        _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
    dsc = torch.from_numpy(sc.view(np.int64)).cuda()
    assert np.array_equal(_affine(lib, out), _want(lib, torch, dsc, n, T0 + 2))

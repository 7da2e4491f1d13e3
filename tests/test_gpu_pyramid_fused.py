"""GPU: steps 1 - 4 of the bucket reduction, the chip-wide ones, of which steps 1 and 2 go in one launch where that launch is one round of two
wavefronts per SIMD (csrc/msm.hip: k_pyramid_pair, msm_reduce_buckets; csrc/reduce_plan.hpp), in the pattern of
tests/test_gpu_reduce_tail.py: 2^10 + 3 walk bases, tables forced to a window size, every result compared as an affine point with the
structured identity of the bases (`bench.structured_point`), every expected point checked not to be the identity.  The cases are chosen by
the steps they reach, not by which of them a build fuses: they hold for single steps as well.  One bucket set of 2^19 (c = 20) and the
batched call at c = 16 with 16 vectors (16 sets of 2^15 as grid rows) both fuse steps 1 + 2 in a launch of 2^17 lanes, so the cases on single
additions run in both shapes; steps 3 and 4 are single launches in every shape (a fused launch of them was measured and not kept).

Bucket k holds the points of digit k + 1, and is element k of X at step 1.  With 8g the first bucket of a group of eight, the two launches
that would replace steps 1 + 2 and steps 3 + 4 add (the single steps add the same operands):
  steps 1 + 2, X lane t = 2g (even) and 2g + 1 (odd), j = bucket - 8g:
      a = X[4t] + X[4t+1]        buckets (0, 1), (4, 5)          b = X[4t+2] + X[4t+3]      buckets (2, 3), (6, 7)
      z = X[4t+1] + X[4t+3]      buckets (1, 3), (5, 7)          X''[t] = a + b             buckets (0, 2), (1, 2) ...
      even lane: z(2g) + z(2g+1) buckets (1, 5), (3, 7)          odd lane: b(2g) + b(2g+1)  buckets (2, 6), (3, 6)
  steps 3 + 4: X element j of step 3 is the sum of buckets 4j .. 4j+3, so the same eight pairs with every bucket number times 4;
      Z^0[w] of step 3 is the sum of buckets 8w + {1, 3, 5, 7}, Z^1[w] that of buckets 8w + {2, 3, 6, 7}; the Z lane u adds
      (Z[4u] + Z[4u+1]) + (Z[4u+2] + Z[4u+3]): buckets 32u + (1, 9), (17, 25), (1, 17) for Z^0 and 32u + (2, 10), (18, 26), (2, 18) for Z^1.
All pairs are taken in the group that starts at bucket 32 (g = 4, u = 1), so bucket 0, which also receives the carry of a negated digit, stays
out of them."""
import numpy as np
import pytest

import bench
from zksnap_circuits_halo2_amd import _lib, fields as F
from test_gpu_reduce_tail import N, T0, D, Tables, _affine, _check_batch, _check_prepared, _sparse, _stream, _walk, _want

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def walk_tables(lib):
    import torch

    t = Tables(lib, torch, T0 + 30, D)
    yield t
    t.release()


@pytest.fixture(scope="module")
def equal_tables(lib):
    """step d = 0: every base is the same point (T0 + 30) G"""
    import torch

    t = Tables(lib, torch, T0 + 30, 0)
    yield t
    t.release()


def _check_rows(lib, tables, c, rows):
    """the batched call on one scalar vector per row, every result against its own structured identity"""
    import torch

    stride = N + 5
    buf = np.zeros((stride * len(rows), 4), dtype=np.uint64)
    for b, r in enumerate(rows):
        buf[b * stride:b * stride + N] = r
    dsc = torch.from_numpy(buf.view(np.int64)).cuda().reshape(-1)
    out = torch.zeros(12 * len(rows), dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_msm_g1_prepared_batch_device(tables.get(c), 0, dsc.data_ptr(), N, len(rows), stride, out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    got = bench.affine_words(lib, _lib, out.cpu().numpy().view(np.uint64).reshape(len(rows), 12))
    for b in range(len(rows)):
        want = _want(lib, torch, dsc[b * stride * 4:(b * stride + N) * 4], N, tables.t0, tables.d)
        assert np.array_equal(got[b], want), b


SHAPES = ["c = 20", "c = 16, 16 vectors"]


def _check_shape(lib, tables, shape, scalars_of_c):
    """c = 20: one call; the batch: the scalars in the first and the last bucket set, one point each in the 14 sets between them"""
    if shape == "c = 20":
        _check_prepared(lib, tables, 20, scalars_of_c(20))
    else:
        sc = scalars_of_c(16)
        _check_rows(lib, tables, 16, [sc] + [_sparse([b + 3]) for b in range(14)] + [sc])


@pytest.mark.parametrize("c", [20, 19, 18])
def test_window_sizes_around_the_fused_steps(lib, walk_tables, c):
    """c = 20: four single-lane entries (steps 1 + 2 in one launch of 2^17 lanes, 3 and 4 single); 19: three (the launch would have 2^16
    lanes: single steps); 18: one, nothing to fuse"""
    _check_prepared(lib, walk_tables, c, bench.synth_scalars(N, 0x3000 + c))


def _uniform(lo, hi, seed, keep=lambda v: True):
    rng = np.random.default_rng(seed)
    pool = [v for v in range(lo, hi + 1) if keep(v)]
    return F.fr_encode([pool[i] for i in rng.integers(0, len(pool), size=N)])


DENSE = {      # (range of digits: the first 2^6 or the last 2^6 and B itself, buckets kept)
    "first lanes": (False, lambda k: True),
    "last lanes, the top bucket and its carry": (True, lambda k: True),
    "first lanes, buckets of Z^0 (odd buckets)": (False, lambda k: k % 2 == 1),
    "last lanes, buckets of Z^0": (True, lambda k: k % 2 == 1),
    "first lanes, buckets of Z^1 (2 and 3 of four)": (False, lambda k: k % 4 >= 2),
    "last lanes, buckets of Z^1": (True, lambda k: k % 4 >= 2),
}


@pytest.mark.parametrize("c", [20, 19])
@pytest.mark.parametrize("case", list(DENSE))
def test_dense_buckets(lib, walk_tables, c, case):
    """1027 scalars uniform in a range of 2^6 digits of window 0: ~16 points per bucket, so every addition of the lanes that own these
    buckets is a general one (random 254-bit scalars leave almost every bucket empty and reach the identity branches only).  With
    B = 2^(c-1) buckets, the scalar B itself recodes to the negated top bucket and a carry into window 1.  The rows Z^0 and Z^1 that steps
    3 and 4 reduce are fed by the odd buckets and by buckets 2 and 3 of every four."""
    top, keep = DENSE[case]
    B = 1 << (c - 1)
    lo, hi = (B - (1 << 6), B) if top else (1, 1 << 6)
    _check_prepared(lib, walk_tables, c, _uniform(lo, hi, 0x3100 + c, lambda v: keep(v - 1)))


G = 32
X12 = [(0, 1), (2, 3), (1, 3), (0, 2), (1, 5), (3, 7), (2, 6), (3, 6)]          # a, b, z, a + b, even lane (two), odd lane (two)
PAIRS = ([("steps 1 + 2", G + i, G + j) for i, j in X12] + [("steps 3 + 4, X", G + 4 * i, G + 4 * j) for i, j in X12]
         + [("steps 3 + 4, Z^0", G + i, G + j) for i, j in [(1, 9), (17, 25), (1, 17)]]
         + [("steps 3 + 4, Z^1", G + i, G + j) for i, j in [(2, 10), (18, 26), (2, 18)]])
PAIR_IDS = [f"{what}: buckets {i}, {j}" for what, i, j in PAIRS]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("what,i,j", PAIRS, ids=PAIR_IDS)
def test_bucket_pair_with_equal_operands(lib, equal_tables, what, i, j, shape):
    """all bases equal: scalars i + 1 and j + 1 put the base point into buckets i and j alone, which meet in the named addition as P + P"""
    _check_shape(lib, equal_tables, shape, lambda c: _sparse([i + 1, j + 1]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("what,i,j", PAIRS, ids=PAIR_IDS)
def test_bucket_pair_with_opposite_operands(lib, equal_tables, what, i, j, shape):
    """all bases equal: i + 1 puts P into bucket i, 2^c - (j + 1) recodes to the digit -(j + 1) -- -P in bucket j -- with a carry into
    window 1 (2^c P in bucket 0, which keeps the result off the identity): the named addition is P + (-P)"""
    _check_shape(lib, equal_tables, shape, lambda c: _sparse([i + 1, (1 << c) - (j + 1)]))


@pytest.mark.parametrize("step", [2, 3, 4])
def test_merge_steps(lib, equal_tables, step):
    """buckets 2^m - 1 and 2^m (m = step - 1) hold the two halves of one X addition of step m + 1: equal, then opposite (the steps of
    test_gpu_reduce_tail.MERGE_STEPS that lie among steps 1 - 4 are step 1 only)"""
    m = step - 1
    _check_prepared(lib, equal_tables, 20, _sparse([1 << m, (1 << m) + 1]))
    _check_prepared(lib, equal_tables, 20, _sparse([1 << m, (1 << 20) - ((1 << m) + 1)]))


@pytest.mark.parametrize("c", [20, 19])
@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_one_bit_at_a_time(lib, walk_tables, c, l):
    """every scalar is 2^l or 2^l + 1: buckets 2^l - 1 and 2^l, so row Z^l -- one of the rows created inside the launches of steps 1 - 4 --
    carries the result alone"""
    _check_prepared(lib, walk_tables, c, F.fr_encode([(1 << l) + (i & 1) for i in range(N)]))


def test_dense_buckets_in_every_set_of_a_batch(lib, walk_tables):
    """c = 16, 16 vectors: the fused launch with bucket sets as grid rows, every set with its own scalars, four sets for each of the first
    four cases above"""
    rows = []
    for b in range(16):
        top, keep = list(DENSE.values())[b % 4]
        lo, hi = ((1 << 15) - (1 << 6), 1 << 15) if top else (1, 1 << 6)
        rows.append(_uniform(lo, hi, 0x3180 + b, lambda v: keep(v - 1)))
    _check_rows(lib, walk_tables, 16, rows)


def test_dense_z_rows_in_a_batch(lib, walk_tables):
    """the same with the buckets that feed Z^0 and Z^1 (the last four cases above): the rows steps 1 and 2 create and steps 3 and 4 reduce"""
    rows = []
    for b in range(16):
        top, keep = list(DENSE.values())[2 + b % 4]
        lo, hi = ((1 << 15) - (1 << 6), 1 << 15) if top else (1, 1 << 6)
        rows.append(_uniform(lo, hi, 0x31C0 + b, lambda v: keep(v - 1)))
    _check_rows(lib, walk_tables, 16, rows)


@pytest.mark.parametrize("c,batch", [(16, 8), (16, 16), (16, 32), (13, 64), (13, 65)])
def test_batched_prepared_call(lib, walk_tables, c, batch):
    """bucket sets as grid rows: c = 16 with 8 vectors has three single-lane entries (2^16 lanes: not fused), with 16 vectors four (steps
    1 + 2 fused: 2^17 lanes) and with 32 vectors five (2^18 lanes, two rounds: not fused); c = 13 with 64 sets has three (2^16 lanes) and
    ends in the finish kernel, with 65 sets it keeps a launch per level and the weighted-sum kernel"""
    _check_batch(lib, walk_tables, c, batch, 0x3200 + batch)


def test_chunked_host_buffer_call(lib):
    """zkhip_msm_g1 on registered bases at 2^21 scalars: two pieces accumulated into one bucket set, reduced once (msm_chunk_finish)"""
    import torch

    n = 1 << 21
    bases = np.ascontiguousarray(_walk(lib, torch, n, T0 + 31).cpu().numpy().view(np.uint64).reshape(n, 8))
    sc = bench.synth_scalars(n, 0x3300)
    out = np.zeros(12, dtype=np.uint64)
    _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
    try:
        _lib.check(lib.zkhip_msm_g1(sc.ctypes.data, bases.ctypes.data, n, out.ctypes.data))
    finally:
        _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
    dsc = torch.from_numpy(sc.view(np.int64)).cuda()
    assert np.array_equal(_affine(lib, out), _want(lib, torch, dsc, n, T0 + 31))


def test_general_path_with_two_single_lane_entries(lib):
    """unregistered bases: a bucket set per window.  Step 2 has B / 2 additions per set, so two adjacent single-lane entries need
    W B / 2 > 65536: the smallest window of the general path that has them is c = 15 (B = 2^14, W = 9), and the smallest n is the first
    whose window is that wide (about 150 000 points: a multiple of 2^12 is close enough)"""
    import torch

    n = next(k << 12 for k in range(1, 1 << 8) if lib.zkhip_msm_window_bits(k << 12) >= 15)
    c = lib.zkhip_msm_window_bits(n)
    assert (1 << (c - 2)) * -(-127 // c) > 65536 and n < (1 << 18)
    bases = _walk(lib, torch, n, T0 + 32)
    dsc = torch.from_numpy(bench.synth_scalars(n, 0x3400).view(np.int64)).cuda()
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_msm_g1_device(dsc.data_ptr(), bases.data_ptr(), n, out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    assert np.array_equal(_affine(lib, out.cpu().numpy()), _want(lib, torch, dsc, n, T0 + 32))

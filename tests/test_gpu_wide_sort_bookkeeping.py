"""GPU: the head of the wide prepared MSM (csrc/msm.hip: k_coarse_sorted, k_fine_sorted, k_scan_apply2, k_make_order).

The sorts keep a lane's entries in registers and place them by the rank the histogram's atomic returned; k_scan_apply2 merges the task-length
histogram; k_make_order scans it and writes the task records, the heavy-bucket list and the largest task count of a bucket.
The wide path needs a table of c > 16, so n is the smallest size `msm_pick_window_prepared` sends there (2^20), and every result is compared
with the structured identity of the walk bases as bench.py computes it (`structured_point`: polynomial evaluations and one fixed-base
multiplication, no MSM kernel and no oracle).  The scalar distributions are the ones that steer those kernels down their different branches;
the last two tests run the same shared kernels from the batched prepared path and from the general (GLV) path."""
import ctypes as C

import numpy as np
import pytest

import bench
from zksnap_circuits_halo2_amd import _lib, fields as F

pytestmark = pytest.mark.gpu
D = 0x9E3779B97F4A7C15F39CC0605CEDC835
T0 = 0x5A4B534E41500002 + 2020
N = 1 << 20
TOTAL = N + 8                     # registered points: room for n = 2^20 + 5 at offset 3


def _win_offsets():
    """bit offsets of the 13 balanced windows of c = 20 (msm.hip win_off): nine of 20 bits, then four of 19"""
    full = 9
    return [w * 20 if w <= full else full * 20 + (w - full) * 19 for w in range(13)]


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _walk(lib, torch, n, t0):
    bases = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    t0m, dm = F.fr_encode([t0])[0], F.fr_encode([D])[0]
    _lib.check(lib.zkhip_g1_gen_walk_device(t0m.ctypes.data, dm.ctypes.data, n, bases.data_ptr(), None))
    torch.cuda.synchronize()
    return bases


def _want(lib, torch, dsc, n, t0):
    return bench.structured_point(lib, _lib, F, torch, dsc, n, t0 % F.R_MOD, D, _stream(torch), torch.device("cuda", torch.cuda.current_device()))


def _got(lib, torch, out):
    torch.cuda.synchronize()
    return bench.affine_words(lib, _lib, out.cpu().numpy().view(np.uint64)[:12])[0]


def _digit_scalars(rng, n, hi, pool=1 << 14):
    """n scalars (Montgomery limbs) whose 13 window digits all lie in [1, hi] (hi < 2^18: no signed-recoding carry; the top window, from
    bit 237, in [1, min(hi, 2^16)]: below r), drawn from a pool of `pool` distinct values -- the Montgomery conversion runs on Python integers"""
    offs = _win_offsets()
    digs = rng.integers(1, hi + 1, size=(pool, 13))
    digs[:, 12] = rng.integers(1, min(hi, 1 << 16) + 1, size=pool)
    vals = [sum(int(d) << o for d, o in zip(row, offs)) for row in digs]
    assert max(vals) < F.R_MOD
    enc = F.fr_encode(vals)
    return np.ascontiguousarray(enc[rng.integers(0, pool, size=n)])


@pytest.fixture(scope="module")
def table(lib):
    import torch

    bases = _walk(lib, torch, TOTAL, T0)
    h = C.c_uint64(0)
    _lib.check(lib.zkhip_prepare_bases_device(bases.data_ptr(), TOTAL, C.byref(h)))
    assert lib.zkhip_prepared_window_bits(h) == 20
    yield h
    _lib.check(lib.zkhip_release_bases(h))


def _check_prepared(lib, table, sc, n=N, off=0):
    import torch

    dsc = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_msm_g1_prepared_device(table, off, dsc.data_ptr(), n, out.data_ptr(), _stream(torch)))
    got = _got(lib, torch, out)
    want = _want(lib, torch, dsc, n, T0 + off * D)
    assert want.any(), "the structured identity of these scalars is the point at infinity: the case checks nothing"
    assert np.array_equal(got, want)


def test_uniform_scalars(lib, table):
    """~26 entries in every bucket: nearly every bucket is one task that the accumulation writes itself"""
    _check_prepared(lib, table, bench.synth_scalars(N, 0x20A1))


def test_all_scalars_equal_one_heavy_bucket(lib, table):
    """the same digit in all 13 windows: ONE bucket holds 13 * 2^20 entries (212992 tasks, 104 heavy slices, order records written by whole
    wavefronts), every other bucket is empty and must read as the identity"""
    s = sum(0x1234 << o for o in _win_offsets())
    _check_prepared(lib, table, np.ascontiguousarray(np.broadcast_to(F.fr_encode([s])[0], (N, 4))))


def test_sixty_percent_zeros_and_empty_groups(lib, table):
    """60 % zero scalars; the others have all digits in [1, 2^18 - 1]: the upper 64 groups of 4096 buckets stay empty as a whole"""
    rng = np.random.default_rng(0x20A3)
    sc = _digit_scalars(rng, N, (1 << 18) - 1)
    sc[rng.integers(0, 10, size=N) < 6] = 0
    _check_prepared(lib, table, sc)


def test_all_digits_in_one_group(lib, table):
    """every digit in [1, 4096]: 13 * 2^20 entries in group 0 -- 476 chunks of one group, 3328 entries = 52 tasks per bucket (all 4096 on the
    heavy list), 127 empty groups"""
    _check_prepared(lib, table, _digit_scalars(np.random.default_rng(0x20A4), N, 4096))


def test_ragged_length_at_an_offset(lib, table):
    """n = 2^20 + 5 from point 3 of the registered array: a ragged last chunk in every kernel of the sort"""
    _check_prepared(lib, table, bench.synth_scalars(N + 5, 0x20A5), n=N + 5, off=3)


def test_batched_prepared_call(lib):
    """5 vectors of 8191 scalars on a narrow-window table: 5 bucket sets in one launch set, above the single-workgroup scan"""
    import torch

    n, batch, stride = 8191, 5, 8191 + 5
    bases = _walk(lib, torch, n, T0 + 5)
    h = C.c_uint64(0)
    _lib.check(lib.zkhip_prepare_bases_device(bases.data_ptr(), n, C.byref(h)))
    try:
        dsc = torch.from_numpy(bench.synth_scalars(stride * batch, 0x20A6).view(np.int64)).cuda().reshape(-1)
        out = torch.zeros(12 * batch, dtype=torch.int64, device="cuda")
        _lib.check(lib.zkhip_msm_g1_prepared_batch_device(h, 0, dsc.data_ptr(), n, batch, stride, out.data_ptr(), _stream(torch)))
        torch.cuda.synchronize()
        res = out.cpu().numpy().view(np.uint64).reshape(batch, 12)
        for b in range(batch):
            want = _want(lib, torch, dsc[b * stride * 4:(b * stride + n) * 4], n, T0 + 5)
            assert np.array_equal(bench.affine_words(lib, _lib, res[b])[0], want), b
    finally:
        _lib.check(lib.zkhip_release_bases(h))


def test_general_path_glv_2p18(lib):
    """unregistered bases at 2^18: GLV digits, the two-level sort at c = 16 with a bucket set per window (2^18 buckets)"""
    import torch

    n = 1 << 18
    bases = _walk(lib, torch, n, T0 + 18)
    dsc = torch.from_numpy(bench.synth_scalars(n, 0x20A7).view(np.int64)).cuda()
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_msm_g1_device(dsc.data_ptr(), bases.data_ptr(), n, out.data_ptr(), _stream(torch)))
    assert np.array_equal(_got(lib, torch, out), _want(lib, torch, dsc, n, T0 + 18))

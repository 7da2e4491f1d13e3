"""GPU: the head of the wide prepared MSM (csrc/msm.hip, csrc/msm_digits.hpp): digits, group offsets, bucket runs, task records.

k_digits_wide<20, 13, 4> recodes from the canonical limbs with constant offsets (every other layout runs the generic instantiation);
k_group_offsets scans the group counts from registers; k_fine_sorted writes bucket runs from one or several chunks of a group, and
k_make_order gathers the first point reference of every task from them (three columns below steer those two: runs of one bucket from two
workgroups, a bucket of many tasks, a heavy bucket).
Tables are forced to a window size with `zkhip_prepare_bases_device_c`, so n stays at 2^12 + 3 points (three padding entries per digit row)
while c = 20 runs the specialised kernel and c = 18 the generic one.  Every affine result is compared with the same MSM on a c = 16 table
(int16 digits from k_digits and the one-level sort: only the conversion is shared) and with the oracle's `best_multiexp`; the oracle itself is checked against the
structured identity of its walk bases, sum_i s_i (t0 + i d) G, so a case passes only if both references agree with each other first."""
import ctypes as C

import numpy as np
import pytest

from zksnap_circuits_halo2_amd import _lib, fields as F

pytestmark = pytest.mark.gpu
N = (1 << 12) + 3
WIDE = (20, 18)                     # the specialised layout (20, 13, 4) and a generic one (18, 15, 14)
R = F.R_MOD
OFFS = [w * 20 if w <= 9 else 180 + (w - 9) * 19 for w in range(13)]          # msm_digits.hpp win_off for (20, 13, 4)
BITS = [20] * 9 + [19] * 4
TOP_MAX = R >> OFFS[12]             # the top window of r


class Setup:
    def __init__(self, lib, cref):
        import torch

        self.lib, self.cref, self.torch = lib, cref, torch
        self.bases, self.t0, self.d = cref.gen_bases(0x5A4B534E41500034, N)
        self.dbases = torch.from_numpy(self.bases.view(np.int64)).cuda()
        self.handles = {}
        for c in WIDE + (16,):
            h = C.c_uint64(0)
            _lib.check(lib.zkhip_prepare_bases_device_c(self.dbases.data_ptr(), N, c, C.byref(h)))
            assert lib.zkhip_prepared_window_bits(h) == c
            self.handles[c] = h

    def msm(self, c, dsc):
        torch = self.torch
        out = torch.zeros(12, dtype=torch.int64, device="cuda")
        _lib.check(self.lib.zkhip_msm_g1_prepared_device(self.handles[c], 0, dsc.data_ptr(), N, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return F.g1_decode_jacobian(out.cpu().numpy().view(np.uint64))

    def release(self):
        for h in self.handles.values():
            _lib.check(self.lib.zkhip_release_bases(h))


@pytest.fixture(scope="module")
def setup(lib, cref):
    s = Setup(lib, cref)
    yield s
    s.release()


def _check(setup, values):
    """values: N canonical integers below r"""
    assert len(values) == N and all(0 <= v < R for v in values)
    sc = np.ascontiguousarray(F.fr_encode(values))
    cref = setup.cref
    oracle = F.g1_decode_jacobian(cref.best_multiexp(sc, setup.bases, 4))
    k = sum(v * (setup.t0 + i * setup.d) for i, v in enumerate(values)) % R
    structured = F.g1_decode_jacobian(cref.scalar_mul(k, cref.generator()))
    assert oracle == structured, "the two references disagree: the case checks nothing"
    assert oracle is not None, "the expected point is the identity: the case checks nothing"
    dsc = setup.torch.from_numpy(sc.view(np.int64)).cuda()
    narrow = setup.msm(16, dsc)
    for c in WIDE:
        got = setup.msm(c, dsc)
        assert got == narrow, f"c = {c} differs from the c = 16 table"
        assert got == oracle, f"c = {c} differs from the oracle"


def _edge_scalars():
    e = [0, 1, R - 1, (R - 1) // 2]
    for k in OFFS[1:]:
        e += [1 << k, (1 << k) - 1, 1 << (k - 1), (1 << k) + 1]
    for top in (0, 1, TOP_MAX - 1):
        for delta in (-1, 0):     # every window 2^(cw-1) - 1: none carries; 2^(cw-1): the carry runs through all 13 windows
            e.append((top << OFFS[12]) + sum(((1 << (BITS[w] - 1)) + delta) << OFFS[w] for w in range(12)))
    e += [(top << OFFS[12]) + (1 << OFFS[12]) - 1 for top in (0, TOP_MAX - 1)]       # every window carries into the next, the top one takes it
    e.append(((TOP_MAX - 1) << OFFS[12]) + (1 << (OFFS[12] - 1)))                     # only the window below the top carries
    assert all(0 <= v < R for v in e)
    return e


def test_edge_scalars(setup):
    """the host check's scalars (tests/cpp/digits_host_check.cpp), repeated over the N points"""
    e = _edge_scalars()
    _check(setup, [e[i % len(e)] for i in range(N)])


def test_edge_and_random_scalars(setup):
    rng = np.random.default_rng(0x3401)
    e = _edge_scalars()
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(N)]
    for i, v in enumerate(e):
        vals[(i * 37) % N] = v
    _check(setup, vals)


def test_every_digit_in_group_zero(setup):
    """digits in [1, 4096] in all 13 windows of the (20, 13, 4) layout: 13 * N = 53 287 staged entries in coarse group 0, more than one
    chunk of 28 672, so a bucket's runs come from two workgroups of k_fine_sorted and only one of them holds its first reference
    (13 entries per bucket: four tasks of 4)"""
    rng = np.random.default_rng(0x3402)
    digs = rng.integers(1, 4097, size=(N, 13))
    _check(setup, [sum(int(d) << o for d, o in zip(row, OFFS)) for row in digs])


def test_one_bucket_of_two_tasks(setup):
    """100 equal scalars among random ones: in every window one bucket holds more than 64 entries.  (So few entries are cut into tasks
    of 4 -- msm_task_shift -- so that bucket is 25 tasks, each record with the reference its task starts at.)"""
    rng = np.random.default_rng(0x3403)
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(N)]
    v = sum(0x2345 << o for o in OFFS)
    for i in range(100):
        vals[(i * 41 + 5) % N] = v
    _check(setup, vals)


def test_all_ones_column(setup):
    """every scalar is 1: bucket 0 holds the N entries of window 0 (1025 tasks of 4: a heavy bucket, records written by whole
    wavefronts), every other bucket is empty"""
    _check(setup, [1] * N)

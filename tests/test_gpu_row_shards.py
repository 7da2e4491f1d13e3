"""GPU (-m gpu): row-shard sets (zkhip_row_shards_*, include/zkhip.h).  Every window must hold its definition element for element,
scatter / gather / upload must agree, the transform-to-shards call must write the bytes of zkhip_coeff_to_extended_device + scatter, and the
closed-form Lagrange kernel must write the bytes of ifft_scaled + coeff_to_extended of the indicator columns (how keygen_device builds l0,
l_last and l_active_row).  S devices are S contexts of card 0 (ZKHIP_TEST_DUPLICATE_DEVICES, as in tests/test_gpu_quotient_sharded.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F

pytestmark = pytest.mark.gpu


class _Contexts:
    """zkhip_init over `ndev` contexts of card 0; restores the default single-device state on exit"""

    def __init__(self, lib, ndev):
        self.lib, self.ndev = lib, ndev

    def __enter__(self):
        self.lib.zkhip_shutdown()
        if self.ndev > 1:
            os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
        _lib.check(self.lib.zkhip_init((C.c_int * self.ndev)(*([0] * self.ndev)), self.ndev))
        assert self.lib.zkhip_device_count() == self.ndev
        return self

    def __exit__(self, *exc):
        self.lib.zkhip_shutdown()
        os.environ.pop("ZKHIP_TEST_DUPLICATE_DEVICES", None)
        _lib.check(self.lib.zkhip_init(None, 0))
        return False


def _rand(rows, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 1 << 62, (rows, 4), dtype=torch.int64, generator=g)
    t[:, 3] &= (1 << 61) - 1
    return t.cuda()


def _shard_range(n, j, S):
    base, extra = divmod(n, S)
    lo = j * base + min(j, extra)
    return lo, lo + base + (1 if j < extra else 0)


def _download(ptr, elements):
    out = np.empty((elements, 4), dtype=np.uint64)
    _lib.check(_lib.load().zkhip_download(out.ctypes.data, C.c_void_p(ptr), out.nbytes))
    return out


def _check_windows(rs, S, cols):
    """every shard's window of every column against column[(row0 - halo_lo + t) mod N]"""
    N = 1 << rs.ext_k
    torch.cuda.synchronize()
    for j in range(S):
        for c, col in enumerate(cols):
            ptr, dev, row0, count = rs.window(j, c)
            assert dev == 0 and (row0, row0 + count) == _shard_range(N, j, S)
            W = rs.halo_lo + count + rs.halo_hi
            idx = (np.arange(W) + row0 - rs.halo_lo) % N
            assert np.array_equal(_download(ptr, W), col[idx]), (j, c)


@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("ext_k,halo_lo,halo_hi", [(10, 24, 8), (3, 13, 11), (6, 0, 0)])
def test_windows_scatter_gather_upload(lib, S, ext_k, halo_lo, halo_hi):
    """ext_k = 3 with halos 13 / 11: every window is longer than the domain (wraps more than once)"""
    N = 1 << ext_k
    cols = [_rand(N, 100 * ext_k + c) for c in range(3)]
    host = [c.cpu().numpy().view(np.uint64) for c in cols]
    with _Contexts(lib, S):
        with E.RowShards(ext_k, 3, halo_lo, halo_hi) as rs:
            for c in range(3):
                rs.scatter_device(c, cols[c].data_ptr())
            _check_windows(rs, S, host)
            back = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
            for c in range(3):
                rs.gather_device(c, back.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(back.cpu().numpy().view(np.uint64), host[c])
        with E.RowShards(ext_k, 3, halo_lo, halo_hi) as up:
            for c in range(3):
                up.upload(c, host[c])
            _check_windows(up, S, host)
            assert np.array_equal(up.download(1), host[1])


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("k,ek,n_polys", [(4, 6, 5), (8, 10, 2), (12, 14, 4)])
def test_transform_to_shards_is_transform_then_scatter(lib, S, k, ek, n_polys):
    """n_polys < S leaves devices without a column to transform: they still receive their windows"""
    dom = Z.EvaluationDomain(4, k)
    assert dom.extended_k == ek
    n, N = 1 << k, 1 << ek
    coeff = _rand(n_polys * n, 7 * k + S)
    with _Contexts(lib, 1):
        ext = torch.empty((n_polys, N, 4), dtype=torch.int64, device="cuda")
        _lib.check(lib.zkhip_coeff_to_extended_device(coeff.data_ptr(), n, k, ext.data_ptr(), N, ek, n_polys, dom.extended_omega.ctypes.data,
                                                      dom.g_coset.ctypes.data, None))
        torch.cuda.synchronize()
        exp = ext.cpu().numpy().view(np.uint64)
    with _Contexts(lib, S):
        with E.RowShards(ek, n_polys + 2, 17, 9) as rs:
            _lib.check(lib.zkhip_coeff_to_extended_row_shards_device(coeff.data_ptr(), k, n_polys, n, dom.extended_omega.ctypes.data,
                                                                     dom.g_coset.ctypes.data, rs.handle, 1, None))
            for c in range(n_polys):
                assert np.array_equal(rs.download(1 + c), exp[c]), c
            torch.cuda.synchronize()
            for j in range(S):
                for c in range(n_polys):
                    ptr, _, row0, count = rs.window(j, 1 + c)
                    W = 17 + count + 9
                    assert np.array_equal(_download(ptr, W), exp[c][(np.arange(W) + row0 - 17) % N]), (j, c)


def _indicator_cosets(lib, k, u, dom):
    """l0, l_last, l_active_row as keygen_device builds them: indicator columns, ifft_scaled, coeff_to_extended"""
    n, N = 1 << k, dom.extended_len()
    one = F.fr_encode([1])[0]
    ind = np.zeros((3, n, 4), dtype=np.uint64)
    ind[0, 0] = one
    ind[1, u] = one
    ind[2, :u] = one
    d = torch.from_numpy(ind.view(np.int64)).cuda()
    out = torch.empty((3, N, 4), dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_ifft_scaled_batch_device(d.data_ptr(), dom.omega_inv.ctypes.data, k, dom.ifft_divisor.ctypes.data, 3, n, None))
    _lib.check(lib.zkhip_coeff_to_extended_device(d.data_ptr(), n, k, out.data_ptr(), N, dom.extended_k, 3, dom.extended_omega.ctypes.data,
                                                  dom.g_coset.ctypes.data, None))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def _lagrange_cases():
    for k in range(3, 15):
        n = 1 << k
        for degree in (4, 8):
            us = {n - (b + 1) for b in (1, 3, 5) if n - (b + 1) >= 1} | {1, n - 1}
            for u in sorted(us):
                yield k, degree, u


@pytest.mark.parametrize("k,degree,u", list(_lagrange_cases()))
def test_lagrange_kernel_is_the_transformed_indicators(lib, k, degree, u):
    dom = Z.EvaluationDomain(degree, k)
    exp = _indicator_cosets(lib, k, u, dom)
    with E.RowShards(dom.extended_k, 4, 5, 3) as rs:
        _lib.check(lib.zkhip_lagrange_cosets_row_shards_device(k, u, dom.omega.ctypes.data, dom.extended_omega.ctypes.data, dom.g_coset.ctypes.data,
                                                               rs.handle, 1, None))
        for c in range(3):
            assert np.array_equal(rs.download(1 + c), exp[c]), ("l0", "l_last", "l_active_row")[c]


@pytest.mark.parametrize("S", [2, 3, 8])
def test_lagrange_kernel_windows_on_several_devices(lib, S):
    """each device writes its own windows, halos wrapping; k = 3 / ext_k = 5 over 8 devices makes every window wider than its rows"""
    for k, degree in ((3, 4), (9, 8)):
        dom = Z.EvaluationDomain(degree, k)
        u = (1 << k) - 6 if k > 3 else 2
        with _Contexts(lib, 1):
            exp = _indicator_cosets(lib, k, u, dom)
        with _Contexts(lib, S):
            with E.RowShards(dom.extended_k, 3, 40, 7) as rs:
                _lib.check(lib.zkhip_lagrange_cosets_row_shards_device(k, u, dom.omega.ctypes.data, dom.extended_omega.ctypes.data,
                                                                       dom.g_coset.ctypes.data, rs.handle, 0, None))
                _check_windows(rs, S, list(exp))


def test_bad_handles_and_ranges_are_rejected_and_a_correct_call_follows(lib):
    N = 1 << 6
    col = _rand(N, 5)
    host = col.cpu().numpy().view(np.uint64)
    out = C.c_void_p()
    with _Contexts(lib, 3):
        three = E.RowShards(6, 2, 4, 4)
        h3 = three.handle.value
    # after shutdown (the context manager shut the 3-context library down): the handle is stale
    with _Contexts(lib, 2):
        for rc in (lib.zkhip_row_shards_scatter_device(C.c_void_p(h3), 0, col.data_ptr(), None),
                   lib.zkhip_row_shards_window(C.c_void_p(h3), 0, 0, C.byref(out), None, None, None),
                   lib.zkhip_row_shards_destroy(C.c_void_p(h3))):
            assert rc == -1 and lib.zkhip_last_error()
        with E.RowShards(6, 2, 4, 4) as rs:
            rs.scatter_device(1, col.data_ptr())
            assert lib.zkhip_row_shards_window(rs.handle, 2, 0, C.byref(out), None, None, None) == -1          # shard out of range
            assert lib.zkhip_row_shards_window(rs.handle, 0, 2, C.byref(out), None, None, None) == -1          # col out of range
            assert lib.zkhip_row_shards_scatter_device(rs.handle, 2, col.data_ptr(), None) == -1
            assert lib.zkhip_row_shards_gather_device(rs.handle, 5, col.data_ptr(), None) == -1
            assert lib.zkhip_row_shards_upload(rs.handle, 0, None) == -1
            assert lib.zkhip_row_shards_scatter_device(C.c_void_p(rs.handle.value + 8), 0, col.data_ptr(), None) == -1   # never issued
            assert lib.zkhip_row_shards_create(6, 1, 0, 0, None) == -1
            assert np.array_equal(rs.download(1), host)                                                        # a correct call follows
        stale = E.RowShards(6, 1, 0, 0)
        h = stale.handle.value
        stale.destroy()
        assert lib.zkhip_row_shards_scatter_device(C.c_void_p(h), 0, col.data_ptr(), None) == -1               # after destroy
    # a set made under 3 devices, used under 2
    with _Contexts(lib, 3):
        rs3 = E.RowShards(6, 1, 2, 2)
        lib.zkhip_shutdown()
        os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
        _lib.check(lib.zkhip_init((C.c_int * 2)(0, 0), 2))
        assert lib.zkhip_row_shards_scatter_device(rs3.handle, 0, col.data_ptr(), None) == -1
        with E.RowShards(6, 1, 2, 2) as rs2:
            rs2.upload(0, host)
            assert np.array_equal(rs2.download(0), host)

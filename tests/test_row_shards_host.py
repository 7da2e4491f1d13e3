"""CPU: the pieces of the row-shard key that need no device -- the halo helper a key's set is made with (pinned to the quotient program's
own halos), the copy-plan arithmetic of tools/quotient_shard_time.py for both key forms, and ZKHIP_ENODEV from the new entry points on a host
without a GPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from zksnap_circuits_halo2_amd import evaluation as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _systems():
    yield E.halo2_lib_shape(2, 1)
    yield E.halo2_lib_shape(4, 0)
    yield E.halo2_lib_shape(1, 2, blinding=9)
    gates = [[E.Fixed(0) * (E.Advice(0, -3) + E.Advice(1, 2) - E.Advice(0))], [E.Advice(1, -1) * E.Fixed(1, 1)]]
    # one permutation set: no -(blinding + 1) rotation; four columns at degree 4: two sets
    yield E.ConstraintSystem(num_fixed=2, num_advice=2, gates=gates, permutation_columns=[("advice", 0), ("fixed", 1)], blinding_factors=3, degree=4)
    yield E.ConstraintSystem(num_fixed=2, num_advice=2, gates=gates, permutation_columns=[("advice", 0), ("advice", 1), ("fixed", 0), ("fixed", 1)],
                             blinding_factors=7, degree=4)
    yield E.ConstraintSystem(num_fixed=1, num_advice=1, gates=[[E.Fixed(0) * E.Advice(0)]], degree=3)
    yield E.ConstraintSystem(num_fixed=1, num_advice=2, lookups=[E.Lookup([E.Advice(1, 1)], [E.Fixed(0)])], degree=5)


@pytest.mark.parametrize("k", [3, 6, 10])
def test_quotient_halos_are_the_programs(k):
    for cs in _systems():
        ek = k
        while (1 << ek) < (1 << k) * (cs.degree - 1):
            ek += 1
        prog = E.evaluate_h_program(cs, k, ek, 3, 5, 7, 11)
        assert E.quotient_halos(cs, k, ek) == prog.halos(ek), cs


def _tool():
    spec = importlib.util.spec_from_file_location("quotient_shard_time", os.path.join(ROOT, "tools", "quotient_shard_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_copy_plan_of_both_key_forms():
    T = _tool()
    n_cols, n_coeff, k, ek, halo = 29, 13, 24, 26, 200
    N = 1 << ek
    for key in (False, True):
        assert T.exchange_bytes(n_cols, n_coeff, k, ek, halo, 1, 0, key_shards=key) == (0, 0)
        assert T.primary_sent_bytes(n_cols, n_coeff, k, ek, halo, 1, 0, key_shards=key) == 0
    for S in (3, 8):
        for j in range(S):
            lo, hi = T.shard_range(N, j, S)
            W = halo + hi - lo
            olo, ohi = T.shard_range(n_coeff, j, S)
            own = ohi - olo
            ext_recv, ext_out = T.exchange_bytes(n_cols, n_coeff, k, ek, halo, S, j)
            rs_recv, rs_out = T.exchange_bytes(n_cols, n_coeff, k, ek, halo, S, j, key_shards=True)
            assert ext_out == rs_out == ((hi - lo) * 32 if j else 0)
            # the 16 key windows no longer reach a secondary; the COEFF traffic is the same
            assert ext_recv - rs_recv == ((n_cols - n_coeff) * W * 32 if j else 0)
            assert rs_recv == (own * (1 << k) * 32 if j else 0) + (n_coeff - own) * W * 32
            p_ext = T.primary_sent_bytes(n_cols, n_coeff, k, ek, halo, S, j)
            p_rs = T.primary_sent_bytes(n_cols, n_coeff, k, ek, halo, S, j, key_shards=True)
            o0 = T.shard_range(n_coeff, 0, S)[1]
            assert p_rs == (0 if j == 0 else own * (1 << k) * 32 + o0 * W * 32)
            assert p_ext - p_rs == (0 if j == 0 else (n_cols - n_coeff) * W * 32)


def _no_gpu(lib):
    return lib.zkhip_device_count() <= 0


def test_row_shard_entries_report_no_device(lib):
    if not _no_gpu(lib):
        pytest.skip("a GPU is present: the GPU tests cover these entry points")
    h = C.c_void_p()
    assert lib.zkhip_row_shards_create(10, 3, 4, 4, C.byref(h)) == -2                 # ZKHIP_ENODEV
    assert lib.zkhip_last_error() and not h.value
    z = np.zeros(4, dtype=np.uint64)
    assert lib.zkhip_lagrange_cosets_row_shards_device(4, 10, z.ctypes.data, z.ctypes.data, z.ctypes.data, C.c_void_p(0x10), 0, None) == -2
    assert lib.zkhip_coeff_to_extended_row_shards_device(z.ctypes.data, 2, 1, 4, z.ctypes.data, z.ctypes.data, C.c_void_p(0x10), 0, None) == -2
    for rc in (lib.zkhip_row_shards_scatter_device(C.c_void_p(0x10), 0, z.ctypes.data, None),
               lib.zkhip_row_shards_gather_device(C.c_void_p(0x10), 0, z.ctypes.data, None),
               lib.zkhip_row_shards_upload(C.c_void_p(0x10), 0, z.ctypes.data),
               lib.zkhip_row_shards_window(C.c_void_p(0x10), 0, 0, None, None, None, None)):
        assert rc == -2

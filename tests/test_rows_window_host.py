"""CPU: the halos of a row window (RowProgram.halos, the formula of include/zkhip.h) and the two entry points of the sharded quotient
on a host without a GPU (ZKHIP_ENODEV with a message, nothing else happens)."""
import ctypes as C

import numpy as np
import pytest

from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F


def _prog(rots, scale):
    p = E.RowProgram(rot_scale=scale)
    acc = None
    for i, r in enumerate(rots):
        p.emit(E.OP_MOV if acc is None else E.OP_ADD, 0, p.column(i, r), None if acc is None else E.RowProgram.reg(0))
        acc = 0
    p.result_reg = 0
    return p


@pytest.mark.parametrize("rots,scale,exp", [
    ([0], 1, (0, 0)),
    ([-6, -1, 0, 1, 2, 3], 4, (24, 12)),
    ([-3, -1], 2, (6, 0)),                 # negative rotations only
    ([1, 5], 8, (0, 40)),                  # positive rotations only
    ([2, -7], 1, (7, 2)),
    ([], 4, (0, 0)),                       # no column operands
    ([-1, 1], -2, (2, 2)),                 # a negative scale flips the sides
])
def test_halos(rots, scale, exp):
    p = _prog(rots, scale) if rots else E.RowProgram(rot_scale=scale)
    assert p.halos(10) == exp
    assert p.halos(2) == exp              # not reduced modulo the domain: a window may be wider than the domain


def _no_gpu(lib):
    return lib.zkhip_device_count() <= 0


def test_window_and_sharded_entries_report_no_device(lib):
    if not _no_gpu(lib):
        pytest.skip("a GPU is present: the GPU tests cover these entry points")
    p = _prog([-1, 2], 1)
    prog, keep = p._marshal()
    win = np.zeros((16, 4), dtype=np.uint64)
    ptrs = (C.c_void_p * 2)(win.ctypes.data, win.ctypes.data)
    out = np.zeros((8, 4), dtype=np.uint64)
    rc = lib.zkhip_fr_eval_rows_window_device(C.byref(prog), ptrs, 2, 4, 0, 8, 0, out.ctypes.data, None)
    assert rc == -2, rc                                              # ZKHIP_ENODEV
    assert lib.zkhip_last_error()
    forms = (C.c_uint32 * 2)(0, 1)
    om = F.fr_encode([F.omega_for(4)])[0]
    rc = lib.zkhip_fr_eval_rows_sharded_device(C.byref(prog), ptrs, forms, 2, 2, 4, om.ctypes.data, om.ctypes.data, out.ctypes.data, None)
    assert rc == -2, rc
    assert lib.zkhip_last_error()
    del keep

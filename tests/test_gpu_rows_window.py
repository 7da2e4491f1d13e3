"""GPU (-m gpu): row programs over a row window (zkhip_fr_eval_rows_window_device): `count` rows from global row
`row0` of a 2^log_rows domain, every column passed as a window buffer of halo_lo + count + halo_hi elements cut from the whole column by
the cyclic definition (include/zkhip.h).  Every window's output must be the matching rows of the whole-domain launch
(zkhip_fr_eval_rows_device), for both executors: the interpreter here, the compiled kernels in a child process with ZKHIP_VM_JIT=2."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = F.R_MOD


def _random_cols(n_cols, rows, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_cols):
        t = torch.randint(0, 1 << 62, (rows, 4), dtype=torch.int64, generator=g)
        t[:, 3] &= (1 << 61) - 1                      # canonical: below the modulus' top limb
        out.append(t.numpy())
    return out


def _quotient_program(ek, seed=3):
    cs = E.halo2_lib_shape(2, 1)
    rng = random.Random(seed)
    beta, gamma, theta, y = (rng.randrange(R) for _ in range(4))
    return E.evaluate_h_program(cs, ek - 2, ek, beta, gamma, theta, y), E.quotient_columns(cs).total


def _whole(prog, cols, ek, prev=None):
    d_cols = [torch.from_numpy(c).cuda() for c in cols]
    out = torch.from_numpy(prev.copy()).cuda() if prev is not None else torch.zeros((1 << ek, 4), dtype=torch.int64, device="cuda")
    prog.run_device([t.data_ptr() for t in d_cols], ek, out.data_ptr(), accumulate=prev is not None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _windows(prog, cols, ek, row0, count):
    lo, hi = prog.halos(ek)
    idx = (row0 - lo + np.arange(lo + count + hi)) % (1 << ek)
    return [torch.from_numpy(np.ascontiguousarray(c[idx])).cuda() for c in cols]


def _window(prog, cols, ek, row0, count, prev=None):
    wins = _windows(prog, cols, ek, row0, count)
    out = torch.from_numpy(prev.copy()).cuda() if prev is not None else torch.zeros((count, 4), dtype=torch.int64, device="cuda")
    prog.run_window_device([t.data_ptr() for t in wins], ek, row0, count, out.data_ptr(), accumulate=prev is not None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("ek", [8, 12])
def test_windows_match_the_whole_domain_launch(lib, ek):
    prog, ncol = _quotient_program(ek)
    assert prog.omega is not None and min(prog.rotations) < 0 and max(prog.rotations) > 0
    assert prog.halos(ek) == (6 * 4, 3 * 4)
    rows = 1 << ek
    cols = _random_cols(ncol, rows, 11 + ek)
    whole = _whole(prog, cols, ek)
    for row0, count in [(0, rows // 4), (rows // 2 - 3, 37), (rows - 5, 20), (rows // 3, 1), (rows - 1, 1), (0, rows), (7, rows)]:
        got = _window(prog, cols, ek, row0, count)
        exp = whole[(row0 + np.arange(count)) % rows]
        assert np.array_equal(got, exp), (row0, count)


def test_windows_wider_than_the_domain(lib):
    ek = 5
    prog, ncol = _quotient_program(ek)
    lo, hi = prog.halos(ek)
    assert lo + 8 + hi > (1 << ek)
    cols = _random_cols(ncol, 1 << ek, 5)
    whole = _whole(prog, cols, ek)
    for row0 in range(0, 32, 8):
        assert np.array_equal(_window(prog, cols, ek, row0, 8), whole[row0:row0 + 8]), row0
    assert np.array_equal(_window(prog, cols, ek, 29, 8), whole[(29 + np.arange(8)) % 32])


def _prev_program():
    p = E.RowProgram(rot_scale=2, omega=F.omega_for(9))
    p.emit(E.OP_MUL, 0, p.column(0, 1), p.column(1, -2))
    p.emit(E.OP_MAD, 1, E.RowProgram.reg(0), E.RowProgram.ROWPOW, E.RowProgram.PREV)
    p.emit(E.OP_ADD, 0, E.RowProgram.reg(1), p.column(0, -3))
    p.result_reg = 0
    return p


def test_accumulate_reads_the_window_output(lib):
    ek = 9
    p = _prev_program()
    assert p.halos(ek) == (6, 2)
    cols = _random_cols(2, 1 << ek, 21)
    prev = _random_cols(1, 1 << ek, 22)[0]
    whole = _whole(p, cols, ek, prev=prev)
    for row0, count in [(0, 100), (450, 100), (511, 1)]:
        idx = (row0 + np.arange(count)) % (1 << ek)
        got = _window(p, cols, ek, row0, count, prev=np.ascontiguousarray(prev[idx]))
        assert np.array_equal(got, whole[idx]), (row0, count)


def test_bad_arguments_are_rejected_and_the_library_stays_usable(lib):
    ek = 6
    p = _prev_program()
    cols = _random_cols(2, 1 << ek, 31)
    wins = _windows(p, cols, ek, 0, 16)
    out = torch.zeros((1 << ek, 4), dtype=torch.int64, device="cuda")
    prog, keep = p._marshal()
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in wins])
    s = torch.cuda.current_stream().cuda_stream

    def call(row0, count, ptrs=ptrs, prog=prog):
        return lib.zkhip_fr_eval_rows_window_device(C.byref(prog), ptrs, 2, ek, row0, count, 0, out.data_ptr(), s)

    assert call(1 << ek, 1) == -1  # ZKHIP_EINVAL: row0 outside the domain
    assert call(0, 0) == -1  # empty window
    assert call(0, (1 << ek) + 1) == -1  # more rows than the domain
    assert call(0, 16, ptrs=(C.c_void_p * 2)(wins[0].data_ptr(), None)) == -1
    assert b"null" in lib.zkhip_last_error()
    bad, keep2 = p._marshal()
    bad.result_reg = 99
    assert call(0, 16, prog=bad) == -1
    assert lib.zkhip_fr_eval_rows_window_device(C.byref(prog), ptrs, 2, ek, 0, 16, 0, None, s) == -1
    assert call(0, 16) == 0
    torch.cuda.synchronize()
    whole = _whole(p, cols, ek)
    assert np.array_equal(out[:16].cpu().numpy(), whole[:16])
    del keep, keep2


_CHILD = r'''
import sys, hashlib, ctypes as C
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np, torch
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F
import zksnap_circuits_halo2_amd as Z
import test_gpu_rows_window as T
lib = _lib.load()
h = hashlib.sha256()
for ek in (8, 12):
    prog, ncol = T._quotient_program(ek)
    cols = T._random_cols(ncol, 1 << ek, 11 + ek)
    whole = T._whole(prog, cols, ek)
    h.update(whole.tobytes())
    for row0, count in [(0, 64), ((1 << ek) - 5, 20), (3, 1 << ek)]:
        got = T._window(prog, cols, ek, row0, count)
        assert np.array_equal(got, whole[(row0 + np.arange(count)) %% (1 << ek)]), (ek, row0, count)
        h.update(got.tobytes())
# a profiled sharded call over three contexts: the phase names say which executor ran the primary's window
k, ek = 6, 8
prog, ncol = T._quotient_program(ek)
dom = Z.EvaluationDomain(4, k)
coeffs = [torch.from_numpy(c).cuda() for c in T._random_cols(ncol, 1 << k, 77)]
lib.zkhip_shutdown()
_lib.check(lib.zkhip_init((C.c_int * 3)(0, 0, 0), 3))
out = torch.zeros((1 << ek, 4), dtype=torch.int64, device="cuda")
_lib.check(lib.zkhip_profile_enable(1))
E.evaluate_rows_sharded_device(prog, [(c.data_ptr(), E.COL_COEFF) for c in coeffs], k, ek, dom, out.data_ptr())
torch.cuda.synchronize()
ms = (C.c_double * 32)()
names = ((C.c_char * 64) * 32)()
n = lib.zkhip_profile_read(ms, names, 32)
_lib.check(lib.zkhip_profile_enable(0))
print("PHASES", ",".join(names[i].value.decode() for i in range(n)))
h.update(out.cpu().numpy().tobytes())
print("DIGEST", h.hexdigest())
''' % (ROOT, os.path.join(ROOT, "tests"))


def test_compiled_windows_agree_with_the_interpreter():
    res = {}
    for mode in ("0", "2"):
        r = subprocess.run([sys.executable, "-c", _CHILD], capture_output=True, text=True, timeout=900, cwd=ROOT,
                           env=dict(os.environ, ZKHIP_VM_JIT=mode, ZKHIP_VM_JIT_LOG="1", ZKHIP_TEST_DUPLICATE_DEVICES="1"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "compilation failed" not in r.stderr, r.stderr[-3000:]
        lines = dict(l.split(" ", 1) for l in r.stdout.splitlines() if l.startswith(("DIGEST", "PHASES")))
        res[mode] = lines
    assert res["0"]["DIGEST"] == res["2"]["DIGEST"]
    assert res["0"]["PHASES"].split(",") == ["transform", "exchange", "rows_interpreted", "gather"]
    assert res["2"]["PHASES"].split(",") == ["transform", "exchange", "rows_compiled", "gather"]

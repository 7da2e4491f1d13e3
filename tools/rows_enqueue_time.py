#!/usr/bin/env python3
"""The host side of a row-program launch (rowvm.hip row_vm_launch: plan, staging, fill, one copy, one grid) where nothing else is left to
time: `--calls` back-to-back zkhip_fr_eval_rows_device calls of a 4-instruction program over 2^10 rows on one stream, then one synchronize.
The kernel is a few microseconds, so the wall time of a repetition is the enqueue path.  Prints every repetition and the median.
    python tools/rows_enqueue_time.py [--calls 4000] [--reps 15]          (ZKHIP_LIB_PATH names another build for an A/B on one box)"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F
from zksnap_circuits_halo2_amd.tensors import fr_empty, fr_random

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=4000)
ap.add_argument("--reps", type=int, default=15)
args = ap.parse_args()
lib = _lib.load()
k = 10
p = E.RowProgram(omega=F.omega_for(k))                   # a[row + 1] * b[row] + omega^row - 5, then doubled
p.emit(E.OP_MUL, 0, p.column(0, 1), p.column(1))
p.emit(E.OP_ADD, 1, E.RowProgram.reg(0), E.RowProgram.ROWPOW)
p.emit(E.OP_SUB, 0, E.RowProgram.reg(1), p.constant(5))
p.emit(E.OP_DBL, 0, E.RowProgram.reg(0))
cols = [fr_random(1 << k) for _ in range(2)]
out = fr_empty(1 << k)
ptrs = (C.c_void_p * 2)(*[c.data_ptr() for c in cols])
prog, keep = p._marshal()
stream = torch.cuda.current_stream().cuda_stream


def rep():
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.calls):
        rc = lib.zkhip_fr_eval_rows_device(C.byref(prog), ptrs, 2, k, 0, out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    return (time.perf_counter() - t) * 1e3


for _ in range(3):
    rep()
ms = [rep() for _ in range(args.reps)]
print(f"{args.calls} x zkhip_fr_eval_rows_device(4 instructions, 2^{k} rows) + synchronize, wall ms: " + " ".join(f"{v:.2f}" for v in ms))
print(f"median {statistics.median(ms):.3f} ms = {statistics.median(ms) / args.calls * 1e3:.2f} us per call (min {min(ms):.3f}, max {max(ms):.3f})")

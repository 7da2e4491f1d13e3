"""GPU (-m gpu): the one launch path of the row programs (rowvm.hip: row_vm_launch) through every form it serves, compared exactly with
`oracle.bn254.row_program_run`.

Calls back to back: every form of launch -- one program, a long one, a sum, the witness check, a window -- enqueued on one non-default stream
without a host wait in between, one synchronize, then every result.  Each launch fills one of the two pinned staging buffers of the
stream's scratch set while the copy out of the other may still be in flight, and the long program regrows its buffer on the way: what is
pinned is that a buffer is never rewritten before the copy that reads it has completed, whatever form the calls around it have.

Layout edges: the smallest blob there is -- `MOV r0 <- ROWPOW`, no constants, no rotations, no columns -- on both sides of the 2^12 split of
the power tables, alone and as one of two summed parts whose other part names no omega."""
import random

import numpy as np
import pytest
import torch

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import evaluation as E, fields as F, mock as M
from zksnap_circuits_halo2_amd.tensors import fr_empty, fr_ints, fr_words

pytestmark = pytest.mark.gpu
R = F.R_MOD
NONE = (1 << 64) - 1
reg = E.RowProgram.reg


def oracle(p, cols, k, only_rows=None):
    return O.row_program_run(p.insns, p.constants, p.rotations, p.rot_scale, p.result_reg, cols, k, omega=p.omega, only_rows=only_rows)


def short_program(k):
    p = E.RowProgram(omega=F.omega_for(k))                     # a[row + 1] * b[row] + omega^row - 5
    p.emit(E.OP_MUL, 0, p.column(0, 1), p.column(1))
    p.emit(E.OP_ADD, 1, reg(0), E.RowProgram.ROWPOW)
    p.emit(E.OP_SUB, 0, reg(1), p.constant(5))
    return p


def long_program(k, n_insns=700, n_constants=40, seed=7):
    """a chain over 8 registers that reads every constant, three columns at rotations -2 .. 2 and omega^row"""
    rng = random.Random(seed)
    p = E.RowProgram(omega=F.omega_for(k))
    consts = [rng.randrange(R) for _ in range(n_constants)]
    p.emit(E.OP_MOV, 0, p.column(0, -2))
    for i in range(1, n_insns):
        dst, src = i % 8, (i - 1) % 8
        if i % 7 == 3:
            p.emit(E.OP_MUL, dst, p.column(i % 3, i % 5 - 2), reg(src))        # the memory operand first: the fill puts it second
        elif i % 7 == 5:
            p.emit(E.OP_SUB, dst, reg(src), E.RowProgram.ROWPOW)
        elif i % 2:
            p.emit(E.OP_MAD, dst, reg(src), p.constant(consts[i % n_constants]), p.column(i % 3, i % 5 - 2))
        else:
            p.emit(E.OP_ADD, dst, reg(src), p.constant(consts[i % n_constants]))
    p.result_reg = (n_insns - 1) % 8
    assert len(p.insns) == n_insns and len(p.constants) == n_constants
    return p


def sum_programs(k):
    out = []
    p = E.RowProgram(); p.emit(E.OP_MUL, 0, p.column(0), p.column(1)); out.append(p)
    p = E.RowProgram(omega=F.omega_for(k)); p.emit(E.OP_MUL, 7, p.column(2), E.RowProgram.ROWPOW); p.result_reg = 7; out.append(p)
    p = E.RowProgram(); p.emit(E.OP_SUB, 0, p.column(3, -1), p.column(4, 3)); out.append(p)
    p = E.RowProgram(); p.emit(E.OP_SQR, 11, p.column(1, 2)); p.emit(E.OP_ADD, 11, reg(11), p.constant(9)); p.result_reg = 11; out.append(p)
    p = E.RowProgram(); p.emit(E.OP_MOV, 0, p.constant(12345)); out.append(p)
    return out


def window_program(k):
    p = E.RowProgram(omega=F.omega_for(k))                     # a[row - 2] * b[row + 1] + omega^row
    p.emit(E.OP_MUL, 0, p.column(0, -2), p.column(1, 1))
    p.emit(E.OP_ADD, 0, reg(0), E.RowProgram.ROWPOW)
    return p


def test_back_to_back_calls_of_every_form_share_the_staging_ring():
    k, n = 8, 256
    rng = random.Random(0x57A6)
    omega = F.omega_for(k)
    cols = [[rng.randrange(R) for _ in range(n)] for _ in range(5)]
    short, long_, parts, win = short_program(k), long_program(k), sum_programs(k), window_program(k)
    weights = [rng.randrange(R) for _ in parts]
    # the gates of the check: a[row + 1] * b[row] - c[row], d[row] - omega^row, e[row]; they hold except on planted rows
    g0 = E.RowProgram(); g0.emit(E.OP_MUL, 0, g0.column(0, 1), g0.column(1)); g0.emit(E.OP_SUB, 0, reg(0), g0.column(5))
    g1 = E.RowProgram(omega=omega); g1.emit(E.OP_SUB, 6, g1.column(6), E.RowProgram.ROWPOW); g1.result_reg = 6
    g2 = E.RowProgram(); g2.emit(E.OP_MOV, 12, g2.column(7)); g2.result_reg = 12
    gates = [g0, g1, g2]
    check_cols = cols + [[cols[0][(r + 1) % n] * cols[1][r] % R for r in range(n)], [pow(omega, r, R) for r in range(n)], [0] * n]
    for c, planted in ((5, (4, 5, 100, 244, 245)), (6, (77,)), (7, (0, 255))):         # rows next to and inside [5, 245)
        for r in planted:
            check_cols[c][r] = (check_cols[c][r] + 1 + r) % R
    row0, count = 5, 240
    w_row0, w_count = 250, 20                                  # rows 250 .. 255, 0 .. 13: the window wraps the domain's end
    lo, hi = win.halos(k)
    assert (lo, hi) == (2, 1)
    windows = [[c[(w_row0 - lo + t) % n] for t in range(lo + w_count + hi)] for c in cols[:2]]

    # the reference, once
    want_short, want_long = oracle(short, cols, k), oracle(long_, cols, k)
    want_sum = [sum(w * v for w, v in zip(weights, vals)) % R for vals in zip(*[oracle(p, cols, k) for p in parts])]
    want_check = []
    for g in gates:
        failing = [row0 + i for i, v in enumerate(oracle(g, check_cols, k, only_rows=range(row0, row0 + count))) if v]
        want_check.append((len(failing), failing[0] if failing else NONE))
    assert [c for c, _ in want_check] == [3, 1, 0]              # the planted rows inside the range, and none of those next to it
    want_window = oracle(win, cols, k, only_rows=[(w_row0 + i) % n for i in range(w_count)])

    d_cols = [fr_words(c) for c in check_cols]
    d_windows = [fr_words(c) for c in windows]
    outs = {name: fr_empty(n).zero_() for name in ("short", "long", "sum", "short again", "long again")}
    outs["window"] = fr_empty(w_count).zero_()
    reports = torch.full((len(gates), 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=d_cols[0].device)
    ptrs = [c.data_ptr() for c in d_cols]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    assert s != 0
    short.run_device(ptrs[:5], k, outs["short"].data_ptr(), stream=s)
    long_.run_device(ptrs[:5], k, outs["long"].data_ptr(), stream=s)
    E.run_programs_sum_device(parts, weights, ptrs[:5], k, outs["sum"].data_ptr(), stream=s)
    M.enqueue_check_rows(gates, d_cols, k, row0, count, reports.data_ptr(), stream=s)
    win.run_window_device([w.data_ptr() for w in d_windows], k, w_row0, w_count, outs["window"].data_ptr(), stream=s)
    short.run_device(ptrs[:5], k, outs["short again"].data_ptr(), stream=s)
    long_.run_device(ptrs[:5], k, outs["long again"].data_ptr(), stream=s)
    stream.synchronize()

    got_reports = reports.cpu().numpy().view(np.uint64)
    assert [(int(a), int(b)) for a, b in got_reports] == want_check
    for name, want in (("short", want_short), ("long", want_long), ("sum", want_sum), ("window", want_window), ("short again", want_short),
                       ("long again", want_long)):
        assert fr_ints(outs[name]) == want, name


@pytest.mark.parametrize("k", [0, 11, 12, 13])
def test_the_smallest_blob_on_both_sides_of_the_power_table_split(k):
    n = 1 << k
    omega = F.omega_for(k)
    p = E.RowProgram(omega=omega)
    p.emit(E.OP_MOV, 0, E.RowProgram.ROWPOW)
    assert (len(p.insns), p.constants, p.rotations, p.n_columns) == (1, [], [], 0)
    want = oracle(p, [], k)
    assert want[-1] == pow(omega, n - 1, R)
    out = fr_empty(n).zero_()
    p.run_device([], k, out.data_ptr())
    torch.cuda.synchronize()
    assert fr_ints(out) == want
    # ... and as one of two summed parts; the other names no omega
    q = E.RowProgram()
    q.emit(E.OP_MOV, 3, q.constant(7))
    q.result_reg = 3
    w = [0x1234567 + k, R - 2]
    for parts, weights in (([p, q], w), ([q, p], w[::-1])):
        out = fr_empty(n).zero_()
        E.run_programs_sum_device(parts, weights, [], k, out.data_ptr())
        torch.cuda.synchronize()
        assert fr_ints(out) == [(w[0] * v + w[1] * 7) % R for v in want], [len(x.constants) for x in parts]

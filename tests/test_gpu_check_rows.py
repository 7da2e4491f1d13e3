"""GPU: `zkhip_check_rows_device` -- per program, how many rows of [row0, row0 + count) give a non-zero result and which is the first.

Expected values are hand-planted positions (a column that is zero except where the test put something) or Python integers; the one
comparison against the device is the cross-check with `zkhip_fr_eval_rows_device` at 2^11 rows.

Shapes: 2^3 rows (less than a wavefront), 2^6 (one wavefront), 2^8 (one workgroup), 2^9 (two workgroups), 2^11 (several); ranges that start
and end on and next to the wavefront (63 / 64) and workgroup (255 / 256) borders; result registers 5 / 7 / 11 / 15 so that each of the four
kernel variants (6, 8, 12, 16 registers) runs."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F, mock as M
from zksnap_circuits_halo2_amd.tensors import fr_words

pytestmark = pytest.mark.gpu
R = F.R_MOD
DEV = torch.device("cuda", 0)
words = functools.partial(fr_words, device=DEV)
NONE = (1 << 64) - 1
PATTERN = 0x5A5A5A5A5A5A5A5A
EINVAL = -1
REGS = (5, 7, 11, 15)


def reports_buffer(count):
    return torch.full((max(count, 1), 2), PATTERN, dtype=torch.int64, device=DEV)


def read(buf, count):
    torch.cuda.synchronize()
    a = buf.cpu().numpy().view(np.uint64)
    return [(int(a[i, 0]), int(a[i, 1])) for i in range(count)]


def check(progs, cols, k, row0, count):
    buf = reports_buffer(len(progs))
    M.enqueue_check_rows(progs, cols, k, row0, count, buf.data_ptr())
    return read(buf, len(progs))


def expected(planted, row0, count):
    hit = sorted(r for r in planted if row0 <= r < row0 + count)
    return (len(hit), hit[0] if hit else NONE)


def mov(col, reg):
    p = E.RowProgram()
    p.emit(E.OP_MOV, reg, p.column(col))
    p.result_reg = reg
    return p


def ranges(k):
    n = 1 << k
    out = [(0, n), (0, 1), (n - 1, 1), (0, n - 6)]
    if n >= 64:
        out.append((1, 62))
    if n >= 128:
        out.append((63, 2))
    if n >= 512:
        out.append((255, 2))
    return out


@pytest.mark.parametrize("k", [3, 6, 8, 9, 11])
def test_planted_rows_at_the_borders_of_every_range(k):
    n = 1 << k
    rng = random.Random(0xC0 + k)
    zero, ones = words([0] * n), words([1] * n)
    for i, (row0, count) in enumerate(ranges(k)):
        reg = REGS[i % 4]
        # nothing planted: no failure; every row planted: (count, row0)
        assert check([mov(0, reg)], [zero], k, row0, count) == [(0, NONE)]
        assert check([mov(0, reg)], [ones], k, row0, count) == [(count, row0)]
        # the first and the last row of the range, the rows just outside it, both sides of the wavefront and the workgroup border
        outside = {r for r in (row0 - 1, row0 + count) if 0 <= r < n}
        for planted in ({row0}, {row0 + count - 1}, outside, {row0, row0 + count - 1} | outside, {r for r in (63, 64, 255, 256) if r < n},
                        {r for r in (row0 - 1, row0 + count - 1) if r >= 0}):
            vals = [0] * n
            for r in planted:
                vals[r] = rng.randrange(1, R)
            got = check([mov(0, reg)], [words(vals)], k, row0, count)
            assert got == [expected(planted, row0, count)], (k, row0, count, sorted(planted), reg)
        if outside:
            vals = [0] * n
            for r in outside:
                vals[r] = 1
            assert check([mov(0, reg)], [words(vals)], k, row0, count) == [(0, NONE)]      # rows next to the range are not reported


@pytest.mark.parametrize("n_progs", [1, 2, 5, 257])
def test_programs_side_by_side_fail_at_their_own_rows(n_progs):
    k, n = 9, 512
    rng = random.Random(n_progs)
    n_cols = min(n_progs, 7)
    planted = [set(rng.sample(range(n), rng.choice([0, 1, 3, 70]))) for _ in range(n_cols)]
    planted[0] = {300, 17, 511} if n_progs > 1 else {256}
    cols = []
    for c in range(n_cols):
        vals = [0] * n
        for r in planted[c]:
            vals[r] = rng.randrange(1, R)
        cols.append(words(vals))
    progs = [mov(p % n_cols, REGS[(p // n_cols) % 4] if n_progs > 2 else 5) for p in range(n_progs)]
    for row0, count in ((0, n), (18, 283), (256, 256)):
        got = check(progs, cols, k, row0, count)
        assert got == [expected(planted[p % n_cols], row0, count) for p in range(n_progs)], (row0, count)


@pytest.mark.parametrize("reg", REGS)
def test_each_kernel_variant_counts_and_finds_the_first(reg):
    k, n = 9, 512
    planted = {63, 64, 255, 256, 300}
    vals = [0] * n
    for r in planted:
        vals[r] = r + 1
    col = words(vals)
    for row0, count in ((0, n), (64, 192), (64, 193), (257, 255)):
        assert check([mov(0, reg)], [col], k, row0, count) == [expected(planted, row0, count)], (reg, row0, count)


def test_rotation_wraps_past_the_last_row():
    k, n = 8, 256
    rng = random.Random(3)
    a = [rng.randrange(R) for _ in range(n)]
    b = [a[(r + 3) % n] for r in range(n)]
    planted = {10, 253, 254}                     # rows 253 and 254 read rows 0 and 1
    for r in planted:
        b[r] = (b[r] + 1) % R
    gate = E.RowProgram()                        # a[row + 3] - b[row]
    gate.emit(E.OP_SUB, 0, gate.column(0, 3), gate.column(1, 0))
    cols = [words(a), words(b)]
    for row0, count in ((0, n), (250, 6), (253, 3), (255, 1), (0, 253)):
        assert check([gate], cols, k, row0, count) == [expected(planted, row0, count)], (row0, count)
    a2 = list(a)
    a2[1] = (a2[1] + 5) % R                      # seen through the wrap only: row 254 reads it (already failing), and so does no other row
    a2[2] = (a2[2] + 5) % R                      # row 255 reads row 2
    assert check([gate], [words(a2), cols[1]], k, 0, n) == [expected(planted | {255}, 0, n)]


@pytest.mark.parametrize("k,row0,count", [(9, 100, 300), (9, 1, 511), (13, 4090, 20), (13, 8191, 1)])
def test_rowpow_is_omega_to_the_global_row(k, row0, count):
    n = 1 << k
    omega = F.omega_for(k)
    pw, vals = 1, []
    for _ in range(n):
        vals.append(pw)
        pw = pw * omega % R
    planted = {row0, row0 + count - 1, row0 + count // 2} | ({row0 - 1} if row0 else set())
    for r in planted:
        vals[r] = (vals[r] + 1) % R
    prog = E.RowProgram(omega=omega)             # col - omega^row
    prog.emit(E.OP_SUB, 6, prog.column(0), E.RowProgram.ROWPOW)
    prog.result_reg = 6
    assert check([prog], [words(vals)], k, row0, count) == [expected(planted, row0, count)]


def test_lazy_zeros_count_as_zero():
    """results that reach the end of a program as 2r, r or another non-canonical form of zero"""
    k, n = 8, 256
    rng = random.Random(11)
    a = [rng.randrange(R) for _ in range(n)]
    b = [rng.randrange(R) for _ in range(n)]
    a[0], a[1], b[2] = 0, R - 1, R - 1
    neg_a = [-v % R for v in a]
    neg_ab = [-(x * y) % R for x, y in zip(a, b)]
    cols = [words(a), words(a), words(neg_a), words(b), words([0] * n), words(neg_ab)]
    reg = E.RowProgram.reg
    progs = []
    p = E.RowProgram(); p.emit(E.OP_SUB, 0, p.column(0), p.column(1)); progs.append(p)                              # a - b with a == b
    p = E.RowProgram(); p.emit(E.OP_ADD, 0, p.column(0), p.column(2)); progs.append(p)                              # a + (-a)
    p = E.RowProgram(); p.emit(E.OP_MUL, 0, p.column(3), p.column(4)); progs.append(p)                              # x * 0 (a column)
    p = E.RowProgram(); p.emit(E.OP_MUL, 0, p.column(3), p.constant(0)); progs.append(p)                            # x * 0 (a constant)
    p = E.RowProgram(); p.emit(E.OP_MAD, 0, p.column(0), p.column(3), p.column(5)); progs.append(p)                 # a b + (-(a b))
    p = E.RowProgram(); p.emit(E.OP_NEG, 0, p.column(4)); progs.append(p)                                           # -0
    p = E.RowProgram(); p.emit(E.OP_MOV, 1, p.column(0)); p.emit(E.OP_NEG, 2, reg(1)); p.emit(E.OP_ADD, 0, reg(1), reg(2)); progs.append(p)
    p = E.RowProgram(); p.emit(E.OP_MOV, 1, p.column(0)); p.emit(E.OP_DBL, 2, reg(1)); p.emit(E.OP_SUB, 2, reg(2), reg(1)); p.emit(E.OP_SUB, 0, reg(2), reg(1))
    progs.append(p)                                                                                                 # 2a - a - a
    p = E.RowProgram(); p.emit(E.OP_MOV, 1, p.column(0)); p.emit(E.OP_SQR, 2, reg(1)); p.emit(E.OP_MUL, 3, reg(1), reg(1)); p.emit(E.OP_SUB, 0, reg(2), reg(3))
    progs.append(p)                                                                                                 # a^2 - a a
    p = E.RowProgram(); p.emit(E.OP_MOV, 0, E.RowProgram.PREV); progs.append(p)                                     # there is no previous value: 0
    assert check(progs, cols, k, 0, n) == [(0, NONE)] * len(progs)
    for q in progs:                              # ... one at a time as well
        assert check([q], cols, k, 0, n) == [(0, NONE)]
    # and the same programs do see a difference of one
    a1 = list(a)
    a1[77] = (a1[77] + 1) % R
    got = check(progs[:2], [words(a1)] + cols[1:], k, 0, n)
    assert got == [(1, 77), (1, 77)]


def test_argument_errors_leave_the_records_untouched(lib):
    k, n = 6, 64
    col = words([1] * n)
    ptrs = (C.c_void_p * 1)(col.data_ptr())
    good, keep = mov(0, 5)._marshal()
    bad_reg = mov(0, 5)
    bad_reg.result_reg = 16
    bad_col = mov(3, 5)                          # reads column 3 of 1
    untouched = [(PATTERN, PATTERN)] * 2

    def call(prog, n_progs, row0, count, reports=None, columns=ptrs):
        buf = reports_buffer(2)
        arr = (_lib.VmProgram * 2)(prog, prog)
        rc = lib.zkhip_check_rows_device(arr, n_progs, columns, 1, k, row0, count, C.c_void_p(buf.data_ptr() if reports is None else reports), None)
        return rc, read(buf, 2)

    assert call(good, 2, 0, n) == (0, [(n, 0), (n, 0)])
    for args in ((good, 2, 0, 0), (good, 2, 0, n + 1), (good, 2, n, 1), (good, 2, 1, n), (good, 2, (1 << 64) - 1, 2), (good, 0, 0, n), (good, 65536, 0, n)):
        rc, rec = call(*args)
        assert rc == EINVAL and rec == untouched, args
    for prog in (bad_reg, bad_col):
        p, keep2 = prog._marshal()
        assert lib.zkhip_fr_eval_rows_device(C.byref(p), ptrs, 1, k, 0, C.c_void_p(reports_buffer(n * 2).data_ptr()), None) == EINVAL      # the evaluator rejects it
        rc, rec = call(p, 2, 0, n)
        assert rc == EINVAL and rec == untouched
        del keep2
    assert call(good, 2, 0, n, reports=0)[0] == EINVAL
    assert call(good, 2, 0, n, columns=None)[0] == EINVAL
    del keep


def test_counts_equal_the_nonzero_rows_of_the_evaluator():
    """2^11 rows, gate-shaped programs with rotations: what the check counts is what `zkhip_fr_eval_rows_device` writes as non-zero"""
    k, n = 11, 2048
    rng = random.Random(2048)
    G = 3
    sel = [[1 if (r % 4 == 0 and rng.random() < 0.9) else 0 for r in range(n)] for _ in range(G)]
    adv = [[rng.randrange(R) for _ in range(n)] for _ in range(G)]
    for g in range(G):
        for r in range(0, n - 3, 4):
            if rng.random() < 0.8:               # most gates hold
                adv[g][r + 3] = (adv[g][r] + adv[g][r + 1] * adv[g][r + 2]) % R
    cs = E.ConstraintSystem(num_fixed=G, num_advice=G, gates=[[E.Fixed(i) * (E.Advice(i, 0) + E.Advice(i, 1) * E.Advice(i, 2) - E.Advice(i, 3))] for i in range(G)] +
                            [[E.Fixed(1, 5) * (E.Advice(0, -1) * E.Advice(1, 2) - E.Advice(2, 0))]])      # rotations -1, 2 and 5, selected on a fifth of the rows
    progs = M.gate_programs(cs)
    cols = [words(c) for c in sel + adv]
    out = torch.empty((n, 4), dtype=torch.int64, device=DEV)
    nonzero = []
    for p in progs:
        p.run_device([c.data_ptr() for c in cols], k, out.data_ptr())
        torch.cuda.synchronize()
        nonzero.append(sorted(torch.nonzero((out != 0).any(dim=1)).flatten().tolist()))
    assert all(0 < len(z) < n for z in nonzero)
    for row0, count in ((0, n), (0, n - 6), (700, 801)):
        got = check(progs, cols, k, row0, count)
        assert got == [expected(z, row0, count) for z in nonzero], (row0, count)
    # the first gate against Python integers as well
    want = [r for r in range(n) if sel[0][r] * (adv[0][r] + adv[0][(r + 1) % n] * adv[0][(r + 2) % n] - adv[0][(r + 3) % n]) % R]
    assert nonzero[0] == want

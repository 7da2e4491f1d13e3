"""GPU: `zkhip_check_copies_device` -- how many cells of the permutation's columns differ from the cell they are mapped to, and which is the
first (column 2^log_n + row).  Expected values come from `mock.verify_host` (Python integers) or from positions the test planted."""
import functools
import random

import numpy as np
import pytest
import torch

from zksnap_circuits_halo2_amd import evaluation as E, fields as F, mock as M
from zksnap_circuits_halo2_amd.keygen import Assembly
from zksnap_circuits_halo2_amd.tensors import fr_words

pytestmark = pytest.mark.gpu
R = F.R_MOD
DEV = torch.device("cuda", 0)
words = functools.partial(fr_words, device=DEV)
NONE = (1 << 64) - 1
PATTERN = 0x5A5A5A5A5A5A5A5A


def check(cols, k, map_col, map_row):
    """cols: device tensors; map_col / map_row: [columns][2^k] integer arrays, uploaded as u32 in the layout keygen uploads them"""
    mc = torch.from_numpy(np.ascontiguousarray(np.asarray(map_col, dtype=np.uint32)).view(np.int32)).to(DEV)
    mr = torch.from_numpy(np.ascontiguousarray(np.asarray(map_row, dtype=np.uint32)).view(np.int32)).to(DEV)
    buf = torch.full((1, 2), PATTERN, dtype=torch.int64, device=DEV)
    M.enqueue_check_copies(cols, k, mc.data_ptr(), mr.data_ptr(), buf.data_ptr())
    torch.cuda.synchronize()
    a = buf.cpu().numpy().view(np.uint64)
    return int(a[0, 0]), int(a[0, 1])


def host(values, k, asm):
    """(failures, first) from verify_host over a circuit that is nothing but the permutation"""
    nc = len(values)
    cs = E.ConstraintSystem(num_fixed=0, num_advice=nc, permutation_columns=[("advice", i) for i in range(nc)])
    got = M.verify_host(cs, k, [], values, (), asm)
    if not got:
        return (0, NONE)
    (kind, c, r, failures), = got
    assert kind == "copy"
    return (failures, (c << k) + r)


def cycles_for(nc, n, rng):
    """a 3-cycle through cell 0, a 3-cycle through the last cell of the last column, a 2-cycle; with room for them, another 3-cycle and a 2-cycle
    inside one column.  No cell is in two cycles."""
    middle = [(c, r) for c in range(nc) for r in range(n)][1:-1]
    rng.shuffle(middle)
    take = middle.pop
    out = [[(0, 0), take(), take()], [take(), take(), (nc - 1, n - 1)], [take(), take()]]
    if len(middle) >= 8:
        out.append([take(), take(), take()])
        a = take()
        b = next(cell for cell in middle if cell[0] == a[0])
        middle.remove(b)
        out.append([a, b])
    return out


def build(nc, k, seed):
    n = 1 << k
    rng = random.Random(seed)
    values = [[rng.randrange(R) for _ in range(n)] for _ in range(nc)]
    asm = Assembly(n, nc)
    cycles = cycles_for(nc, n, rng)
    for cyc in cycles:
        v = rng.randrange(R)
        for c, r in cyc:
            values[c][r] = v
        for (c1, r1), (c2, r2) in zip(cyc, cyc[1:]):
            asm.copy(c1, r1, c2, r2)
    return values, asm, cycles


@pytest.mark.parametrize("k", [3, 6, 8, 10])
@pytest.mark.parametrize("nc", [1, 3, 9])
def test_cycles_hold_and_a_changed_cell_is_found(nc, k):
    n = 1 << k
    values, asm, cycles = build(nc, k, 100 * nc + k)
    ident = Assembly(n, nc)
    dev = [words(v) for v in values]
    assert check(dev, k, ident.map_col, ident.map_row) == (0, NONE)                 # the identity mapping constrains nothing
    assert check(dev, k, asm.map_col, asm.map_row) == host(values, k, asm) == (0, NONE)
    three = [cyc for cyc in cycles if len(cyc) == 3]
    assert three and cycles[0][0] == (0, 0)
    for cyc in three:                                   # one cell of a 3-cycle changed, each cell in turn
        for c, r in cyc:
            bad = [list(v) for v in values]
            bad[c][r] = (bad[c][r] + 1) % R
            want = host(bad, k, asm)
            assert want[0] == 2                         # the changed cell and the cell that maps to it
            dev_bad = list(dev)
            dev_bad[c] = words(bad[c])
            assert check(dev_bad, k, asm.map_col, asm.map_row) == want, (cyc, c, r)
    # cell 0 and the last cell of the last column, by hand
    bad = [list(v) for v in values]
    bad[0][0] = (bad[0][0] + 1) % R
    got = check([words(bad[0])] + dev[1:], k, asm.map_col, asm.map_row)
    assert got == host(bad, k, asm) and got[1] == 0
    last = next(cyc for cyc in cycles if (nc - 1, n - 1) in cyc)
    bad = [list(v) for v in values]
    for c, r in last[:-1]:
        bad[c][r] = (bad[c][r] + 1) % R                 # the other two cells change together: the last cell and the one mapping to it fail
    got = check([words(v) for v in bad], k, asm.map_col, asm.map_row)
    assert got == host(bad, k, asm) and got[0] == 2
    everything = [[(v + c + 1) % R for v in col] for c, col in enumerate(values)]      # several cycles broken at once
    for cyc in cycles:
        c, r = cyc[0]
        everything[c][r] = (everything[c][r] + 7) % R
    got = check([words(v) for v in everything], k, asm.map_col, asm.map_row)
    assert got == host(everything, k, asm) and got[0] > 0


@pytest.mark.parametrize("nc,k", [(1, 3), (3, 6), (9, 8), (3, 10)])
def test_out_of_range_map_entries_are_reduced(nc, k):
    n = 1 << k
    values, asm, cycles = build(nc, k, 7 * nc + k)
    c, r = cycles[0][1]
    values[c][r] = (values[c][r] + 1) % R
    want = host(values, k, asm)
    assert want[0] == 2
    rng = random.Random(k)
    big_col = np.asarray(asm.map_col, dtype=np.uint64) + nc * np.array([[rng.randrange(0, (1 << 31) // nc) for _ in range(n)] for _ in range(nc)], dtype=np.uint64)
    big_row = np.asarray(asm.map_row, dtype=np.uint64) + n * np.array([[rng.randrange(0, (1 << 32) // n) for _ in range(n)] for _ in range(nc)], dtype=np.uint64)
    assert int(big_col.max()) < 1 << 32 and int(big_row.max()) < 1 << 32 and int(big_col.max()) >= nc and int(big_row.min()) >= 0
    dev = [words(v) for v in values]
    assert check(dev, k, big_col, big_row) == check(dev, k, asm.map_col, asm.map_row) == want


@pytest.mark.parametrize("word", [0, 3])
def test_values_that_differ_in_one_word_only(word):
    """raw words, not field encodings: the cells' 32 bytes are compared"""
    k, n, nc = 6, 64, 3
    rng = random.Random(word)
    raw = np.array([[[rng.getrandbits(64) for _ in range(4)] for _ in range(n)] for _ in range(nc)], dtype=np.uint64)
    asm = Assembly(n, nc)
    asm.copy(0, 5, 2, 63)
    asm.copy(1, 0, 1, 40)
    raw[2, 63] = raw[0, 5]
    raw[1, 40] = raw[1, 0]
    cols = lambda a: [torch.from_numpy(a[c].view(np.int64)).to(DEV) for c in range(nc)]
    assert check(cols(raw), k, asm.map_col, asm.map_row) == (0, NONE)
    for bit in (0, 63):
        bad = raw.copy()
        bad[2, 63, word] ^= np.uint64(1 << bit)
        assert check(cols(bad), k, asm.map_col, asm.map_row) == (2, (0 << k) + 5)      # cells (0, 5) and (2, 63)
        bad = raw.copy()
        bad[1, 40, word] ^= np.uint64(1 << bit)
        assert check(cols(bad), k, asm.map_col, asm.map_row) == (2, (1 << k) + 0)


def test_argument_errors_leave_the_record_untouched(lib):
    import ctypes as C

    k, n = 4, 16
    col = words([1] * n)
    asm = Assembly(n, 1)
    mc = torch.from_numpy(np.asarray(asm.map_col, dtype=np.int32)).to(DEV)
    mr = torch.from_numpy(np.asarray(asm.map_row, dtype=np.int32)).to(DEV)
    ptrs = (C.c_void_p * 1)(col.data_ptr())
    null = (C.c_void_p * 1)(None)
    for args in ((ptrs, 0, k, mc.data_ptr(), mr.data_ptr()), (ptrs, 1, 29, mc.data_ptr(), mr.data_ptr()), (ptrs, 1, k, None, mr.data_ptr()),
                 (ptrs, 1, k, mc.data_ptr(), None), (None, 1, k, mc.data_ptr(), mr.data_ptr()), (null, 1, k, mc.data_ptr(), mr.data_ptr()),
                 (ptrs, 4097, k, mc.data_ptr(), mr.data_ptr())):
        buf = torch.full((1, 2), PATTERN, dtype=torch.int64, device=DEV)
        assert lib.zkhip_check_copies_device(args[0], args[1], args[2], C.c_void_p(args[3]), C.c_void_p(args[4]), C.c_void_p(buf.data_ptr()), None) == -1, args[1:3]
        torch.cuda.synchronize()
        assert buf.cpu().numpy().view(np.uint64).tolist() == [[PATTERN, PATTERN]]
    assert lib.zkhip_check_copies_device(ptrs, 1, k, C.c_void_p(mc.data_ptr()), C.c_void_p(mr.data_ptr()), None, None) == -1

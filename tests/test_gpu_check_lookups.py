"""GPU: `zkhip_check_lookups_device` -- per lookup, how many of the usable rows hold an input value that is none of the table's usable rows,
and which is the first.  Expected values come from `mock.verify_host` (Python sets of integers); the last test holds the call against
`zkhip_lookup_permute_many_device`, which fails exactly when a lookup has a missing value and names the lowest such lookup."""
import ctypes as C
import functools
import random
import re

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
K, N = 11, 2048
USABLE = [1, 2, 63, 64, 65, N - 6]
GROUPS = {"shared": lambda l: 0, "distinct": lambda l: l, "aab": lambda l: (0, 0, 1)[l % 3]}


def check(inputs, tables, u, k=K):
    buf = torch.full((max(len(inputs), 1), 2), PATTERN, dtype=torch.int64, device=DEV)
    M.enqueue_check_lookups(inputs, tables, k, u, buf.data_ptr())
    torch.cuda.synchronize()
    a = buf.cpu().numpy().view(np.uint64)
    return [(int(a[i, 0]), int(a[i, 1])) for i in range(len(inputs))]


def host(input_ints, table_ints, group, u, n=N, k=K):
    """[(failures, first)] per lookup from verify_host: a circuit of nothing but lookups whose usable rows are the first u"""
    L, T = len(input_ints), len(table_ints)
    cs = E.ConstraintSystem(num_fixed=T, num_advice=L, lookups=[E.Lookup([E.Advice(l)], [E.Fixed(group[l])]) for l in range(L)], blinding_factors=n - u - 1)
    out = [(0, NONE)] * L
    for kind, l, first, failures in M.verify_host(cs, k, table_ints, input_ints, (), None):
        assert kind == "lookup"
        out[l] = (failures, first)
    return out


def make_table(u, rng, t):
    """duplicates and gaps among the usable rows (values 100 + 3 j + t), one value that occurs behind the usable rows only"""
    m = max(1, (u + 1) // 2)
    usable = [100 + t + 3 * rng.randrange(m) for _ in range(u)]
    usable[0] = 100 + t                                  # the minimum
    usable[-1] = 100 + t + 3 * (m - 1)                   # the maximum (the same cell when u = 1)
    return usable + [7777] * (N - u)


def missing_values(table, u):
    lo, hi = min(table[:u]), max(table[:u])
    return [lo - 1, 0, hi + 1, 1 << 70, lo + 1, 7777]   # below the minimum, above the maximum, inside a gap, behind the usable rows only


@pytest.mark.parametrize("u", USABLE)
@pytest.mark.parametrize("L,combo", [(1, "shared"), (3, "shared"), (3, "distinct"), (3, "aab")])
def test_missing_values_are_counted_per_lookup(L, combo, u):
    rng = random.Random(1000 * L + u + len(combo))
    group = [GROUPS[combo](l) for l in range(L)]
    T = max(group) + 1
    table_ints = [make_table(u, rng, t) for t in range(T)]
    tables = [words(t) for t in table_ints]
    input_ints = []
    for l in range(L):
        t = table_ints[group[l]]
        inp = [t[rng.randrange(u)] for _ in range(u)] + [rng.randrange(R) for _ in range(N - u)]      # the rows behind the usable ones are not looked up
        input_ints.append(inp)
    args = lambda ints: ([words(i) for i in ints], [tables[group[l]] for l in range(L)])
    assert check(*args(input_ints), u) == host(input_ints, table_ints, group, u) == [(0, NONE)] * L
    # each kind of missing value alone, in the last lookup, at the last usable row
    for v in missing_values(table_ints[group[L - 1]], u):
        bad = [list(i) for i in input_ints]
        bad[L - 1][u - 1] = v
        want = host(bad, table_ints, group, u)
        assert want[L - 1] == (1, u - 1) and want[:L - 1] == [(0, NONE)] * (L - 1)
        assert check(*args(bad), u) == want, (v, u)
    # several failing rows in several lookups at once
    bad = [list(i) for i in input_ints]
    for l in range(L):
        miss = missing_values(table_ints[group[l]], u)
        for r in sorted(set(rng.sample(range(u), min(u, 1 + 2 * l)) + ([u - 1, 0] if l == 0 else []))):
            bad[l][r] = miss[rng.randrange(len(miss))]
    want = host(bad, table_ints, group, u)
    assert all(w[0] > 0 for w in want)
    assert check(*args(bad), u) == want


def test_full_width_keys_that_differ_in_the_top_limb_only():
    u = 65
    rng = random.Random(5)
    base = rng.randrange(1 << 190)
    table = [base + ((j % 5) << 192) for j in range(N)]                 # top limbs 0 .. 4
    inp = [table[rng.randrange(u)] for _ in range(N)]
    assert check([words(inp)], [words(table)], u) == [(0, NONE)]
    inp[3] = base + (5 << 192)
    inp[40] = base + (1 << 252)
    inp[64] = base + 1 + (2 << 192)                                     # the low limb differs
    inp[65] = base + (9 << 192)                                         # not a usable row
    assert check([words(inp)], [words(table)], u) == host([inp], [table], [0], u) == [(3, 3)]


def test_no_lookups_and_no_usable_rows(lib):
    t, i = words([1] * 64), words([2] * 64)
    assert check([], [], 10, k=6) == []
    assert check([i, i], [t, t], 0, k=6) == [(0, NONE)] * 2             # nothing to look up: the records say "no failure"
    ptrs = (C.c_void_p * 2)(i.data_ptr(), i.data_ptr())
    tabs = (C.c_void_p * 2)(t.data_ptr(), None)
    for args in ((ptrs, tabs, 2, 6, 10), (ptrs, ptrs, 2, 6, 65), (ptrs, ptrs, 2, 29, 10), (None, ptrs, 2, 6, 10), (ptrs, ptrs, 1366, 6, 10)):
        buf = torch.full((2, 2), PATTERN, dtype=torch.int64, device=DEV)
        assert lib.zkhip_check_lookups_device(args[0], args[1], args[2], args[3], args[4], C.c_void_p(buf.data_ptr()), None) == -1, args[2:]
        torch.cuda.synchronize()
        assert buf.cpu().numpy().view(np.uint64).tolist() == [[PATTERN, PATTERN]] * 2
    assert lib.zkhip_check_lookups_device(ptrs, ptrs, 2, 6, 10, None, None) == -1


@pytest.mark.parametrize("u", [64, N - 6])
def test_agrees_with_the_permute_call(lib, u):
    """zkhip_lookup_permute_many_device returns ZKHIP_EINVAL exactly when some record has failures, and names the lowest such lookup"""
    rng = random.Random(u)
    L = 3
    table_ints = [make_table(u, rng, 0), make_table(u, rng, 1)]
    tables = [words(t) for t in table_ints]
    group = [0, 0, 1]
    good = [[table_ints[group[l]][rng.randrange(u)] for _ in range(N)] for l in range(L)]
    for failing in ((), (2,), (1, 2), (0,), (0, 1, 2)):
        ints = [list(i) for i in good]
        for l in failing:
            ints[l][rng.randrange(u)] = 7777
        inputs = [words(i) for i in ints]
        tabs = [tables[g] for g in group]
        got = check(inputs, tabs, u)
        assert got == host(ints, table_ints, group, u)
        assert [l for l in range(L) if got[l][0]] == list(failing)
        pa = torch.zeros((L, N, 4), dtype=torch.int64, device=DEV)
        ps = torch.zeros((L, N, 4), dtype=torch.int64, device=DEV)
        ip = (C.c_void_p * L)(*[t.data_ptr() for t in inputs])
        tp = (C.c_void_p * L)(*[t.data_ptr() for t in tabs])
        rc = lib.zkhip_lookup_permute_many_device(ip, tp, L, K, u, C.c_void_p(pa.data_ptr()), C.c_void_p(ps.data_ptr()), None)
        assert (rc == -1) == bool(failing) and rc in (0, -1)
        if failing:
            named = re.search(r"lookup (\d+)", lib.zkhip_last_error().decode())
            assert named and int(named.group(1)) == failing[0]

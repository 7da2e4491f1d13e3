"""GPU: the lookup argument of every lookup of a circuit in one call (`zkhip_lookup_permute_many_device`, `zkhip_lookup_products_device`).
Every comparison is of bytes: against the single-lookup entry points (`zkhip_lookup_permute_device`; `lookup_product_programs` +
`zkhip_fr_grand_product_device`), against the oracle, and at the proof level through tools/prove_flow.py.

Switches of method inside the two calls, each with a size on both sides here:
  scan_one_tile / scan_two_levels      the slot scans of the permute call: u + 1 <= 2048 entries are one workgroup, more take a second level
  scan_two_levels / scan_three_levels  ... and more than 2048^2 entries a third (u = 2^22 - 1 against u = 2^22)
  single_call_route                    the Python mirror hands ONE lookup of 2^20 usable rows or more to the single-lookup call (same bytes)
  product_levels                       the prefix product of the products call adds a level at n = 32, 512, 8192, 2^17 (16 elements per thread)"""
import ctypes as C
import functools
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F
from zksnap_circuits_halo2_amd.tensors import fr_from_small, fr_ints as ints, fr_words

pytestmark = pytest.mark.gpu
R = F.R_MOD
DEV = torch.device("cuda", 0)
words = functools.partial(fr_words, device=DEV)
BETA, GAMMA, THETA = 0x1234567 * 0x10001 + (1 << 200), (1 << 250) + 99, 7
SENTINEL = 0x5E5E5E5E5E5E5E5E5E5E5E5E5E5E5E5E


def small_ints(v, k):
    """int64 device tensor of n = 2^k small non-negative integers -> Montgomery words, on the current stream"""
    return fr_from_small(v, k, stream=torch.cuda.current_stream().cuda_stream)


def sentinel(shape_rows, count=None):
    row = words([SENTINEL])[0]
    shape = (shape_rows, 4) if count is None else (count, shape_rows, 4)
    return row.expand(shape).contiguous()


def make_columns(shape, n, u, rng):
    """(input ints, table ints), n each; the inputs' first u rows hold values of the table's first u rows only"""
    if shape == "range":            # i mod 2^bits: duplicate table values, and many zeros among the inputs (padding)
        bits = min(8, max(0, u.bit_length() - 1))
        table = [i % (1 << bits) for i in range(n)]
        inp = [rng.randrange(1 << bits) if rng.random() < 0.5 else 0 for _ in range(n)]
    elif shape == "full":           # full-width random values
        table = [rng.randrange(R) for _ in range(n)]
        inp = [table[rng.randrange(u)] for _ in range(n)]
    elif shape == "straddle":       # on both sides of 2^64
        table = [(1 << 64) + (i % 9) - 4 for i in range(n)]
        inp = [table[rng.randrange(u)] for _ in range(n)]
    elif shape == "equal":          # all inputs of the column equal
        table = [rng.randrange(1 << 70) for _ in range(n)]
        inp = [table[rng.randrange(u)]] * n
    else:                           # "distinct": every input distinct
        assert shape == "distinct"
        table = [(i << 34) + rng.randrange(1 << 34) for i in rng.sample(range(1 << 26), n)]
        inp = table[:u]
        rng.shuffle(inp)
        inp = inp + table[u:]
    return inp, table


def build(L, combo, shape, n, u, seed):
    """device columns of L lookups: combo = shared (one table), distinct (a table each), aab (A, A, B, A, A, B, ...)"""
    rng = random.Random(seed)
    groups = {"shared": [0] * L, "distinct": list(range(L)), "aab": [(0, 0, 1)[l % 3] for l in range(L)]}[combo]
    tables, table_ints = {}, {}
    inputs, input_ints, tabs = [], [], []
    for l in range(L):
        g = groups[l]
        if g not in tables:
            _, t = make_columns(shape, n, u, random.Random(seed * 1000 + g))
            table_ints[g], tables[g] = t, words(t)
        t = table_ints[g]
        if shape == "range":
            i, _ = make_columns(shape, n, u, rng)
        elif shape == "equal":
            i = [t[rng.randrange(u)]] * n
        elif shape == "distinct":
            i = t[:u]
            rng.shuffle(i)
            i = i + t[u:]
        else:
            i = [t[rng.randrange(u)] for _ in range(n)]
        inputs.append(words(i)); input_ints.append(i); tabs.append(tables[g])
    return inputs, tabs, input_ints, [table_ints[g] for g in groups]


def single_permute(lib, lk, table, u, n):
    pa, ps = sentinel(n), sentinel(n)
    _lib.check(lib.zkhip_lookup_permute_device(lk.data_ptr(), table.data_ptr(), u, pa.data_ptr(), ps.data_ptr(), None))
    return pa, ps


_PROGS = {}


def composed_product(lib, lk, table, pa, ps, k):
    if "p" not in _PROGS:
        _PROGS["p"] = E.lookup_product_programs(1, 1, BETA, GAMMA, THETA)
    pn, pd = _PROGS["p"]
    n = 1 << k
    zl, den = torch.empty((n, 4), dtype=torch.int64, device=DEV), torch.empty((n, 4), dtype=torch.int64, device=DEV)
    pn.run_device([lk.data_ptr(), table.data_ptr()], k, zl.data_ptr())
    pd.run_device([pa.data_ptr(), ps.data_ptr()], k, den.data_ptr())
    _lib.check(lib.zkhip_fr_grand_product_device(zl.data_ptr(), den.data_ptr(), n, zl.data_ptr(), None))
    return zl


def check_case(lib, L, combo, shape, k, u, seed, oracle_permute=True, oracle_product=False):
    n = 1 << k
    inputs, tabs, input_ints, table_ints = build(L, combo, shape, n, u, seed)
    pa, ps = E.permute_expression_pairs_device(inputs, tabs, u, k, sentinel(n, L), sentinel(n, L))
    sent = sentinel(n)
    for l in range(L):
        ra, rs = single_permute(lib, inputs[l], tabs[l], u, n)
        assert torch.equal(pa[l, :u], ra[:u]) and torch.equal(ps[l, :u], rs[:u]), f"lookup {l}: differs from zkhip_lookup_permute_device"
        assert torch.equal(pa[l, u:], sent[u:]) and torch.equal(ps[l, u:], sent[u:]), f"lookup {l}: rows >= usable_rows were written"
        if oracle_permute:
            ea, es = O.permute_expression_pair(input_ints[l], table_ints[l], u)
            assert ints(pa[l, :u]) == ea and ints(ps[l, :u]) == es, f"lookup {l}: differs from the oracle"
    z = E.lookup_products_device(inputs, tabs, pa, ps, u, k, BETA, GAMMA)
    for l in range(L):
        ref = composed_product(lib, inputs[l], tabs[l], pa[l], ps[l], k)
        assert torch.equal(z[l, :min(u + 1, n)], ref[:min(u + 1, n)]), f"lookup {l}: z differs from the row programs + zkhip_fr_grand_product_device"
        if u < n:
            assert torch.equal(z[l, u:], z[l, u:u + 1].expand(n - u, 4)), f"lookup {l}: the rows after usable_rows do not repeat z[usable_rows]"
        if oracle_product:
            a, s = input_ints[l][:u], table_ints[l][:u]
            ap, sp = ints(pa[l, :u]), ints(ps[l, :u])
            ez = O.grand_product([(x + BETA) * (y + GAMMA) % R for x, y in zip(a, s)], [(x + BETA) * (y + GAMMA) % R for x, y in zip(ap, sp)] )
            got = ints(z[l, :min(u + 1, n)])
            assert got[:u] == ez[:u], f"lookup {l}: z differs from O.grand_product"
            if u < n:
                assert got[u] == 1, f"lookup {l}: the product does not close"


LS = (1, 2, 3, 8, 11)
COMBOS = ("shared", "distinct", "aab")
SHAPES = ("range", "full", "straddle", "equal", "distinct")


def _usable(n):
    return sorted({u for u in (1, 2, n - 6, n) if 1 <= u <= n})


def _grid():
    cases, i = [], 0
    for L in LS:                                    # every lookup count with every table combination, every key shape in turn
        for combo in COMBOS:
            cases.append((L, combo, SHAPES[i % 5], 10, (1 << 10) - 6)); i += 1
    for k in (1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 13, 14, 16, 17):      # n from 2 up; 4/5, 8/9, 12/13, 16/17: product_levels
        for u in _usable(1 << k):
            cases.append((LS[i % 5] if k <= 14 else min(LS[i % 5], 3), COMBOS[i % 3], SHAPES[i % 5], k, u)); i += 1
    for shape in SHAPES:                            # every key shape at L = 8 on the voter's rows
        cases.append((8, "aab", shape, 13, (1 << 13) - 6))
    return cases


@pytest.mark.parametrize("L,combo,shape,k,u", _grid())
def test_matches_single_calls_and_oracle(lib, L, combo, shape, k, u):
    check_case(lib, L, combo, shape, k, u, seed=k * 100003 + u * 17 + L, oracle_permute=k <= 14, oracle_product=k <= 9)


@pytest.mark.parametrize("name,k,u", [("scan_one_tile", 11, 2046), ("scan_one_tile", 11, 2047), ("scan_two_levels", 11, 2048),
                                      ("scan_two_levels", 12, 2049), ("scan_one_tile", 12, 2047)])
@pytest.mark.parametrize("shape", ["range", "full"])
def test_scan_depth_switch(lib, name, k, u, shape):
    check_case(lib, 3, "aab", shape, k, u, seed=u)


def _range_columns(k, L, bits, seed):
    n = 1 << k
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    rows = torch.arange(n, dtype=torch.int64, device=DEV)
    tv = rows % (1 << bits)
    ivs = []
    for _ in range(L):
        iv = torch.randint(0, 1 << bits, (n,), dtype=torch.int64, device=DEV, generator=g)
        iv[torch.rand(n, device=DEV, generator=g) < 0.4] = 0                                  # padding zeros: one heavy slot
        ivs.append(iv)
    return tv, ivs, small_ints(tv, k), [small_ints(iv, k) for iv in ivs]


def test_2p20_against_numpy_oracle_and_single_call(lib):
    k, L = 20, 2
    n, u = 1 << k, (1 << k) - 6
    tv, ivs, table, inputs = _range_columns(k, L, 16, 20)
    pa, ps = E.permute_expression_pairs_device(inputs, [table] * L, u, k, sentinel(n, L), sentinel(n, L))
    z = E.lookup_products_device(inputs, [table] * L, pa, ps, u, k, BETA, GAMMA)
    for l in range(L):
        ea, es = O.permute_expression_pair_np(ivs[l].cpu().numpy(), tv.cpu().numpy(), u)
        assert torch.equal(pa[l, :u], small_ints(torch.from_numpy(np.concatenate([ea, np.zeros(n - u, dtype=np.int64)])).to(DEV), k)[:u])
        assert torch.equal(ps[l, :u], small_ints(torch.from_numpy(np.concatenate([es, np.zeros(n - u, dtype=np.int64)])).to(DEV), k)[:u])
        ra, rs = single_permute(lib, inputs[l], table, u, n)
        assert torch.equal(pa[l, :u], ra[:u]) and torch.equal(ps[l, :u], rs[:u])
        assert torch.equal(pa[l, u:], ra[u:]) and torch.equal(ps[l, u:], rs[u:])               # the sentinel rows
        ref = composed_product(lib, inputs[l], table, pa[l], ps[l], k)
        assert torch.equal(z[l, :u + 1], ref[:u + 1]) and torch.equal(z[l, u:], z[l, u:u + 1].expand(n - u, 4))
        assert ints(z[l, u:u + 1]) == [1]


@pytest.mark.parametrize("name,u", [("scan_two_levels", (1 << 22) - 1), ("scan_three_levels", 1 << 22)])
def test_scan_third_level_switch(lib, name, u):
    k = 22
    n = 1 << k
    tv, ivs, table, inputs = _range_columns(k, 1, 18, u)
    pa, ps = sentinel(n, 1), sentinel(n, 1)          # the C entry point itself: the Python mirror hands one lookup of this size to the single call
    iptr, tptr = (C.c_void_p * 1)(inputs[0].data_ptr()), (C.c_void_p * 1)(table.data_ptr())
    _lib.check(lib.zkhip_lookup_permute_many_device(iptr, tptr, 1, k, u, pa.data_ptr(), ps.data_ptr(), None))
    ra, rs = single_permute(lib, inputs[0], table, u, n)
    assert torch.equal(pa[0], ra) and torch.equal(ps[0], rs)
    qa, qs = E.permute_expression_pairs_device(inputs, [table], u, k, sentinel(n, 1), sentinel(n, 1))          # ... with the same bytes
    assert torch.equal(qa, pa) and torch.equal(qs, ps)
    z = E.lookup_products_device(inputs, [table], pa, ps, u, k, BETA, GAMMA)
    ref = composed_product(lib, inputs[0], table, pa[0], ps[0], k)
    assert torch.equal(z[0, :min(u + 1, n)], ref[:min(u + 1, n)])


@pytest.mark.parametrize("name,u", [("many_lookup_call", (1 << 20) - 6), ("single_call_route", 1 << 20)])
def test_single_lookup_route(lib, name, u):
    k = 20
    n = 1 << k
    assert (u >= E.SINGLE_LOOKUP_ROWS) == (name == "single_call_route")
    tv, ivs, table, inputs = _range_columns(k, 1, 12, u)
    pa, ps = E.permute_expression_pairs_device(inputs, [table], u, k, sentinel(n, 1), sentinel(n, 1))
    ra, rs = single_permute(lib, inputs[0], table, u, n)
    assert torch.equal(pa[0], ra) and torch.equal(ps[0], rs)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def _five(k=10):
    n, u = 1 << k, (1 << k) - 6
    inputs, tabs, ii, ti = build(5, "aab", "range", n, u, 5)
    return n, u, k, inputs, tabs


@pytest.mark.parametrize("bad,lowest", [((2,), 2), ((1, 3), 1), ((3, 1), 1), ((4, 0), 0)])
def test_missing_value_names_the_lowest_lookup_and_the_next_call_works(lib, bad, lowest):
    n, u, k, inputs, tabs = _five()
    good = [c.clone() for c in inputs]
    for l in bad:
        inputs[l][(37 * (l + 1)) % u] = words([1 << 8])[0]                 # the table is 0 .. 255
    iptr = (C.c_void_p * 5)(*[c.data_ptr() for c in inputs])
    tptr = (C.c_void_p * 5)(*[c.data_ptr() for c in tabs])
    pa, ps = sentinel(n, 5), sentinel(n, 5)
    rc = lib.zkhip_lookup_permute_many_device(iptr, tptr, 5, k, u, pa.data_ptr(), ps.data_ptr(), None)
    assert rc == -1                                                       # ZKHIP_EINVAL, from the call itself
    msg = lib.zkhip_last_error().decode()
    m = re.search(r"lookup (\d+)", msg)
    assert m and int(m.group(1)) == lowest, msg
    with pytest.raises(_lib.ZkhipError):
        E.permute_expression_pairs_device(inputs, tabs, u, k)
    pa, ps = E.permute_expression_pairs_device(good, tabs, u, k, sentinel(n, 5), sentinel(n, 5))     # a correct call right after it
    for l in range(5):
        ra, rs = single_permute(lib, good[l], tabs[l], u, n)
        assert torch.equal(pa[l], ra) and torch.equal(ps[l], rs)


def test_wide_input_against_a_narrow_table_is_an_error(lib):
    n, u, k, inputs, tabs = _five()
    inputs[0][11] = words([(1 << 64) + 5])[0]                                # its low 64 bits are in the table
    with pytest.raises(_lib.ZkhipError, match=r"lookup 0"):
        E.permute_expression_pairs_device(inputs, tabs, u, k)
    inputs[0][11] = words([(1 << 192) + 5])[0]
    with pytest.raises(_lib.ZkhipError, match=r"lookup 0"):
        E.permute_expression_pairs_device(inputs, tabs, u, k)


def test_argument_errors_and_empty_calls(lib):
    n, u, k, inputs, tabs = _five()
    iptr = (C.c_void_p * 5)(*[c.data_ptr() for c in inputs])
    tptr = (C.c_void_p * 5)(*[c.data_ptr() for c in tabs])
    pa, ps, z = sentinel(n, 5), sentinel(n, 5), sentinel(n, 5)
    b, g = F.fr_encode([BETA])[0], F.fr_encode([GAMMA])[0]
    P = lambda *a: lib.zkhip_lookup_permute_many_device(*a)
    Z = lambda *a: lib.zkhip_lookup_products_device(*a)
    assert P(iptr, tptr, 0, k, u, pa.data_ptr(), ps.data_ptr(), None) == 0 and P(iptr, tptr, 5, k, 0, pa.data_ptr(), ps.data_ptr(), None) == 0
    assert Z(iptr, tptr, pa.data_ptr(), ps.data_ptr(), 0, k, u, b.ctypes.data, g.ctypes.data, z.data_ptr(), None) == 0
    assert Z(iptr, tptr, pa.data_ptr(), ps.data_ptr(), 5, k, 0, b.ctypes.data, g.ctypes.data, z.data_ptr(), None) == 0
    torch.cuda.synchronize()
    s = sentinel(n, 5)
    assert torch.equal(pa, s) and torch.equal(ps, s) and torch.equal(z, s)                    # nothing written
    null_col = (C.c_void_p * 5)(*([inputs[0].data_ptr()] * 4 + [None]))
    bad = [P(None, tptr, 5, k, u, pa.data_ptr(), ps.data_ptr(), None), P(iptr, None, 5, k, u, pa.data_ptr(), ps.data_ptr(), None),
           P(iptr, tptr, 5, k, u, None, ps.data_ptr(), None), P(iptr, tptr, 5, k, u, pa.data_ptr(), None, None),
           P(iptr, tptr, 5, k, n + 1, pa.data_ptr(), ps.data_ptr(), None), P(iptr, tptr, 5, 29, u, pa.data_ptr(), ps.data_ptr(), None),
           P(null_col, tptr, 5, k, u, pa.data_ptr(), ps.data_ptr(), None),
           Z(None, tptr, pa.data_ptr(), ps.data_ptr(), 5, k, u, b.ctypes.data, g.ctypes.data, z.data_ptr(), None),
           Z(iptr, tptr, None, ps.data_ptr(), 5, k, u, b.ctypes.data, g.ctypes.data, z.data_ptr(), None),
           Z(iptr, tptr, pa.data_ptr(), ps.data_ptr(), 5, k, u, None, g.ctypes.data, z.data_ptr(), None),
           Z(iptr, tptr, pa.data_ptr(), ps.data_ptr(), 5, k, u, b.ctypes.data, g.ctypes.data, None, None),
           Z(iptr, tptr, pa.data_ptr(), ps.data_ptr(), 5, k, n + 1, b.ctypes.data, g.ctypes.data, z.data_ptr(), None),
           Z(iptr, tptr, pa.data_ptr(), ps.data_ptr(), 5, 29, u, b.ctypes.data, g.ctypes.data, z.data_ptr(), None)]
    assert all(rc != 0 for rc in bad), bad
    torch.cuda.synchronize()
    assert torch.equal(pa, s) and torch.equal(ps, s) and torch.equal(z, s)                    # nothing enqueued
    check_case(lib, 2, "shared", "range", 6, 58, seed=1)                                      # and the library still works


# ---- streams ----------------------------------------------------------------------------------------------------------------------------------
def _reference(lib, inputs, tabs, u, k):
    n = 1 << k
    pas, pss, zs = [], [], []
    for lk, tb in zip(inputs, tabs):
        ra, rs = single_permute(lib, lk, tb, u, n)
        pas.append(ra); pss.append(rs); zs.append(composed_product(lib, lk, tb, ra, rs, k))
    return torch.stack(pas), torch.stack(pss), torch.stack(zs)


def test_inputs_from_an_unsynchronised_kernel_on_a_side_stream(lib):
    k, L, bits = 13, 8, 8
    n, u = 1 << k, (1 << k) - 6
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rows = torch.arange(n, dtype=torch.int64, device=DEV)
        table = small_ints(rows % (1 << bits), k)
        inputs = [small_ints((rows * (2 * l + 3) + l) % (1 << bits), k) for l in range(L)]      # produced on `side`, never waited for
        pa, ps = E.permute_expression_pairs_device(inputs, [table] * L, u, k, sentinel(n, L), sentinel(n, L), stream=side.cuda_stream)
        z = E.lookup_products_device(inputs, [table] * L, pa, ps, u, k, BETA, GAMMA, stream=side.cuda_stream)
    torch.cuda.synchronize()
    ra, rs, rz = _reference(lib, inputs, [table] * L, u, k)
    assert torch.equal(pa, ra) and torch.equal(ps, rs) and torch.equal(z[:, :u + 1], rz[:, :u + 1])


def test_back_to_back_calls_reuse_the_scratch(lib):
    k = 12
    n, u = 1 << k, (1 << k) - 6
    i8, t8, _, _ = build(8, "aab", "range", n, u, 8)
    i3, t3, _, _ = build(3, "distinct", "full", n, u, 3)
    torch.cuda.synchronize()
    pa8, ps8 = E.permute_expression_pairs_device(i8, t8, u, k, sentinel(n, 8), sentinel(n, 8))
    z8 = E.lookup_products_device(i8, t8, pa8, ps8, u, k, BETA, GAMMA)
    pa3, ps3 = E.permute_expression_pairs_device(i3, t3, u, k, sentinel(n, 3), sentinel(n, 3))
    z3 = E.lookup_products_device(i3, t3, pa3, ps3, u, k, BETA, GAMMA)
    for (i_, t_, pa, ps, z) in ((i8, t8, pa8, ps8, z8), (i3, t3, pa3, ps3, z3)):
        ra, rs, rz = _reference(lib, i_, t_, u, k)
        assert torch.equal(pa, ra) and torch.equal(ps, rs) and torch.equal(z[:, :u + 1], rz[:, :u + 1])


def test_calls_on_two_streams_at_once(lib):
    k = 13
    n, u = 1 << k, (1 << k) - 6
    ia, ta, _, _ = build(8, "shared", "range", n, u, 21)
    ib, tb, _, _ = build(3, "aab", "straddle", n, u, 22)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    b, g = F.fr_encode([BETA])[0], F.fr_encode([GAMMA])[0]
    outs = []
    for (i_, t_, st) in ((ia, ta, s1), (ib, tb, s2)):
        L = len(i_)
        outs.append((sentinel(n, L), sentinel(n, L), sentinel(n, L)))
    torch.cuda.synchronize()
    for rnd in range(2):                       # permute on both streams, then products on both: the second stream's call is issued while the first's products run
        for (i_, t_, st), (pa, ps, z) in zip(((ia, ta, s1), (ib, tb, s2)), outs):
            if rnd == 0:
                E.permute_expression_pairs_device(i_, t_, u, k, pa, ps, stream=st.cuda_stream)
            else:
                E.lookup_products_device(i_, t_, pa, ps, u, k, BETA, GAMMA, z=z, stream=st.cuda_stream)
    torch.cuda.synchronize()
    for (i_, t_), (pa, ps, z) in zip(((ia, ta), (ib, tb)), outs):
        ra, rs, rz = _reference(lib, i_, t_, u, k)
        assert torch.equal(pa, ra) and torch.equal(ps, rs) and torch.equal(z[:, :u + 1], rz[:, :u + 1])


# ---- proof level ------------------------------------------------------------------------------------------------------------------------------
def test_prove_flow_same_commitments_on_both_paths():
    import prove_flow

    a = prove_flow.run(13, 32, seed=9, lookups=8, verbose=False, lookups_one_call=True)
    b = prove_flow.run(13, 32, seed=9, lookups=8, verbose=False, lookups_one_call=False)
    assert all(a["checks"].values()) and all(b["checks"].values()), (a["checks"], b["checks"])
    assert a["h_commitments"] == b["h_commitments"]                       # h depends on every A', S' and z


def test_prove_flow_corrupt_gate_on_the_new_path():
    import prove_flow

    r = prove_flow.run(13, 32, seed=9, lookups=8, verbose=False, corrupt="gate", lookups_one_call=True)
    assert not r["checks"]["quotient_is_a_polynomial"] and r["checks"]["lookup_product_closes"]


@pytest.mark.parametrize("one_call", [True, False])
def test_prove_flow_corrupt_lookup_raises(one_call):
    import prove_flow

    with pytest.raises(_lib.ZkhipError):
        prove_flow.run(13, 32, seed=9, lookups=8, verbose=False, corrupt="lookup", lookups_one_call=one_call)

"""GPU (-m gpu): the chunked Fr scans of csrc/poly.hip -- the suffix Horner scan (eval_polynomial, kate_division, the batched evaluation),
the exclusive prefix product (and the grand product on top of it) and the batch inversion -- at the sizes where their 16-element chunking
adds a recursion level, and on the inputs a wrong carry, a wrong parked power b^(16^l), the line-of-four fast path, the lazy
`a + b*q < 3p` accumulation and the aliased store get wrong first.

Every expectation comes from oracle/cpu_ref (the C restatement) or from Python integers (closed forms, oracle/bn254.py); no library result
is the expectation of another.  Outputs are compared limb for limb (canonical Montgomery limbs), whole arrays, with no tolerance.  Every
device buffer is filled with 0xA5 first and the elements around an output are checked to hold that fill afterwards."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import zksnap_circuits_halo2_amd
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib

pytestmark = pytest.mark.gpu

R = O.R_MOD
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R)
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD = 8                                  # elements after every output that must keep the fill
EINVAL = -1
PY_WHOLE = 65537                           # whole arrays from Python integers up to here, the C restatement alone above
PY_PRODUCT = 4097                          # polynomial products in Python integers up to here

SCAN_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 18, 19, 20, 255, 256, 257, 259,
              4095, 4096, 4097, 65535, 65536, 65537, (1 << 20) - 1, 1 << 20, (1 << 20) + 1]
HOST_SIZES = {1, 2, 16, 17, 257, 4097, 65537, (1 << 20) + 1}
OFFSETS = (1, 2, 3)                        # elements into an allocation: 32-byte-aligned addresses that are not 128-byte aligned


# ---------------------------------------------------------------- plumbing
def enc(vals):
    """Python integers -> (n, 4) uint64 Montgomery limbs"""
    vals = list(vals)
    raw = b"".join((v % R * MONT % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(vals), 4).copy()


def dec(arr):
    """(n, 4) uint64 Montgomery limbs -> Python integers"""
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * MONT_INV % R for i in range(0, len(raw), 32)]


def one(v):
    return enc([v])[0]


class Dev:
    """`elems` 32-byte elements of device memory from zkhip_alloc, every byte 0xA5 so that an element the kernel never wrote cannot pass"""

    def __init__(self, lib, elems):
        self.lib, self.elems, self.p = lib, elems, C.c_void_p()
        _lib.check(lib.zkhip_alloc(max(elems * 32, 256), C.byref(self.p)))
        if elems:
            fill = np.full((elems, 4), FILL, dtype=np.uint64)
            _lib.check(lib.zkhip_upload(self.p, fill.ctypes.data, fill.nbytes))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.zkhip_free(self.p)

    def at(self, elem):
        assert 0 <= elem <= self.elems
        return self.p.value + 32 * elem

    def put(self, arr, elem=0):
        arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
        assert elem + arr.shape[0] <= self.elems
        if arr.nbytes:
            _lib.check(self.lib.zkhip_upload(self.at(elem), arr.ctypes.data, arr.nbytes))

    def whole(self):
        out = np.zeros((self.elems, 4), dtype=np.uint64)
        if out.nbytes:
            _lib.check(self.lib.zkhip_download(out.ctypes.data, self.p, out.nbytes))   # blocking copy on the stream the kernels ran on
        return out


def same(got, exp, what=""):
    """limb-for-limb equality of two arrays, reporting the first rows that differ (row / 16^l is the chunk at level l)"""
    got, exp = np.asarray(got).reshape(-1, 4), np.asarray(exp).reshape(-1, 4)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        pytest.fail(f"{what}: {bad.size} of {got.shape[0]} rows differ, first at {bad[:8].tolist()}")


def untouched(rows, what=""):
    assert (rows == FILL).all(), f"{what}: an element outside the output was written"


@functools.lru_cache(maxsize=None)
def _scalars(cref, seed, n):
    a = cref.gen_scalars(seed, n, 0)
    a.setflags(write=False)
    return a


def random_scalars(cref, seed, n):
    """oracle-made field elements, read-only; made once for the tests that share them (the 32 MiB ones are cheap to make and not kept)"""
    return _scalars(cref, seed, n) if n <= PY_WHOLE else cref.gen_scalars(seed, n, 0)


def random_point(cref, seed):
    return dec(cref.gen_scalars(seed, 1, 0))[0]


# ---------------------------------------------------------------- 1. the sizes
CH = 16


def chunks_of(n):
    return (n + CH - 1) // CH


def scan_levels(n):
    """stored levels of a scan over n elements (csrc/scan_plan.hpp, scan_plan::L): one more at every 16^l + 1"""
    levels = 0
    while n > CH:
        n, levels = chunks_of(n), levels + 1
    return levels


def invert_chunk(n):
    """elements per lane of the batch inversion (csrc/poly.hip fr_batch_invert_device)"""
    ch = 32
    while ch > 4 and n // ch < 65536:
        ch >>= 1
    return ch


INVERT_SIZES = [1, 63, 64, 65, 4 * 65536 - 1, 4 * 65536 + 1, 8 * 65536 + 1]


def test_chunk_length_the_sizes_are_chosen_around():
    assert [scan_levels(n) for n in SCAN_SIZES] == [0] * 7 + [1] * 6 + [2] * 4 + [3] * 3 + [4] * 3 + [5]
    for l in range(1, 6):
        assert 16 ** l in SCAN_SIZES and 16 ** l + 1 in SCAN_SIZES
        assert (scan_levels(16 ** l), scan_levels(16 ** l + 1)) == (l - 1, l)
    assert [invert_chunk(n) for n in INVERT_SIZES] == [4, 4, 4, 4, 4, 4, 8]
    # the next change of the chunk length fails here instead of moving the code's switches away from SCAN_SIZES
    src = os.path.join(os.path.dirname(zksnap_circuits_halo2_amd.__file__), "csrc", "scan_plan.hpp")
    assert "constexpr uint32_t SCAN_CH = 16;" in open(src).read()


# ---------------------------------------------------------------- 2. Horner scans
def horner_device(lib, a, b_int, off=0, stream=None):
    """(eval_polynomial, kate_division) of one upload of `a`, input and outputs `off` elements into their allocations.  The quotient has
    GUARD fill elements behind it (and `off` in front); the evaluation sits inside a buffer whose other elements keep the fill: 96 bytes
    with the result in the middle when off = 0."""
    n, m = a.shape[0], max(a.shape[0] - 1, 0)
    b = one(b_int)
    at = max(off, 1)
    with Dev(lib, off + n) as d_a, Dev(lib, off + m + GUARD) as d_q, Dev(lib, at + 2) as d_r:
        d_a.put(a, off)
        _lib.check(lib.zkhip_fr_kate_division_device(d_a.at(off), n, b.ctypes.data, d_q.at(off), stream))
        _lib.check(lib.zkhip_fr_eval_polynomial_device(d_a.at(off), n, b.ctypes.data, d_r.at(at), stream))
        q, r, back = d_q.whole(), d_r.whole(), d_a.whole()
    same(back[off:], a, "the input changed")
    untouched(q[:off], "kate_division"), untouched(q[off + m:], "kate_division")
    untouched(r[:at], "eval_polynomial"), untouched(r[at + 1:], "eval_polynomial")
    return r[at].copy(), q[off:off + m].copy()


def horner_host(lib, a, b_int):
    n, m = a.shape[0], max(a.shape[0] - 1, 0)
    a, b = np.ascontiguousarray(a), one(b_int)
    q = np.full((m + GUARD, 4), FILL, dtype=np.uint64)
    r = np.full((3, 4), FILL, dtype=np.uint64)
    _lib.check(lib.zkhip_fr_kate_division(a.ctypes.data, n, b.ctypes.data, q.ctypes.data))
    _lib.check(lib.zkhip_fr_eval_polynomial(a.ctypes.data, n, b.ctypes.data, r.ctypes.data + 32))
    untouched(q[m:], "kate_division (host)"), untouched(r[[0, 2]], "eval_polynomial (host)")
    return r[1].copy(), q[:m].copy()


def check_horner(lib, cref, a, b_int, what, scan=None, value=None, offsets=(0,), host=False):
    """both scans of `a` with the multiplier b against the C restatement, and against Python integers where the caller has them:
    `scan` = the whole suffix scan s[i] = sum_{j >= i} a[j] b^(j - i) (s[0] the evaluation, s[1:] the quotient), `value` = s[0] alone"""
    b = one(b_int)
    exp_r, exp_q = cref.eval_polynomial(a, b), cref.kate_division(a, b)
    if scan is not None:
        assert len(scan) == a.shape[0]
        value = scan[0]
        same(exp_q, enc(scan[1:]), f"{what}: the C restatement against Python integers")
    if value is not None:
        same(exp_r, one(value), f"{what}: the C restatement's evaluation against Python integers")
    runs = [(f"device, offset {off}", lambda off=off: horner_device(lib, a, b_int, off)) for off in offsets]
    if host:
        runs.append(("host", lambda: horner_host(lib, a, b_int)))
    got = None
    for name, run in runs:
        got = run()
        same(got[1], exp_q, f"{what}: kate_division, {name}")
        same(got[0], exp_r, f"{what}: eval_polynomial, {name}")
    return got


def suffix_scan(a, b):
    """s[i] = a[i] + b s[i + 1] in Python integers"""
    s, acc = [0] * len(a), 0
    for i in range(len(a) - 1, -1, -1):
        acc = (a[i] + b * acc) % R
        s[i] = acc
    return s


def horner_py(a, x):
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % R
    return acc


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_horner_random_coefficients_random_point(lib, cref, n):
    """random data through every level, at allocation offsets 0 .. 3 (the fast path keys on the index, so the address must not matter),
    through the host forms on a subset; and without the C restatement: q(t) (t - b) + a(b) = a(t) at a fresh point t"""
    a = random_scalars(cref, 0x5CA0000 + n, n)
    b = random_point(cref, 0x5CB0000 + n)
    r, q = check_horner(lib, cref, a, b, "random", offsets=(0,) + OFFSETS, host=n in HOST_SIZES)
    if n <= PY_WHOLE:
        t = random_point(cref, 0x5CC0000 + n)
        assert (horner_py(dec(q), t) * (t - b) + dec(r)[0]) % R == horner_py(dec(a), t)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_horner_multipliers_0_1_minus_1_and_2(lib, cref, n):
    """closed forms: b = 0 leaves the coefficients, b = 1 gives the suffix sums, b = r - 1 the alternating ones"""
    a = random_scalars(cref, 0x5CA0000 + n, n)
    ai = dec(a)
    whole = n <= PY_WHOLE
    # b = 0: eval is a[0], kate is a[1:]
    check_horner(lib, cref, a, 0, "b = 0", scan=ai if whole else None, value=ai[0])
    # b = 1: the sum and the suffix sums
    sums = [v % R for v in itertools.accumulate(reversed(ai))][::-1] if whole else None
    check_horner(lib, cref, a, 1, "b = 1", scan=sums, value=sum(ai) % R)
    # b = r - 1: s[i] = a[i] - a[i + 1] + a[i + 2] - ...
    alt, acc = [0] * n, 0
    for i in range(n - 1, -1, -1):
        acc = (ai[i] - acc) % R
        alt[i] = acc
    assert alt[0] == (sum(ai[0::2]) - sum(ai[1::2])) % R
    check_horner(lib, cref, a, R - 1, "b = r - 1", scan=alt if whole else None, value=alt[0])
    check_horner(lib, cref, a, 2, "b = 2", scan=suffix_scan(ai, 2) if whole else None)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_horner_every_coefficient_r_minus_1(lib, cref, n):
    """the largest canonical value in every position: the largest the lazy accumulation and the canonical store see, through every level"""
    a = np.tile(one(R - 1), (n, 1))
    # b = r - 1: s[i] = -(1 - 1 + 1 - ...) over n - i terms: r - 1 when that count is odd, 0 when it is even
    scan = [(R - 1) if (n - i) & 1 else 0 for i in range(n)]
    check_horner(lib, cref, a, R - 1, "all r - 1, b = r - 1", scan=scan)
    b = random_point(cref, 0x5CD0000 + n)
    # s[i] = -(1 + b + ... + b^(n - 1 - i)) = -(b^(n - i) - 1) / (b - 1)
    value = -(pow(b, n, R) - 1) * pow(b - 1, -1, R) % R
    check_horner(lib, cref, a, b, "all r - 1, b random", scan=suffix_scan([R - 1] * n, b) if n <= PY_WHOLE else None, value=value)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_horner_only_the_top_coefficient(lib, cref, n):
    """a = X^(n - 1): eval = b^(n - 1) goes through every parked power b^(16^l) and nothing else; kate = [b^(n - 2), ..., b, 1]"""
    a = np.zeros((n, 4), dtype=np.uint64)
    a[n - 1] = one(1)
    b = random_point(cref, 0x5CE0000 + n)
    scan = None
    if n <= PY_WHOLE:
        scan = list(itertools.accumulate(range(n - 1), lambda p, _: p * b % R, initial=1))[::-1]
        assert scan[0] == pow(b, n - 1, R)
    r, q = check_horner(lib, cref, a, b, "top coefficient 1", scan=scan, value=pow(b, n - 1, R))
    for i in sorted({0, 14, 15, 16, 255, 256, n - 2} & set(range(n - 1))):
        assert dec(q[i])[0] == pow(b, n - 2 - i, R), i
    check_horner(lib, cref, a, 2, "top coefficient 1, b = 2", value=pow(2, n - 1, R))


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_horner_at_a_root(lib, cref, n):
    """a = (X - b) g: the evaluation is zero and the division gives g back exactly"""
    b = random_point(cref, 0x5CF0000 + n)
    g = random_scalars(cref, 0x5D00000 + n, n - 1)
    if n <= PY_PRODUCT:
        gi = dec(g)
        a = enc([((gi[i - 1] if i else 0) - (b * gi[i] if i < n - 1 else 0)) % R for i in range(n)])
    else:   # the same product with the oracle's field operations: a = X g - b g
        bg = cref.field_op(1, 0, np.tile(one(b), (n - 1, 1)), np.ascontiguousarray(g))
        zero = np.zeros((1, 4), dtype=np.uint64)
        a = cref.field_op(1, 2, np.vstack([zero, g]), np.vstack([bg, zero]))
    r, q = check_horner(lib, cref, a, b, "b is a root", value=0, host=n in HOST_SIZES)
    assert not r.any()
    same(q, g, "b is a root: the quotient is g")


# ---------------------------------------------------------------- 3. batched evaluation
def eval_batch(lib, polys, x_int, count=None, shared=False):
    """the polynomials carved out of one allocation at odd element offsets (one fill element at least between two of them); `shared`:
    `count` pointers to the one polynomial given.  Returns the `count` results; GUARD fill elements behind them are checked."""
    n = polys[0].shape[0]
    count = len(polys) if count is None else count
    stride = (n + 2) & ~1                                     # even and > n: every offset 1 + i * stride is odd
    x = one(x_int)
    with Dev(lib, 1 + len(polys) * stride) as d_in, Dev(lib, count + GUARD) as d_out:
        for i, p in enumerate(polys):
            d_in.put(p, 1 + i * stride)
        addrs = [d_in.at(1)] * count if shared else [d_in.at(1 + i * stride) for i in range(count)]
        ptrs = (C.c_void_p * count)(*addrs)
        _lib.check(lib.zkhip_fr_eval_polynomial_batch_device(ptrs, count, n, x.ctypes.data, d_out.p, None))
        out = d_out.whole()
    untouched(out[count:], "eval_polynomial_batch")
    return out[:count]


@pytest.mark.parametrize("count", [1, 3, 40])
@pytest.mark.parametrize("n", [16, 17, 256, 257, 4096, 4097, 65537])
def test_eval_batch_counts_against_the_oracle(lib, cref, n, count):
    polys = [cref.gen_scalars(0xBA7C0000 + 64 * n + i, n, i % 2) for i in range(count)]
    x = random_point(cref, 0xBA7D0000 + n)
    got = eval_batch(lib, polys, x)
    same(got, np.array([cref.eval_polynomial(p, one(x)) for p in polys]), "batched evaluation")
    if n <= PY_PRODUCT:
        assert dec(got[0])[0] == O.eval_polynomial(dec(polys[0]), x)


def test_eval_batch_largest_count_and_one_more(lib, cref):
    """65535 polynomials is the grid's limit: all of them (pointers to one shared polynomial) come out right; 65536 is refused with nothing
    written, and a correct call succeeds afterwards"""
    n = 17
    poly = random_scalars(cref, 0xBA7E0000, n)
    x = random_point(cref, 0xBA7E0001)
    value = one(O.eval_polynomial(dec(poly), x))
    same(value, cref.eval_polynomial(poly, one(x)))
    same(eval_batch(lib, [poly], x, count=65535, shared=True), np.tile(value, (65535, 1)), "65535 polynomials")
    count = 65536
    with Dev(lib, 1 + n) as d_in, Dev(lib, count + GUARD) as d_out:
        d_in.put(poly, 1)
        ptrs = (C.c_void_p * count)(*[d_in.at(1)] * count)
        assert lib.zkhip_fr_eval_polynomial_batch_device(ptrs, count, n, one(x).ctypes.data, d_out.p, None) == EINVAL
        untouched(d_out.whole(), "a refused call")
    same(eval_batch(lib, [poly], x, count=3, shared=True), np.tile(value, (3, 1)), "after the refused call")


@pytest.mark.parametrize("n", [257, 4097])
def test_eval_batch_edge_values(lib, cref, n):
    top = np.zeros((n, 4), dtype=np.uint64)
    top[n - 1] = one(1)
    largest = np.tile(one(R - 1), (n, 1))
    for b in (random_point(cref, 0xBA7F0000 + n), R - 1, 1, 0):
        v_top = pow(b, n - 1, R)
        v_largest = -sum(pow(b, i, R) for i in range(n)) % R
        same(eval_batch(lib, [top, largest, top], b), enc([v_top, v_largest, v_top]), f"b = {b:#x}")
        same(eval_batch(lib, [largest, top, largest], b), enc([v_largest, v_top, v_largest]), f"b = {b:#x}")


# ---------------------------------------------------------------- 4. prefix product and grand product
def prefix_device(lib, v, off=0, alias=False, zero_at=None):
    """out aliases v when `alias`; `zero_at`: that element of v is zeroed on the device after the upload"""
    n = v.shape[0]
    with Dev(lib, off + n + GUARD) as d_v, Dev(lib, off + n + GUARD) as d_out:
        d_v.put(v, off)
        if zero_at is not None:
            d_v.put(np.zeros((1, 4), dtype=np.uint64), off + zero_at)
        dst = d_v if alias else d_out
        _lib.check(lib.zkhip_fr_prefix_product_device(d_v.at(off), n, dst.at(off), None))
        w_v, w_out = d_v.whole(), d_out.whole()
    got = (w_v if alias else w_out)[off:off + n]
    if alias:
        untouched(w_out, "prefix_product (aliased)")
    else:
        untouched(w_out[:off], "prefix_product"), untouched(w_out[off + n:], "prefix_product")
        if zero_at is None:
            same(w_v[off:off + n], v, "the input changed")
    untouched(w_v[:off], "prefix_product"), untouched(w_v[off + n:], "prefix_product")
    return got.copy()


def prefix_host(lib, v):
    v = np.ascontiguousarray(v)
    n = v.shape[0]
    out = np.full((n + GUARD, 4), FILL, dtype=np.uint64)
    _lib.check(lib.zkhip_fr_prefix_product(v.ctypes.data, n, out.ctypes.data))
    untouched(out[n:], "prefix_product (host)")
    return out[:n].copy()


def check_prefix(lib, v, exp, what, offsets=(0,), host=False):
    for off in offsets:
        same(prefix_device(lib, v, off), exp, f"{what}: device, offset {off}")
    same(prefix_device(lib, v, alias=True), exp, f"{what}: device, out = v")
    if host:
        same(prefix_host(lib, v), exp, f"{what}: host")


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_prefix_product_random(lib, cref, n):
    v = random_scalars(cref, 0x9F0D0000 + n, n)
    exp = cref.prefix_product(np.ascontiguousarray(v))
    if n <= PY_PRODUCT:
        same(exp, enc(O.prefix_product(dec(v))), "the C restatement against Python integers")
    check_prefix(lib, v, exp, "random", offsets=(0,) + OFFSETS, host=True)
    same(prefix_device(lib, v, off=3, alias=True), exp, "random: device, out = v, offset 3")


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_prefix_product_all_2_and_all_r_minus_1(lib, cref, n):
    twos = np.tile(one(2), (n, 1))
    exp = cref.prefix_product(twos)
    if n <= PY_WHOLE:
        same(exp, enc(itertools.accumulate(range(n - 1), lambda p, _: p * 2 % R, initial=1)), "the C restatement against 2^i")
    for i in sorted({0, 15, 16, 17, 255, 256, 257, 4096, 65536, n - 1} & set(range(n))):
        assert dec(exp[i])[0] == pow(2, i, R), i
    check_prefix(lib, twos, exp, "all 2", host=n in HOST_SIZES)
    exp = np.tile(enc([1, R - 1]), ((n + 1) // 2, 1))[:n]          # 1, -1, 1, -1, ...
    check_prefix(lib, np.tile(one(R - 1), (n, 1)), exp, "all r - 1")


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_prefix_product_one_zero(lib, cref, n):
    """a zero first or last in a chunk of level 0 (15, 16) and of level 1 (255, 256), in the last element that is ever read (n - 2) and in
    the one that is never multiplied in (n - 1): everything up to it is as without the zero, everything after it is zero"""
    v = random_scalars(cref, 0x9F0D0000 + n, n)
    assert v.any(axis=1).all()
    base = cref.prefix_product(np.ascontiguousarray(v))
    for p in sorted({0, 15, 16, 17, 255, 256, n - 2, n - 1} & set(range(n))):
        exp = base.copy()
        exp[p + 1:] = 0
        same(prefix_device(lib, v, zero_at=p), exp, f"zero at {p}")
        same(prefix_device(lib, v, zero_at=p, alias=True), exp, f"zero at {p}, out = v")


def grand_product_device(lib, num, den, alias):
    n = num.shape[0]
    with Dev(lib, n + GUARD) as d_num, Dev(lib, n + GUARD) as d_den, Dev(lib, n + GUARD) as d_z:
        d_num.put(num), d_den.put(den)
        _lib.check(lib.zkhip_fr_grand_product_device(d_num.p, d_den.p, n, (d_num if alias else d_z).p, None))
        w_num, w_den, w_z = d_num.whole(), d_den.whole(), d_z.whole()
    untouched(w_num[n:], "grand_product: num"), untouched(w_den[n:], "grand_product: den")
    if alias:
        untouched(w_z, "grand_product (z = num)")
        return w_num[:n].copy()
    untouched(w_z[n:], "grand_product: z")
    same(w_num[:n], num, "grand_product: num changed")
    return w_z[:n].copy()


def grand_product_host(lib, num, den):
    n = num.shape[0]
    num_in, den_in = num.copy(), den.copy()
    z = np.full((n + GUARD, 4), FILL, dtype=np.uint64)
    _lib.check(lib.zkhip_fr_grand_product(num_in.ctypes.data, den_in.ctypes.data, n, z.ctypes.data))
    untouched(z[n:], "grand_product (host)")
    same(num_in, num, "grand_product (host): num changed"), same(den_in, den, "grand_product (host): den changed")
    return z[:n].copy()


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_grand_product(lib, cref, n):
    """z[i + 1] = z[i] num[i] / den[i] against batch_invert -> mul -> prefix_product of the C restatement, without a zero denominator and
    with one on a chunk edge (it counts as zero, so every later z is zero)"""
    num = np.array(random_scalars(cref, 0x6A0D0000 + n, n))
    for zero_at in [None] + [p for p in (15, 16, 256) if p < n]:
        den = np.array(random_scalars(cref, 0x6A0E0000 + n, n))
        if zero_at is not None:
            den[zero_at] = 0
        inv = den.copy()
        cref.batch_invert(inv)
        exp = cref.prefix_product(cref.field_op(1, 0, num, inv))
        if zero_at is not None and zero_at + 1 < n:
            assert exp[zero_at].any() and not exp[zero_at + 1:].any()
        if n <= 1000:
            same(exp, enc(O.grand_product(dec(num), dec(den))), "the C restatement against Python integers")
        same(grand_product_device(lib, num, den, alias=False), exp, f"zero at {zero_at}: device")
        same(grand_product_device(lib, num, den, alias=True), exp, f"zero at {zero_at}: device, z = num")
        same(grand_product_host(lib, num, den), exp, f"zero at {zero_at}: host")


# ---------------------------------------------------------------- 5. batch inversion, device form
def invert_device(lib, a, off=3):
    n = a.shape[0]
    with Dev(lib, off + n + GUARD) as d:
        d.put(a, off)
        _lib.check(lib.zkhip_fr_batch_invert_device(d.at(off), n, None))
        w = d.whole()
    untouched(w[:off], "batch_invert"), untouched(w[off + n:], "batch_invert")
    return w[off:off + n].copy()


@pytest.mark.parametrize("n", INVERT_SIZES)
def test_batch_invert_device(lib, cref, n):
    """in place, 3 elements into its allocation with fill on both sides; zeros (they stay zero and leave their lane's other inverses alone)
    in the first and last lane of a tile, in a lane's second element and at the end; and an all-zero array"""
    a = np.array(random_scalars(cref, 0x1B7E0000 + n, n))
    tile = 64 * invert_chunk(n)
    zeros = sorted({0, 63, 64, tile, tile + 63, tile + 64, n - 1} & set(range(n)))
    a[zeros] = 0
    for i, v in ((1, 1), (2, R - 1), (65, 2)):
        if i < n and i not in zeros:
            a[i] = one(v)
    exp = a.copy()
    cref.batch_invert(exp)
    assert not exp[zeros].any()
    got = invert_device(lib, a)
    same(got, exp, "batch_invert")
    sample = sorted(({1, 2, 3, 62, 65, 66, 127, 128, n - 2} & set(range(n))) - set(zeros))
    for x, y in zip(dec(a[sample]), dec(got[sample])):
        assert x * y % R == 1
    nothing = np.zeros((n, 4), dtype=np.uint64)
    same(invert_device(lib, nothing), nothing, "all zero")


# ---------------------------------------------------------------- 6. queued calls on one stream
def test_queued_calls_on_a_side_stream_keep_their_multipliers(lib, cref):
    """four calls back to back on a non-default stream with no host wait between them, each with another multiplier, the last one growing
    the stream's scratch: a parked multiplier is not overwritten under a queued call and the growth does not disturb earlier work"""
    import torch

    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    n1, n2, n3, n4 = 4097, 17, 65537, (1 << 20) + 1
    a1, a2, a3, a4 = (random_scalars(cref, 0x57AE0000 + n, n) for n in (n1, n2, n3, n4))
    b1, b2, b4 = (random_point(cref, 0x57AF0000 + i) for i in range(3))
    assert len({b1, b2, b4}) == 3
    e1, e2, e4 = one(b1), one(b2), one(b4)
    with Dev(lib, n1) as d_a1, Dev(lib, n1 - 1 + GUARD) as d_q1, Dev(lib, n2) as d_a2, Dev(lib, 3) as d_r2, Dev(lib, n3) as d_a3, \
            Dev(lib, n3 + GUARD) as d_p3, Dev(lib, n4) as d_a4, Dev(lib, n4 - 1 + GUARD) as d_q4:
        d_a1.put(a1), d_a2.put(a2), d_a3.put(a3), d_a4.put(a4)
        _lib.check(lib.zkhip_sync())                      # the uploads and fills are done before the side stream starts
        _lib.check(lib.zkhip_fr_kate_division_device(d_a1.p, n1, e1.ctypes.data, d_q1.p, s))
        _lib.check(lib.zkhip_fr_eval_polynomial_device(d_a2.p, n2, e2.ctypes.data, d_r2.at(1), s))
        _lib.check(lib.zkhip_fr_prefix_product_device(d_a3.p, n3, d_p3.p, s))
        _lib.check(lib.zkhip_fr_kate_division_device(d_a4.p, n4, e4.ctypes.data, d_q4.p, s))
        _lib.check(lib.zkhip_stream_sync(s))
        q1, r2, p3, q4 = d_q1.whole(), d_r2.whole(), d_p3.whole(), d_q4.whole()
    same(q1[:n1 - 1], cref.kate_division(a1, e1), "first call: kate_division"), untouched(q1[n1 - 1:])
    same(r2[1], cref.eval_polynomial(a2, e2), "second call: eval_polynomial"), untouched(r2[[0, 2]])
    same(p3[:n3], cref.prefix_product(np.ascontiguousarray(a3)), "third call: prefix_product"), untouched(p3[n3:])
    same(q4[:n4 - 1], cref.kate_division(a4, e4), "fourth call: kate_division"), untouched(q4[n4 - 1:])

"""GPU (-m gpu): `zkhip_fr_divide_by_roots(_device)` -- the quotient of a polynomial by the vanishing polynomial of 1 .. 8 points in one
pass -- gives the bytes of the fold of `kate_division`s it replaces.

The arithmetic is exact and every output canonical, so every comparison is on whole arrays, byte for byte:
  1. against the fold of `zkhip_fr_kate_division_device` (both orders), the zero tail, the evaluations against `zkhip_fr_eval_polynomial_device`;
  2. against the oracle (`oracle.cpu_ref.kate_division` folded; Python integers: a = q Z + interpolant(evals));
  3. roots as the prover has them, and awkward roots;  4. rejections;  5. stream order;  6. the host form;  7. the wrapper size.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F

pytestmark = pytest.mark.gpu

MAX_ROOTS = 8
EINVAL = -1
POISON = 0x5A5A5A5A5A5A5A5A


def _random_fr_device(torch, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    a = torch.randint(-(1 << 63), (1 << 63) - 1, (max(n, 1), 4), dtype=torch.int64, device="cuda", generator=g)[:n]
    if n:
        a[:, 3] = torch.randint(0, 1 << 61, (n,), dtype=torch.int64, device="cuda", generator=g)   # < r: canonical Montgomery words
    return a.contiguous()


def _roots(m, seed):
    """m distinct canonical field elements (Montgomery words, [m][4] uint64)"""
    rng = np.random.default_rng(seed)
    vals = set()
    while len(vals) < m:
        vals.add(int.from_bytes(rng.bytes(40), "little") % O.R_MOD)
    return F.fr_encode(sorted(vals, key=lambda v: (v * 0x9E3779B97F4A7C15) % O.R_MOD))


def _patterns(torch, n, seed):
    yield "random", _random_fr_device(torch, n, seed)
    yield "zero", torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    top = torch.from_numpy(F.fr_encode([O.R_MOD - 1]).view(np.int64)).cuda()
    yield "all r-1", top.repeat(n, 1).contiguous()
    one_top = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    if n:
        one_top[n - 1] = torch.from_numpy(F.fr_encode([1]).view(np.int64)).cuda()[0]
    yield "one at the top", one_top


def _fold(lib, torch, a, roots, stream=None):
    """m successive `zkhip_fr_kate_division_device` calls in the order of `roots`: the n - m quotient coefficients (none when n <= m)"""
    cur, n = a, a.shape[0]
    for z in roots:
        if n < 2:
            return torch.zeros((0, 4), dtype=torch.int64, device="cuda")
        z = np.ascontiguousarray(z)
        nxt = torch.full((n - 1, 4), POISON, dtype=torch.int64, device="cuda")
        _lib.check(lib.zkhip_fr_kate_division_device(cur.data_ptr(), n, z.ctypes.data, nxt.data_ptr(), stream))
        _lib.check(lib.zkhip_stream_sync(stream))
        cur, n = nxt, n - 1
    return cur


def _divide(lib, torch, a, roots, want_evals=True, stream=None):
    n, m = a.shape[0], roots.shape[0]
    q = torch.full((n, 4), POISON, dtype=torch.int64, device="cuda")
    ev = torch.full((m, 4), POISON, dtype=torch.int64, device="cuda")
    roots = np.ascontiguousarray(roots)
    _lib.check(lib.zkhip_fr_divide_by_roots_device(a.data_ptr() if n else None, n, roots.ctypes.data, m, q.data_ptr() if n else None,
                                                   ev.data_ptr() if want_evals else None, stream))
    _lib.check(lib.zkhip_stream_sync(stream))
    return q, ev


def _evals(lib, torch, a, roots):
    out = torch.full((roots.shape[0], 4), POISON, dtype=torch.int64, device="cuda")
    for i, z in enumerate(roots):
        z = np.ascontiguousarray(z)
        _lib.check(lib.zkhip_fr_eval_polynomial_device(a.data_ptr() if a.shape[0] else None, a.shape[0], z.ctypes.data, out[i].data_ptr(), None))
    _lib.check(lib.zkhip_stream_sync(None))
    return out


def _check_against_fold(lib, torch, a, roots, tag):
    n, m = a.shape[0], roots.shape[0]
    keep = a.clone()
    q, ev = _divide(lib, torch, a, roots)
    assert torch.equal(a, keep), (tag, "the input was modified")
    fwd = _fold(lib, torch, a, roots)
    rev = _fold(lib, torch, a, roots[::-1])
    assert torch.equal(fwd, rev), (tag, "the fold itself depends on the order")
    head = max(n - m, 0)
    assert fwd.shape[0] == head
    assert torch.equal(q[:head], fwd), (tag, "quotient")
    assert not bool(q[head:].any()), (tag, "zero tail")
    assert torch.equal(ev, _evals(lib, torch, a, roots)), (tag, "evaluations")
    q2, ev2 = _divide(lib, torch, a, roots, want_evals=False)      # without evaluations: the same quotient, the evaluation buffer untouched
    assert torch.equal(q2, q), (tag, "quotient without evaluations")
    assert bool((ev2 == POISON).all()), (tag, "evaluations written though not asked for")


def _sizes(m):
    # around every size at which poly.hip's recursion gains a level (16^j), the issue's list, and the sizes around m
    base = [0, 1, 2, m - 1, m, m + 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, (1 << 16) + 3, (1 << 20) - 1, 1 << 20,
            (1 << 20) + 1]
    return sorted({s for s in base if s >= 0})


@pytest.mark.parametrize("m", list(range(1, MAX_ROOTS + 1)))
def test_equals_the_fold_of_kate_divisions(lib, m):
    import torch

    roots = _roots(m, 100 + m)
    for n in _sizes(m):
        for name, a in _patterns(torch, n, 1000 * m + n % 997):
            _check_against_fold(lib, torch, a, roots, (m, n, name))


def _interpolate(points, evals):
    m = len(points)
    coeffs = [0] * m
    for i in range(m):
        num, den = [1], 1
        for j in range(m):
            if j != i:
                num = [(x - points[j] * y) % O.R_MOD for x, y in zip([0] + num, num + [0])]
                den = den * (points[i] - points[j]) % O.R_MOD
        scale = evals[i] * pow(den, -1, O.R_MOD) % O.R_MOD
        for t in range(m):
            coeffs[t] = (coeffs[t] + scale * num[t]) % O.R_MOD
    return coeffs


@pytest.mark.parametrize("m", list(range(1, MAX_ROOTS + 1)))
def test_equals_the_oracle(lib, cref, m):
    """independent of every HIP path: the oracle's `kate_division` folded (n <= 2^12); Python integers for n <= 64"""
    import torch

    roots = _roots(m, 200 + m)
    points = F.fr_decode(roots)
    for n in [1, 2, m, m + 1, 2 * m + 1, 16, 17, 33, 63, 64, 255, 256, 257, 1000, 4095, 4096]:
        host = cref.gen_scalars(7000 + 13 * m + n, n, 0)
        a = torch.from_numpy(host.view(np.int64)).cuda()
        q, ev = _divide(lib, torch, a, roots)
        got = q.cpu().numpy().view(np.uint64)
        cur = host
        for z in roots:
            cur = cref.kate_division(np.ascontiguousarray(cur), np.ascontiguousarray(z)) if cur.shape[0] > 1 else np.zeros((0, 4), dtype=np.uint64)
        exp = np.zeros((n, 4), dtype=np.uint64)
        exp[:cur.shape[0]] = cur
        assert np.array_equal(got, exp), (m, n)
        if n <= 64:
            ai, qi, ei = F.fr_decode(host), F.fr_decode(got), F.fr_decode(ev.cpu().numpy().view(np.uint64))
            z_poly = [1]
            for p in points:
                z_poly = [(x - p * y) % O.R_MOD for x, y in zip([0] + z_poly, z_poly + [0])]
            prod = [0] * (n + m + 1)
            for i, x in enumerate(qi):
                for j, y in enumerate(z_poly):
                    prod[i + j] = (prod[i + j] + x * y) % O.R_MOD
            for t, c in enumerate(_interpolate(points, ei)):
                prod[t] = (prod[t] + c) % O.R_MOD
            assert prod[:n] == ai and not any(prod[n:]), (m, n, "a != q Z + interpolant(evals)")


def test_roots_as_the_prover_has_them(lib):
    import torch

    k, blinding = 10, 5
    n = 1 << k
    w = O.omega_for(k)
    x = 0x1234567890ABCDEF1122334455667788AABBCCDDEEFF00112233445566778899 % O.R_MOD
    sets = [
        F.fr_encode([x, w * x % O.R_MOD, pow(w, -1, O.R_MOD) * x % O.R_MOD, pow(w, -(blinding + 1), O.R_MOD) * x % O.R_MOD]),
        F.fr_encode([x, w * x % O.R_MOD]),
        F.fr_encode([0, 1, O.R_MOD - 1]),
        F.fr_encode([0]),
        F.fr_encode([1, 0]),
    ]
    top = np.zeros((3, 4), dtype=np.uint64)                      # Montgomery words that differ in the top limb only
    top[:, 0], top[:, 1], top[:, 2] = 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, 0xFFFFFFFF00000000
    top[:, 3] = [0, 1, 0x30644E72E131A028]
    sets.append(top)
    for s, roots in enumerate(sets):
        for size in (n, n + 1, 17):
            for name, a in _patterns(torch, size, 31 * s + size):
                _check_against_fold(lib, torch, a, roots, (s, size, name))


def test_rejections_enqueue_nothing(lib):
    import torch

    n = 1000
    a = _random_fr_device(torch, n, 5)
    good = _roots(3, 9)
    r_words = np.array([[(O.R_MOD >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]], dtype=np.uint64)
    ones = np.full((1, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    cases = {
        "m = 0": (a.data_ptr(), good, 0, True),
        "m = 9": (a.data_ptr(), _roots(9, 3), 9, True),
        "null roots": (a.data_ptr(), None, 3, True),
        "null a": (None, good, 3, True),
        "null q": (a.data_ptr(), good, 3, False),
        "root = r": (a.data_ptr(), np.concatenate([good[:2], r_words]), 3, True),
        "root = 2^256 - 1": (a.data_ptr(), np.concatenate([ones, good[:2]]), 3, True),
        "equal roots": (a.data_ptr(), np.concatenate([good[:2], good[:1]]), 3, True),
        "equal roots, m = 2": (a.data_ptr(), np.concatenate([good[:1], good[:1]]), 2, True),
    }
    for name, (pa, roots, m, with_q) in cases.items():
        q = torch.full((n, 4), POISON, dtype=torch.int64, device="cuda")
        ev = torch.full((MAX_ROOTS + 1, 4), POISON, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        roots = None if roots is None else np.ascontiguousarray(roots)
        rc = lib.zkhip_fr_divide_by_roots_device(pa, n, None if roots is None else roots.ctypes.data, m, q.data_ptr() if with_q else None, ev.data_ptr(), None)
        assert rc == EINVAL, (name, rc)
        assert lib.zkhip_last_error(), name
        _lib.check(lib.zkhip_stream_sync(None))
        assert bool((q == POISON).all()) and bool((ev == POISON).all()), (name, "something was written")
        # the host form rejects the same
        hq = np.full((n, 4), POISON, dtype=np.uint64)
        hev = np.full((MAX_ROOTS + 1, 4), POISON, dtype=np.uint64)
        ha = np.ascontiguousarray(a.cpu().numpy().view(np.uint64))
        rc = lib.zkhip_fr_divide_by_roots(ha.ctypes.data if pa else None, n, None if roots is None else roots.ctypes.data, m, hq.ctypes.data if with_q else None,
                                          hev.ctypes.data)
        assert rc == EINVAL, (name, "host form", rc)
        assert (hq == POISON).all() and (hev == POISON).all(), (name, "host form wrote something")
    # n = 0 is fine: nothing to divide, the evaluations are zeros
    ev = torch.full((3, 4), POISON, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_fr_divide_by_roots_device(None, 0, good.ctypes.data, 3, None, ev.data_ptr(), None))
    _lib.check(lib.zkhip_stream_sync(None))
    assert not bool(ev.any())
    hev = np.full((3, 4), POISON, dtype=np.uint64)
    _lib.check(lib.zkhip_fr_divide_by_roots(None, 0, good.ctypes.data, 3, None, hev.ctypes.data))
    assert not hev.any()


def test_stream_order(lib):
    """the input comes from an unsynchronised `zkhip_ifft_scaled_device` on a side stream and is divided on that stream with no host
    synchronisation in between; two calls with different m back to back on one stream; two streams at once"""
    import torch

    k = 16
    n = 1 << k
    om_inv = F.fr_encode([pow(O.omega_for(k), -1, O.R_MOD)])[0]
    div = F.fr_encode([pow(n, -1, O.R_MOD)])[0]
    r4, r2 = _roots(4, 41), _roots(2, 42)
    src = _random_fr_device(torch, n, 77)
    # expected, everything synchronised
    coeffs = src.clone()
    _lib.check(lib.zkhip_ifft_scaled_device(coeffs.data_ptr(), om_inv.ctypes.data, k, div.ctypes.data, None))
    _lib.check(lib.zkhip_stream_sync(None))
    exp4, exp4_ev = _divide(lib, torch, coeffs, r4)
    exp2, exp2_ev = _divide(lib, torch, coeffs, r2)
    assert torch.equal(exp4[:n - 4], _fold(lib, torch, coeffs, r4)) and torch.equal(exp2[:n - 2], _fold(lib, torch, coeffs, r2))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    h1, h2 = C.c_void_p(s1.cuda_stream), C.c_void_p(s2.cuda_stream)
    b1, b2 = src.clone(), src.clone()
    q4 = torch.full((n, 4), POISON, dtype=torch.int64, device="cuda")
    q2 = torch.full((n, 4), POISON, dtype=torch.int64, device="cuda")
    q4b = torch.full((n, 4), POISON, dtype=torch.int64, device="cuda")
    e4 = torch.full((4, 4), POISON, dtype=torch.int64, device="cuda")
    e2 = torch.full((2, 4), POISON, dtype=torch.int64, device="cuda")
    e4b = torch.full((4, 4), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.zkhip_ifft_scaled_device(b1.data_ptr(), om_inv.ctypes.data, k, div.ctypes.data, h1))
    _lib.check(lib.zkhip_fr_divide_by_roots_device(b1.data_ptr(), n, r4.ctypes.data, 4, q4.data_ptr(), e4.data_ptr(), h1))
    _lib.check(lib.zkhip_fr_divide_by_roots_device(b1.data_ptr(), n, r2.ctypes.data, 2, q2.data_ptr(), e2.data_ptr(), h1))     # back to back, another m
    _lib.check(lib.zkhip_ifft_scaled_device(b2.data_ptr(), om_inv.ctypes.data, k, div.ctypes.data, h2))                        # a second stream at once
    _lib.check(lib.zkhip_fr_divide_by_roots_device(b2.data_ptr(), n, r4.ctypes.data, 4, q4b.data_ptr(), e4b.data_ptr(), h2))
    _lib.check(lib.zkhip_stream_sync(h1))
    _lib.check(lib.zkhip_stream_sync(h2))
    assert torch.equal(q4, exp4) and torch.equal(e4, exp4_ev)
    assert torch.equal(q2, exp2) and torch.equal(e2, exp2_ev)
    assert torch.equal(q4b, exp4) and torch.equal(e4b, exp4_ev)


@pytest.mark.parametrize("m", [1, 2, 3, 5, 8])
def test_host_form_equals_device_form(lib, m):
    import torch

    roots = _roots(m, 300 + m)
    for n in [1, m, m + 1, 16, 17, 4097, 1 << 16]:
        a = _random_fr_device(torch, n, 50 + n % 91)
        q, ev = _divide(lib, torch, a, roots)
        host = np.ascontiguousarray(a.cpu().numpy().view(np.uint64))
        hq = np.full((n, 4), POISON, dtype=np.uint64)
        hev = np.full((m, 4), POISON, dtype=np.uint64)
        _lib.check(lib.zkhip_fr_divide_by_roots(host.ctypes.data, n, roots.ctypes.data, m, hq.ctypes.data, hev.ctypes.data))
        assert np.array_equal(hq, q.cpu().numpy().view(np.uint64)) and np.array_equal(hev, ev.cpu().numpy().view(np.uint64)), (m, n)
        hq2 = np.full((n, 4), POISON, dtype=np.uint64)
        _lib.check(lib.zkhip_fr_divide_by_roots(host.ctypes.data, n, roots.ctypes.data, m, hq2.ctypes.data, None))
        assert np.array_equal(hq2, hq), (m, n, "without evaluations")


def test_wrapper_size_against_the_fold(lib):
    """n = 2^22 (the wrapper circuit's polynomials), a rotation set of three points"""
    import torch

    a = _random_fr_device(torch, 1 << 22, 2203)
    _check_against_fold(lib, torch, a, _roots(3, 2204), "2^22, m = 3")

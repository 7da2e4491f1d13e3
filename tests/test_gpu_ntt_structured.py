"""The Fr transforms on structured inputs (tests/ntt_cases.py): outputs that are exact zeros, inputs at the top of their range, zero-padding
ratios on both sides of the first pass's N/4 shortcut, output cuts on both store paths of the last pass, and zkhip_mul_periodic past its grid cap.
Every comparison is limb for limb: an output is right only if it is the canonical word."""
import numpy as np
import pytest

import ntt_cases as NC
from zksnap_circuits_halo2_amd import _lib

pytestmark = pytest.mark.gpu

R = NC.R
SENT = np.uint64(0xDEADBEEFDEADBEEF)
ZETA = NC.word(NC.enc(NC.O.FR_ZETA))
ZETA2 = NC.word(NC.enc(NC.O.FR_ZETA * NC.O.FR_ZETA))
EINVAL = -1


def _root(L):
    w = NC.omega(L)
    return NC.word(NC.enc(w)), NC.word(NC.enc(pow(w, -1, R)))


def _dev(host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host).view(np.int64)).cuda()


def _host(d, shape):
    import torch

    torch.cuda.synchronize()
    return d.cpu().numpy().view(np.uint64).reshape(shape)


def _failures(results):
    return [r for r in results if r]


# ---- forward transform and scaled inverse --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", list(NC.SIZES))
def test_forward_batch_then_scaled_inverse(lib, cref, L):
    """every family x constant of one size as one strided batch: the forward results are the closed forms and best_fft's, the sentinel between the
    polynomials survives, and the scaled inverse of those results (N - 1 exact zeros behind the out_scale multiply) returns the inputs as words"""
    cs = NC.cases(L)
    V, N = len(cs), 1 << L
    stride = N + 3
    om, om_inv = _root(L)
    div = NC.word(NC.enc(pow(N, -1, R)))
    host = np.full((V, stride, 4), SENT, dtype=np.uint64)

    def fill(v):
        host[v, :N] = NC.vector(L, cs[v])[0]

    NC.for_each(fill, V, L)
    d = _dev(host)
    _lib.check(lib.zkhip_ntt_fr_batch_device(d.data_ptr(), om.ctypes.data, L, V, stride, None))
    got = _host(d, (V, stride, 4))
    assert (got[:, N:] == SENT).all()

    def mismatch(v):
        a, e = NC.vector(L, cs[v])
        if not np.array_equal(got[v, :N], e):
            return NC.case_id(cs[v]) + ": closed form, first at %d" % int(np.argmax((got[v, :N] != e).any(axis=1)))
        cref.best_fft(a, om, L, 1)
        return None if np.array_equal(got[v, :N], a) else NC.case_id(cs[v]) + ": best_fft"

    assert _failures(NC.for_each(mismatch, V, L)) == []
    _lib.check(lib.zkhip_ifft_scaled_batch_device(d.data_ptr(), om_inv.ctypes.data, L, div.ctypes.data, V, stride, None))
    back = _host(d, (V, stride, 4))
    wrong = [NC.case_id(cs[v]) for v in range(V) if not np.array_equal(back[v], host[v])]     # canonical inputs, sentinel included
    assert wrong == []


@pytest.mark.parametrize("L", [4, 10])
@pytest.mark.parametrize("divisor", [1, R - 1], ids=["one", "r_minus_1"])
def test_scaled_inverse_with_divisor_one_and_minus_one(lib, cref, L, divisor):
    cs = NC.cases(L)
    V, N = len(cs), 1 << L
    stride = N + 1
    _, om_inv = _root(L)
    div = NC.word(NC.enc(divisor))
    pairs = [NC.vector(L, c) for c in cs]
    host = np.full((V, stride, 4), SENT, dtype=np.uint64)
    for v in range(V):
        host[v, :N] = pairs[v][1]
    d = _dev(host)
    _lib.check(lib.zkhip_ifft_scaled_batch_device(d.data_ptr(), om_inv.ctypes.data, L, div.ctypes.data, V, stride, None))
    got = _host(d, (V, stride, 4))
    assert (got[:, N:] == SENT).all()
    for v in range(V):
        ref = pairs[v][1].copy()
        cref.best_fft(ref, om_inv, L, 1)
        cref.scale(ref, div)
        assert np.array_equal(got[v, :N], ref), NC.case_id(cs[v])
        assert np.array_equal(ref, NC.words([N * x * divisor % R for x in NC.ints(pairs[v][0])])), NC.case_id(cs[v])   # N a or -N a, as words


@pytest.mark.parametrize("L", list(NC.SIZES))
def test_host_form_one_vector_at_a_time(lib, L):
    om, _ = _root(L)
    for c in NC.cases(L):
        if c.family not in ("zero", "constant", "geometric"):
            continue
        a, e = NC.vector(L, c)
        _lib.check(lib.zkhip_ntt_fr(a.ctypes.data, om.ctypes.data, L))
        assert np.array_equal(a, e), NC.case_id(c)


# ---- zero-padding ratios of coeff_to_extended -------------------------------------------------------------------------------------------------------
PAD_CASES = [(ek, k) for ek in (5, 10, 11, 19) for k in sorted({ek - d for d in (0, 1, 2, 3, 5) if ek - d >= 0} | {0}, reverse=True)]
# one-pass (5), two-pass (10, 11) and three-pass (19) sizes each see the general first round (in_len > N/4) and the shortcut (in_len <= N/4)
assert all(any(e == ek and ek - k in (0, 1) for e, k in PAD_CASES) and any(e == ek and ek - k >= 2 for e, k in PAD_CASES) for ek in (5, 10, 19))


@pytest.mark.parametrize("ek,k", PAD_CASES)
def test_coeff_to_extended_padding_ratios(lib, cref, ek, k):
    n, EN = 1 << k, 1 << ek
    ext_om, _ = _root(ek)
    polys = [cref.gen_scalars(7100 + 32 * ek + k, n, 0), np.zeros((n, 4), dtype=np.uint64)] + [np.tile(NC.word(m), (n, 1)) for m in NC.CONSTANTS.values()]
    B = len(polys)
    refs = np.zeros((B, EN, 4), dtype=np.uint64)

    def reference(b):
        refs[b, :n] = polys[b]
        cref.distribute_powers_zeta(refs[b, :n], ZETA, ZETA2)
        cref.best_fft(refs[b], ext_om, ek, 1)

    NC.for_each(reference, B, ek)
    assert not refs[1].any()
    # device form: strided in and out
    a_stride, o_stride = n + 5, EN + 3
    h_a = np.full((B, a_stride, 4), SENT, dtype=np.uint64)
    for b in range(B):
        h_a[b, :n] = polys[b]
    d_a, d_o = _dev(h_a), _dev(np.full((B, o_stride, 4), SENT, dtype=np.uint64))
    _lib.check(lib.zkhip_coeff_to_extended_device(d_a.data_ptr(), a_stride, k, d_o.data_ptr(), o_stride, ek, B, ext_om.ctypes.data, ZETA.ctypes.data, None))
    got = _host(d_o, (B, o_stride, 4))
    assert (got[:, EN:] == SENT).all()
    assert [b for b in range(B) if not np.array_equal(got[b, :EN], refs[b])] == []
    assert np.array_equal(_host(d_a, (B, a_stride, 4)), h_a)
    # host batch form
    flat = np.ascontiguousarray(np.concatenate(polys))
    out = np.full((B, EN, 4), SENT, dtype=np.uint64)
    _lib.check(lib.zkhip_coeff_to_extended_batch(flat.ctypes.data, k, out.ctypes.data, ek, B, ext_om.ctypes.data, ZETA.ctypes.data))
    assert [b for b in range(B) if not np.array_equal(out[b], refs[b])] == []
    # host form, one polynomial per call
    for b in range(B):
        one = np.full((EN, 4), SENT, dtype=np.uint64)
        _lib.check(lib.zkhip_coeff_to_extended(polys[b].ctypes.data, k, one.ctypes.data, ek, ext_om.ctypes.data, ZETA.ctypes.data))
        assert np.array_equal(one, refs[b]), b


# ---- output cuts of extended_to_coeff -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ek", [5, 10, 12])
def test_extended_to_coeff_output_cuts(lib, cref, ek):
    """ek = 5: one pass whose last round stores directly (J = 1); 10 and 12: the last pass of two.  Below out_len the uncut reference, from
    out_len to the end of the stride the sentinel."""
    k, N = ek - 2, 1 << ek
    n = 1 << k
    _, om_inv = _root(ek)
    div = NC.word(NC.enc(pow(N, -1, R)))
    polys = [cref.gen_scalars(7300 + ek, N, 0), np.zeros((N, 4), dtype=np.uint64), np.tile(NC.word(NC.CONSTANTS["enc1"]), (N, 1)),
             np.tile(NC.word(NC.CONSTANTS["raw_r_minus_1"]), (N, 1))]
    B = len(polys)
    refs = []
    for p in polys:
        ref = p.copy()
        cref.best_fft(ref, om_inv, ek, 1)
        cref.scale(ref, div)
        cref.distribute_powers_zeta(ref, ZETA2, ZETA)
        refs.append(ref)
    assert not refs[1].any() and not refs[2][1:].any() and refs[2][0].any()            # constant evaluations: one coefficient, N - 1 exact zeros
    a_stride, o_stride = N + 1, N + 2
    h_a = np.full((B, a_stride, 4), SENT, dtype=np.uint64)
    for b in range(B):
        h_a[b, :N] = polys[b]
    d_a = _dev(h_a)
    blank = np.full((B, o_stride, 4), SENT, dtype=np.uint64)

    def device_call(out_len):
        d_o = _dev(blank)
        rc = lib.zkhip_extended_to_coeff_device(d_a.data_ptr(), a_stride, ek, om_inv.ctypes.data, div.ctypes.data, ZETA.ctypes.data, d_o.data_ptr(), o_stride,
                                                out_len, B, None)
        return rc, _host(d_o, (B, o_stride, 4))

    def host_call(b, out_len):
        a, out = polys[b].copy(), np.full((o_stride, 4), SENT, dtype=np.uint64)
        rc = lib.zkhip_extended_to_coeff(a.ctypes.data, ek, om_inv.ctypes.data, div.ctypes.data, ZETA.ctypes.data, out.ctypes.data, out_len)
        return rc, out

    for out_len in [1, 3, n - 1, 3 * n, 3 * n + 1, N - 1, N]:
        rc, got = device_call(out_len)
        assert rc == 0, out_len
        for b in range(B):
            assert np.array_equal(got[b, :out_len], refs[b][:out_len]), (out_len, b)
            assert (got[b, out_len:] == SENT).all(), (out_len, b)
            rc, out = host_call(b, out_len)
            assert rc == 0 and np.array_equal(out[:out_len], refs[b][:out_len]) and (out[out_len:] == SENT).all(), (out_len, b)
    rc, got = device_call(0)
    assert rc == 0 and np.array_equal(got, blank)
    rc, got = device_call(N + 1)
    assert rc == EINVAL and np.array_equal(got, blank)
    rc, out = host_call(0, N + 1)
    assert rc == EINVAL and (out == SENT).all()
    rc, got = device_call(3 * n)                                                       # both forms still work after a refusal
    assert rc == 0 and all(np.array_equal(got[b, :3 * n], refs[b][:3 * n]) for b in range(B))
    rc, out = host_call(0, 3 * n)
    assert rc == 0 and np.array_equal(out[:3 * n], refs[0][:3 * n])
    assert np.array_equal(_host(d_a, (B, a_stride, 4)), h_a)


# ---- mul_periodic ---------------------------------------------------------------------------------------------------------------------------------
def _with_edges(cref, seed, count, step, first):
    """seeded words with 0, 1 and r - 1 (encoded) at every `step`-th place, in turn, starting with edge number `first`"""
    a = cref.gen_scalars(seed, count, 0)
    edges = [NC.word(NC.CONSTANTS[k]) for k in ("enc0", "enc1", "enc_r_minus_1")]
    for i in range(0, count, step):
        a[i] = edges[(i // step + first) % 3]
    return a


def _mul_periodic_both_forms(lib, cref, n, period):
    a = _with_edges(cref, 7500 + n % 1000 + period, n, 2 if n < 1000 else 5, 0)
    table = _with_edges(cref, 7600 + period, period, 1 if period <= 4 else 3, period)
    ref = a.copy()
    cref.mul_periodic(ref, table)
    assert not ref[0].any()                                                            # 0 times anything: an exact zero to canonicalise
    h = np.full((n + 2, 4), SENT, dtype=np.uint64)
    h[:n] = a
    d_a, d_t = _dev(h), _dev(table)
    _lib.check(lib.zkhip_mul_periodic_device(d_a.data_ptr(), n, d_t.data_ptr(), period, None))
    got = _host(d_a, (n + 2, 4))
    assert np.array_equal(got[:n], ref) and (got[n:] == SENT).all(), (n, period, "device")
    assert np.array_equal(_host(d_t, (period, 4)), table)
    b = a.copy()
    _lib.check(lib.zkhip_mul_periodic(b.ctypes.data, n, table.ctypes.data, period))
    assert np.array_equal(b, ref), (n, period, "host")


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_mul_periodic_small_sizes_and_periods(lib, cref, n):
    for period in sorted({1, 2, 3, 4, 7, n, n + 3}):                                   # a period above n reads only its first n entries
        _mul_periodic_both_forms(lib, cref, n, period)


@pytest.mark.parametrize("period", [3, 8])
def test_mul_periodic_second_trip_of_the_stride_loop(lib, cref, period):
    _mul_periodic_both_forms(lib, cref, (1 << 20) + 5, period)                         # the grid is capped at 4096 x 256 = 2^20 threads

"""GPU: random field elements drawn in HBM (`zkhip_fr_random_device`, `zkhip_fr_random`, `zkhip_fr_random_rows_device`) against the restatement
of the stream in tests/test_fr_random_host.py (a numpy ChaCha20 pinned by RFC 8439, reduced mod r in big integers).  Every comparison is of
bytes: exact equality, no tolerance.  The stream is addressed by index, so one call equals the same range cut anywhere -- inside a wavefront,
inside a workgroup -- and the rows form equals the flat stream."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zksnap_circuits_halo2_amd as Z
from test_fr_random_host import PINS, SEED, restate, stored_number
from zksnap_circuits_halo2_amd import _lib, arithmetic as A, evaluation as E

pytestmark = pytest.mark.gpu
ZKHIP_EINVAL = -1
DEV = torch.device("cuda", 0)
M64 = (1 << 64) - 1
SENTINEL = 0x5E5E5E5E5E5E5E5E


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _sentinel(rows):
    return torch.full((rows, 4), SENTINEL, dtype=torch.int64, device=DEV)


def test_pins_through_the_host_form(lib):
    for first, stream_id, stored in PINS:
        got = A.random_fr(SEED, 1, first=first, stream_id=stream_id)
        assert got.shape == (1, 4) and stored_number(got[0]) == stored, hex(first)
    # ... and a run of the host form equals the device form
    host = A.random_fr(SEED, 1000, first=12345, stream_id=9)
    device = E.random_fr_device(SEED, 1000, first=12345, stream_id=9)
    torch.cuda.synchronize()
    assert np.array_equal(host, _host(device))


def test_a_column_equals_the_restatement_in_full(lib):
    n = (1 << 16) + 37
    got = E.random_fr_device(SEED, n)
    torch.cuda.synchronize()
    assert np.array_equal(_host(got), restate(SEED, 0, list(range(n))))


def test_one_call_equals_the_range_cut_at_uneven_points(lib):
    n = 1 << 22
    seed, stream_id, first = bytes(range(7, 39)), 0xABCDEF0123, (1 << 32) - (1 << 21) - 11           # the counter's low word wraps inside the range
    whole = E.random_fr_device(seed, n, first=first, stream_id=stream_id)
    # cuts inside a wavefront (1, 63, 65, 100), inside a workgroup (255, 257, 1000), and far from any power of two
    cuts = [0, 1, 63, 64, 65, 100, 255, 256, 257, 1000, (1 << 16) + 37, (1 << 20) + 13, (1 << 21) - 1, (1 << 21) + 129, n - 300, n - 1, n]
    pieces = _sentinel(n)
    for lo, hi in zip(cuts, cuts[1:]):
        E.random_fr_device(seed, hi - lo, first=first + lo, stream_id=stream_id, out=pieces[lo:hi])
    torch.cuda.synchronize()
    assert torch.equal(whole, pieces)
    rng = random.Random(22)
    idx = {0, n - 1, 63, 64, 255, 256, (1 << 21) + 10, (1 << 21) + 11}                           # the first, the last, the wrap of the low word
    while len(idx) < 4096:
        idx.add(rng.randrange(n))
    idx = sorted(idx)
    sample = _host(whole[torch.tensor(idx, device=DEV)])
    assert np.array_equal(sample, restate(seed, stream_id, [first + i for i in idx]))


def test_counters_at_their_edges_and_the_end_of_the_stream(lib):
    for first in ((1 << 32) - 5, (1 << 64) - 64):
        got = E.random_fr_device(SEED, 64, first=first, stream_id=3)
        torch.cuda.synchronize()
        assert np.array_equal(_host(got), restate(SEED, 3, [first + j for j in range(64)])), hex(first)
    buf = _sentinel(64)
    seed = (C.c_uint8 * 32)(*SEED)
    rc = lib.zkhip_fr_random_device(seed, 3, (1 << 64) - 63, 64, buf.data_ptr(), None)          # first + n = 2^64 + 1
    torch.cuda.synchronize()
    assert rc == ZKHIP_EINVAL and b"2^64" in lib.zkhip_last_error()
    assert torch.equal(buf, _sentinel(64))
    out = np.full((64, 4), SENTINEL, dtype=np.uint64)
    assert lib.zkhip_fr_random(seed, 3, (1 << 64) - 63, 64, out.ctypes.data) == ZKHIP_EINVAL and (out == SENTINEL).all()


@pytest.mark.parametrize("count", [1, 5, 6])
@pytest.mark.parametrize("n_cols", [1, 3, 270, 2048])
def test_rows_form_equals_the_flat_stream_and_touches_nothing_else(lib, n_cols, count):
    rows = 1 << 13
    row0 = rows - count
    seed, stream_id, first = bytes(range(100, 132)), 5, (1 << 32) - 1000
    cols = [_sentinel(rows) for _ in range(n_cols)]                                              # separately allocated columns
    E.blind_rows_device(cols, row0, count, seed, first=first, stream_id=stream_id)
    flat = E.random_fr_device(seed, n_cols * count, first=first, stream_id=stream_id)
    torch.cuda.synchronize()
    got = torch.stack(cols)                                                                      # (n_cols, rows, 4)
    assert torch.equal(got[:, row0:, :].reshape(-1, 4), flat)
    assert bool((got[:, :row0, :] == SENTINEL).all())
    assert np.array_equal(_host(flat), restate(seed, stream_id, [first + i for i in range(n_cols * count)]))


def test_seed_and_pointer_array_are_consumed_before_the_call_returns(lib):
    """both are overwritten as soon as the call returns, with work still queued on the stream in front of it"""
    rows, n_cols, count = 1 << 13, 270, 5
    side = torch.cuda.Stream(device=DEV)
    sid = side.cuda_stream
    busy = torch.empty((1 << 24, 4), dtype=torch.int64, device=DEV)
    cols = [_sentinel(rows) for _ in range(n_cols)]
    decoy = _sentinel(rows)
    flat = _sentinel(1 << 20)
    torch.cuda.synchronize()
    seed = (C.c_uint8 * 32)(*SEED)
    ptrs = (C.c_void_p * n_cols)(*[c.data_ptr() for c in cols])
    assert lib.zkhip_fr_random_device(seed, 0, 0, 1 << 24, busy.data_ptr(), sid) == 0           # the stream is busy for a while
    assert lib.zkhip_fr_random_rows_device(seed, 1, 77, ptrs, n_cols, rows - count, count, sid) == 0
    assert lib.zkhip_fr_random_device(seed, 2, 99, 1 << 20, flat.data_ptr(), sid) == 0
    for i in range(32):
        seed[i] = 0xEE
    for c in range(n_cols):
        ptrs[c] = decoy.data_ptr()
    side.synchronize()
    torch.cuda.synchronize()
    want_rows = restate(SEED, 1, [77 + i for i in range(n_cols * count)])
    assert np.array_equal(_host(torch.stack(cols)[:, rows - count:, :].reshape(-1, 4)), want_rows)
    assert torch.equal(decoy, _sentinel(rows))
    sample = [0, 1, 4095, (1 << 20) - 1]
    assert np.array_equal(_host(flat)[sample], restate(SEED, 2, [99 + i for i in sample]))


def test_no_ops_and_bad_arguments_return_a_status(lib):
    seed = (C.c_uint8 * 32)(*SEED)
    buf = _sentinel(64)
    ptrs = (C.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + 32 * 32)
    # no-ops: nothing is read, nothing is written (null pointers are fine)
    assert lib.zkhip_fr_random_device(None, 0, 0, 0, None, None) == 0
    assert lib.zkhip_fr_random(None, 0, 0, 0, None) == 0
    assert lib.zkhip_fr_random_rows_device(seed, 0, 0, ptrs, 0, 0, 5, None) == 0
    assert lib.zkhip_fr_random_rows_device(seed, 0, 0, ptrs, 2, 0, 0, None) == 0
    assert lib.zkhip_fr_random_rows_device(None, 0, 0, None, 0, 0, 0, None) == 0
    # null pointers
    assert lib.zkhip_fr_random_device(None, 0, 0, 64, buf.data_ptr(), None) == ZKHIP_EINVAL
    assert lib.zkhip_fr_random_device(seed, 0, 0, 64, None, None) == ZKHIP_EINVAL
    assert lib.zkhip_fr_random(seed, 0, 0, 64, None) == ZKHIP_EINVAL
    assert lib.zkhip_fr_random_rows_device(None, 0, 0, ptrs, 2, 0, 5, None) == ZKHIP_EINVAL
    assert lib.zkhip_fr_random_rows_device(seed, 0, 0, None, 2, 0, 5, None) == ZKHIP_EINVAL
    null_col = (C.c_void_p * 2)(buf.data_ptr(), None)
    assert lib.zkhip_fr_random_rows_device(seed, 0, 0, null_col, 2, 0, 5, None) == ZKHIP_EINVAL
    # first + n_cols * count above 2^64
    assert lib.zkhip_fr_random_rows_device(seed, 0, (1 << 64) - 9, ptrs, 2, 0, 5, None) == ZKHIP_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf, _sentinel(64))
    assert lib.zkhip_fr_random_rows_device(seed, 0, (1 << 64) - 10, ptrs, 2, 0, 5, None) == 0      # the last ten indices of the stream
    torch.cuda.synchronize()
    got = _host(buf)
    assert np.array_equal(np.concatenate([got[0:5], got[32:37]]), restate(SEED, 0, [(1 << 64) - 10 + i for i in range(10)]))
    assert (got[5:32] == SENTINEL).all() and (got[37:] == SENTINEL).all()


def test_a_filled_column_commits_to_the_oracles_point(lib, cref):
    """the vanishing argument's use: fill a column of 2^16 coefficients in HBM, commit it against params.g -- the same point as the oracle's
    multi-exponentiation over the RESTATED coefficients"""
    k = 16
    n = 1 << k
    seed = bytes(range(200, 232))
    with Z.ParamsKZG.setup(k, 0x5EED5) as params:
        col = E.random_fr_device(seed, n, first=0, stream_id=1)
        point = torch.zeros(12, dtype=torch.int64, device=DEV)
        params.commit_device(col.data_ptr(), n, point.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        coeffs = restate(seed, 1, list(range(n)))
        want = cref.jac_to_affine(cref.best_multiexp(np.ascontiguousarray(coeffs), np.ascontiguousarray(params.g), 4))
        assert np.array_equal(cref.jac_to_affine(_host(point)), want)
        assert np.array_equal(cref.jac_to_affine(params.commit(_host(col))), want)


def test_prove_flow_with_device_randomness_keeps_every_invariant(lib):
    """tools/prove_flow.py --device-randomness: every blinding tail through the rows call, the vanishing argument's random polynomial filled and
    committed on the device; the prover's own invariants hold as in the default flow, whose laps are unchanged"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_flow

    for lookups_one_call in (True, False):
        r = prove_flow.run(13, 8, lookups=2, verbose=False, device_randomness=True, lookups_one_call=lookups_one_call)
        assert all(r["checks"].values()), r["checks"]
        assert "vanishing_random_poly" in r["timings_ms"] and r["vanishing_random_commitment"] is not None
    r0 = prove_flow.run(13, 8, lookups=2, verbose=False)
    assert all(r0["checks"].values()) and "vanishing_random_poly" not in r0["timings_ms"] and r0["vanishing_random_commitment"] is None

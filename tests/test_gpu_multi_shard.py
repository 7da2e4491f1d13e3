"""GPU (-m gpu): the multi-GPU MSM and the thread / stream rules of the C ABI.

One process, `zkhip_init(devices, ndev)`, `zkhip_register_bases` sharding the SRS by point range, `zkhip_msm_g1` fanning the scalar
slices out, gathering the 96-byte partials and folding them.  The test box has ONE card, so the path is rehearsed two ways:
virtual shards (`zkhip_set_msm_shards`: S tables, S Pippenger runs, gather, fold on one device) and duplicate device contexts
(`ZKHIP_TEST_DUPLICATE_DEVICES=1` + `zkhip_init([0, 0, 0], 3)`: the worker threads, per-device lanes and peer copies of the real
multi-device path, all landing on the same card).  A sum of points is a unique group element, so every shard count must give the
same affine point as the unsharded MSM and as the structured-SRS identity."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F

pytestmark = pytest.mark.gpu
D = 0x9E3779B97F4A7C15F39CC0605CEDC835
T0 = 0x5A4B534E41500002 + 1001


def _walk_host(lib, n, t0=T0):
    """host copy of the structured SRS (t0 + i D) G, generated on the device"""
    import torch

    bases = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    t0m, dm = F.fr_encode([t0])[0], F.fr_encode([D])[0]
    _lib.check(lib.zkhip_g1_gen_walk_device(t0m.ctypes.data, dm.ctypes.data, n, bases.data_ptr(), None))
    torch.cuda.synchronize()
    return np.ascontiguousarray(bases.cpu().numpy().view(np.uint64).reshape(n, 8))


def _expect(cref, sc, t0):
    return cref.jac_to_affine(cref.scalar_mul(cref.expected_scalar(sc, t0, D), cref.generator()))


def _msm(lib, sc, bases):
    out = np.zeros(12, dtype=np.uint64)
    _lib.check(lib.zkhip_msm_g1(sc.ctypes.data, bases.ctypes.data, sc.shape[0], out.ctypes.data))
    return out


@pytest.fixture
def restore_shards(lib):
    yield
    lib.zkhip_set_msm_shards(0)


@pytest.mark.parametrize("n", [10007, (1 << 17) + 3])
def test_virtual_shards_equal_unsharded(lib, cref, restore_shards, n):
    bases = _walk_host(lib, n)
    sc = cref.gen_scalars(9100 + n % 13, n, 0)
    sc[5] = 0
    bases_with_id = bases.copy(); bases_with_id[17] = 0          # an identity base inside shard 0
    exp = _expect(cref, sc, T0)
    results = {}
    for S in (1, 3, 8):
        _lib.check(lib.zkhip_set_msm_shards(S))
        assert lib.zkhip_msm_shards() == S
        _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
        try:
            full = cref.jac_to_affine(_msm(lib, sc, bases))
            assert np.array_equal(full, exp), S
            # sub-ranges: inside one shard, across a shard boundary, a prefix (what ParamsKZG::commit of a short polynomial passes)
            for lo, hi in ((3, 100), (n // 8 - 50, n // 8 + 60), (0, n - 1), (n // 3 - 1, 2 * n // 3 + 5), (n - 9, n)):
                part = cref.jac_to_affine(_msm(lib, np.ascontiguousarray(sc[lo:hi]), bases[lo:hi]))
                assert np.array_equal(part, _expect(cref, np.ascontiguousarray(sc[lo:hi]), (T0 + lo * D) % O.R_MOD)), (S, lo, hi)
            results[S] = full
        finally:
            _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
    assert np.array_equal(results[1], results[3]) and np.array_equal(results[1], results[8])
    # fewer points than shards, and the empty MSM
    _lib.check(lib.zkhip_set_msm_shards(8))
    _lib.check(lib.zkhip_register_bases(bases.ctypes.data, 5))
    try:
        assert np.array_equal(cref.jac_to_affine(_msm(lib, np.ascontiguousarray(sc[:5]), bases[:5])), _expect(cref, np.ascontiguousarray(sc[:5]), T0))
        assert F.g1_decode_jacobian(_msm(lib, np.zeros((0, 4), dtype=np.uint64), bases[:0])) is None
    finally:
        _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
    del bases_with_id


def test_config4_rehearsal_8_shards_of_2p21(lib, cref, restore_shards):
    """BASELINE configs[4]: the wrapper circuit at k + 2 = 24, MSM sharded over 8 GPUs = 2^21 points per shard -- here 8 shards on the
    one card, through the same register / fan-out / gather / fold code the 8-GPU host runs"""
    n = 1 << 24
    bases = _walk_host(lib, n)
    sc = cref.gen_scalars(92400, n, 0)
    _lib.check(lib.zkhip_set_msm_shards(8))
    _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
    try:
        assert np.array_equal(cref.jac_to_affine(_msm(lib, sc, bases)), _expect(cref, sc, T0))
    finally:
        _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))


def test_stale_registration_is_not_trusted(lib, cref):
    """memory that still carries a registration but no longer the registered points (freed and reused, or modified in place) must not
    be multiplied against the stale table: the sampled-point guard sends the call down the general path"""
    n = 5000
    bases = _walk_host(lib, n)
    sc = cref.gen_scalars(9300, n, 0)
    _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
    try:
        assert np.array_equal(cref.jac_to_affine(_msm(lib, sc, bases)), _expect(cref, sc, T0))
        other = _walk_host(lib, n, T0 + 77)
        bases[:] = other                                          # same address, different points
        assert np.array_equal(cref.jac_to_affine(_msm(lib, sc, bases)), _expect(cref, sc, T0 + 77))
    finally:
        _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))


def test_two_host_threads_on_two_streams(lib, cref):
    """`_device` calls from two host threads, each on its own stream, at the same time: scratch memory belongs to the stream, so the MSMs,
    transforms and row-a7 passes of one thread must not disturb the other's"""
    import torch

    n, L = 1 << 16, 16
    errors, ok = [], {}
    t0m, dm = F.fr_encode([T0])[0], F.fr_encode([D])[0]
    bases = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_g1_gen_walk_device(t0m.ctypes.data, dm.ctypes.data, n, bases.data_ptr(), None))
    h = C.c_uint64(0)
    _lib.check(lib.zkhip_prepare_bases_device(bases.data_ptr(), n, C.byref(h)))
    om = F.fr_encode([F.omega_for(L)])[0]
    omi = F.fr_encode([pow(F.omega_for(L), -1, F.R_MOD)])[0]
    div = F.fr_encode([pow(n, -1, F.R_MOD)])[0]
    torch.cuda.synchronize()

    def work(tid):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for rep in range(6):
                    sc = cref.gen_scalars(9400 + 16 * tid + rep, n, rep % 2)
                    dsc = torch.from_numpy(sc.view(np.int64)).cuda()
                    out = torch.zeros(12, dtype=torch.int64, device="cuda")
                    out2 = torch.zeros(12, dtype=torch.int64, device="cuda")
                    poly = dsc.clone()
                    st.synchronize()
                    s = st.cuda_stream
                    _lib.check(lib.zkhip_msm_g1_prepared_device(h, 0, dsc.data_ptr(), n, out.data_ptr(), s))
                    _lib.check(lib.zkhip_ntt_fr_device(poly.data_ptr(), om.ctypes.data, L, s))
                    _lib.check(lib.zkhip_msm_g1_device(dsc.data_ptr(), bases.data_ptr(), n, out2.data_ptr(), s))
                    _lib.check(lib.zkhip_ifft_scaled_device(poly.data_ptr(), omi.ctypes.data, L, div.ctypes.data, s))
                    st.synchronize()
                    exp = cref.jac_to_affine(cref.scalar_mul(cref.expected_scalar(sc, T0, D), cref.generator()))
                    a = cref.jac_to_affine(np.ascontiguousarray(out.cpu().numpy().view(np.uint64)))
                    b = cref.jac_to_affine(np.ascontiguousarray(out2.cpu().numpy().view(np.uint64)))
                    ok[(tid, rep)] = bool(np.array_equal(a, exp) and np.array_equal(b, exp) and torch.equal(poly, dsc))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    _lib.check(lib.zkhip_release_bases(h))
    assert not errors, errors
    assert len(ok) == 12 and all(ok.values()), ok


def test_two_host_threads_share_the_side_stream_of_large_batches(lib, cref):
    """two host threads, each on its own stream, call the batch entry point with wide-window tables at the same time: both use the
    library's one side stream (fork / join events are recorded per call under the library lock), and every result must be right"""
    import torch

    n, batch = 1 << 20, 2
    errors, ok = [], {}
    t0m, dm = F.fr_encode([T0])[0], F.fr_encode([D])[0]
    bases = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    _lib.check(lib.zkhip_g1_gen_walk_device(t0m.ctypes.data, dm.ctypes.data, n, bases.data_ptr(), None))
    h = C.c_uint64(0)
    _lib.check(lib.zkhip_prepare_bases_device(bases.data_ptr(), n, C.byref(h)))
    assert lib.zkhip_prepared_window_bits(h) > 16
    torch.cuda.synchronize()

    def work(tid):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for rep in range(3):
                    vecs = [cref.gen_scalars(9700 + 16 * tid + 2 * rep + i, n, i) for i in range(batch)]
                    dsc = torch.from_numpy(np.ascontiguousarray(np.stack(vecs)).view(np.int64)).cuda()
                    out = torch.zeros((batch, 12), dtype=torch.int64, device="cuda")
                    st.synchronize()
                    _lib.check(lib.zkhip_msm_g1_prepared_batch_device(h, 0, dsc.data_ptr(), n, batch, n, out.data_ptr(), st.cuda_stream))
                    st.synchronize()
                    got = out.cpu().numpy().view(np.uint64)
                    for i in range(batch):
                        exp = cref.jac_to_affine(cref.scalar_mul(cref.expected_scalar(vecs[i], T0, D), cref.generator()))
                        ok[(tid, rep, i)] = bool(np.array_equal(cref.jac_to_affine(np.ascontiguousarray(got[i])), exp))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    _lib.check(lib.zkhip_release_bases(h))
    assert not errors, errors
    assert len(ok) == 12 and all(ok.values()), ok


def test_host_calls_overlap_on_lanes(lib, cref):
    """host-buffer calls from four threads: each borrows a lane (two by default), none holds the library lock while it waits for
    the device; all results right"""
    n = 1 << 15
    bases = _walk_host(lib, n)
    _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
    res, errors = {}, []

    def work(tid):
        try:
            for rep in range(5):
                sc = cref.gen_scalars(9500 + 8 * tid + rep, n, 0)
                got = cref.jac_to_affine(_msm(lib, sc, bases))
                a = cref.gen_scalars(9600 + 8 * tid + rep, 1 << 14, 0)
                ref = a.copy()
                om = F.fr_encode([F.omega_for(14)])[0]
                cref.best_fft(ref, om, 14, 1)
                _lib.check(lib.zkhip_ntt_fr(a.ctypes.data, om.ctypes.data, 14))
                res[(tid, rep)] = bool(np.array_equal(got, _expect(cref, sc, T0)) and np.array_equal(a, ref))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    try:
        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
    assert not errors, errors
    assert len(res) == 20 and all(res.values())


def test_multi_device_path_on_duplicate_contexts(lib, cref):
    """zkhip_init with three device contexts (the same card three times under ZKHIP_TEST_DUPLICATE_DEVICES): registered bases are cut
    into one shard per context, the secondary contexts run on their worker threads and send their partials with peer copies.
    Also the unregistered case, which splits bases and scalars evenly over the devices."""
    n = (1 << 16) + 11
    lib.zkhip_shutdown()
    os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
    try:
        devs = (C.c_int * 3)(0, 0, 0)
        _lib.check(lib.zkhip_init(devs, 3))
        assert lib.zkhip_device_count() == 3 and lib.zkhip_msm_shards() == 3
        bases = _walk_host(lib, n)
        sc = cref.gen_scalars(9700, n, 0)
        exp = _expect(cref, sc, T0)
        assert np.array_equal(cref.jac_to_affine(_msm(lib, sc, bases)), exp)          # not registered: even split, general path per device
        _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
        try:
            for rep in range(3):
                assert np.array_equal(cref.jac_to_affine(_msm(lib, sc, bases)), exp), rep
            lo, hi = n // 3 - 100, n // 3 + 100                                        # two shards, two devices
            assert np.array_equal(cref.jac_to_affine(_msm(lib, np.ascontiguousarray(sc[lo:hi]), bases[lo:hi])),
                                  _expect(cref, np.ascontiguousarray(sc[lo:hi]), (T0 + lo * D) % O.R_MOD))
            _lib.check(lib.zkhip_set_msm_shards(7))                                    # more shards than devices: round robin
            _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))                 # re-registration replaces the tables
            assert np.array_equal(cref.jac_to_affine(_msm(lib, sc, bases)), exp)
        finally:
            _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
        # the `_device` entry points keep working on the primary context
        a = cref.gen_scalars(9701, 1 << 12, 0)
        ref = a.copy()
        om = F.fr_encode([F.omega_for(12)])[0]
        cref.best_fft(ref, om, 12, 1)
        _lib.check(lib.zkhip_ntt_fr(a.ctypes.data, om.ctypes.data, 12))
        assert np.array_equal(a, ref)
    finally:
        lib.zkhip_shutdown()
        del os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"]
        _lib.check(lib.zkhip_init(None, 0))


def _registered_device(lib, bases_host, d_sc, n, batch=1, stride=None, stream=None):
    """zkhip_msm_g1_registered(_batch)_device with the scalars at torch tensor d_sc; returns (batch, 12) uint64"""
    import torch

    out = torch.zeros((batch, 12), dtype=torch.int64, device="cuda")
    if batch == 1 and stride is None:
        _lib.check(lib.zkhip_msm_g1_registered_device(bases_host.ctypes.data, d_sc.data_ptr(), n, out.data_ptr(), stream))
    else:
        _lib.check(lib.zkhip_msm_g1_registered_batch_device(bases_host.ctypes.data, d_sc.data_ptr(), n, batch, stride if stride is not None else n, out.data_ptr(), stream))
    torch.cuda.synchronize()
    return np.ascontiguousarray(out.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("n", [10007, (1 << 17) + 3])
def test_device_resident_commit_over_virtual_shards(lib, cref, restore_shards, n):
    """zkhip_msm_g1_registered_device on a range that spans several shards (round 2 returned EINVAL here): 1 / 3 / 8 virtual shards give the
    unsharded point and the structured-SRS point, for the whole array, for sub-ranges across shard boundaries and for a batch of vectors
    with a padded stride"""
    import torch

    bases = _walk_host(lib, n)
    sc = cref.gen_scalars(9800 + n % 13, n, 0)
    sc[7] = 0
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    exp = _expect(cref, sc, T0)
    batch, stride = 3, n + 5
    vecs = [cref.gen_scalars(9810 + i, n, i % 2) for i in range(batch)]
    padded = np.zeros((batch, stride, 4), dtype=np.uint64)
    for i, v in enumerate(vecs):
        padded[i, :n] = v
    d_vecs = torch.from_numpy(padded.view(np.int64)).cuda()
    exp_vecs = [_expect(cref, v, T0) for v in vecs]
    for S in (1, 3, 8):
        _lib.check(lib.zkhip_set_msm_shards(S))
        _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
        try:
            assert np.array_equal(cref.jac_to_affine(_registered_device(lib, bases, d_sc, n)[0]), exp), S
            for lo, hi in ((3, 100), (n // 8 - 50, n // 8 + 60), (0, n - 1), (n // 3 - 1, 2 * n // 3 + 5), (n - 9, n)):
                got = _registered_device(lib, bases[lo:], d_sc.view(-1, 4)[lo:], hi - lo)[0]
                assert np.array_equal(cref.jac_to_affine(got), _expect(cref, np.ascontiguousarray(sc[lo:hi]), (T0 + lo * D) % O.R_MOD)), (S, lo, hi)
            got = _registered_device(lib, bases, d_vecs, n, batch, stride)
            for i in range(batch):
                assert np.array_equal(cref.jac_to_affine(got[i]), exp_vecs[i]), (S, i)
            # on a caller stream of its own: the fold is ordered on that stream
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                assert np.array_equal(cref.jac_to_affine(_registered_device(lib, bases, d_sc, n, stream=st.cuda_stream)[0]), exp), S
        finally:
            _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
    # n = 0 and an unregistered pointer
    assert F.g1_decode_jacobian(_registered_device(lib, bases, d_sc, 0)[0]) is None
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    assert lib.zkhip_msm_g1_registered_device(bases.ctypes.data, d_sc.data_ptr(), n, out.data_ptr(), None) == -1


def test_device_resident_commit_on_duplicate_contexts(lib, cref):
    """the same with three device contexts on the one card (ZKHIP_TEST_DUPLICATE_DEVICES): the secondary contexts wait for the caller's
    stream by event, pull their scalar slices with peer copies, run on their own streams and return their partials with peer copies; the
    caller's stream waits for their events and folds.  Host-buffer calls (worker threads, the secondaries' lanes) interleave with it."""
    import torch

    n = (1 << 16) + 11
    lib.zkhip_shutdown()
    os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
    try:
        devs = (C.c_int * 3)(0, 0, 0)
        _lib.check(lib.zkhip_init(devs, 3))
        bases = _walk_host(lib, n)
        sc = cref.gen_scalars(9900, n, 0)
        d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
        exp = _expect(cref, sc, T0)
        batch = 4
        vecs = [cref.gen_scalars(9910 + i, n, i % 2) for i in range(batch)]
        d_vecs = torch.from_numpy(np.ascontiguousarray(np.stack(vecs)).view(np.int64)).cuda()
        for S in (3, 7):
            _lib.check(lib.zkhip_set_msm_shards(S))
            _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
            try:
                for rep in range(3):
                    assert np.array_equal(cref.jac_to_affine(_registered_device(lib, bases, d_sc, n)[0]), exp), (S, rep)
                    assert np.array_equal(cref.jac_to_affine(_msm(lib, sc, bases)), exp), (S, rep)          # host-buffer path in between
                lo, hi = n // 3 - 100, n // 3 + 100
                got = _registered_device(lib, bases[lo:], d_sc.view(-1, 4)[lo:], hi - lo)[0]
                assert np.array_equal(cref.jac_to_affine(got), _expect(cref, np.ascontiguousarray(sc[lo:hi]), (T0 + lo * D) % O.R_MOD)), S
                got = _registered_device(lib, bases, d_vecs, n, batch, n)
                for i in range(batch):
                    assert np.array_equal(cref.jac_to_affine(got[i]), _expect(cref, vecs[i], T0)), (S, i)
                # scalars produced on the caller's stream right before the call: the secondaries must wait for them
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    d2 = torch.zeros_like(d_sc)
                    for _ in range(20):
                        d2.copy_(d_vecs[0])
                    d2.copy_(d_sc)
                    out = torch.zeros(12, dtype=torch.int64, device="cuda")
                    _lib.check(lib.zkhip_msm_g1_registered_device(bases.ctypes.data, d2.data_ptr(), n, out.data_ptr(), st.cuda_stream))
                st.synchronize()
                assert np.array_equal(cref.jac_to_affine(np.ascontiguousarray(out.cpu().numpy().view(np.uint64))), exp), S
            finally:
                _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))
    finally:
        lib.zkhip_shutdown()
        del os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"]
        _lib.check(lib.zkhip_init(None, 0))


def test_config4_device_resident_8_shards_of_2p21(lib, cref, restore_shards):
    """BASELINE configs[4] with the scalars resident in HBM: the 2^24-point commit as 8 registered shards of 2^21 points through
    zkhip_msm_g1_registered_device"""
    import torch

    n = 1 << 24
    bases = _walk_host(lib, n)
    sc = cref.gen_scalars(92401, n, 0)
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    _lib.check(lib.zkhip_set_msm_shards(8))
    _lib.check(lib.zkhip_register_bases(bases.ctypes.data, n))
    try:
        assert np.array_equal(cref.jac_to_affine(_registered_device(lib, bases, d_sc, n)[0]), _expect(cref, sc, T0))
    finally:
        _lib.check(lib.zkhip_unregister_bases(bases.ctypes.data))


def test_reinit_with_other_devices_while_a_host_call_runs_is_refused(lib, cref):
    """zkhip_init with a different device list used to wait for the running host-buffer calls on a mutex it held twice (a deadlock: the lane
    holder could never take the lock to give its lane back); it now returns ZKHIP_EBUSY while a lane is busy and re-initialises afterwards"""
    L = 24
    a = cref.gen_scalars(9950, 1 << L, 0)
    om = F.fr_encode([F.omega_for(L)])[0]
    rcs, done = [], threading.Event()

    def long_call():
        rcs.append(lib.zkhip_ntt_fr(a.ctypes.data, om.ctypes.data, L))        # 512 MiB each way over PCIe: tens of milliseconds on a lane
        done.set()

    os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
    try:
        devs = (C.c_int * 2)(0, 0)
        t = threading.Thread(target=long_call)
        t.start()
        seen = []
        while not done.is_set():
            rc = lib.zkhip_init(devs, 2)
            seen.append(rc)
            if rc == 0:
                break                                  # the call had already finished (or not yet begun): the re-init went through
        t.join()
        assert rcs == [0]
        assert all(rc in (0, -5) for rc in seen), seen
        if -5 in seen:
            assert b"in flight" in lib.zkhip_last_error()
        _lib.check(lib.zkhip_init(devs, 2))            # nothing is running now: accepted
        assert lib.zkhip_device_count() == 2
    finally:
        lib.zkhip_shutdown()
        del os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"]
        _lib.check(lib.zkhip_init(None, 0))


def _config4_worker(rank, world, port, q):
    """one rank of bench.py's configs[4] leg (world > 1 branch), gloo in place of RCCL, all ranks on the one card of the test box"""
    import os
    import sys

    import torch
    import torch.distributed as dist

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from oracle import cpu_ref as Cr
    from zksnap_circuits_halo2_amd import _lib as L, fields as FF
    from zksnap_circuits_halo2_amd.multi_gpu import gather_fold_device

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    lib = L.load()
    dev = torch.device("cuda", 0)
    dbg = {}
    res = bench.config4_leg(lib, L, FF, torch, dist, dev, torch.cuda.current_stream().cuda_stream, rank, world, gather_fold_device, debug=dbg)
    # every rank's share of the expected scalar, summed over the ranks: MSM = [sum_r sum_i a_{r,i} (t0_r + i d)] G
    mine = Cr.expected_scalar(dbg["scalars"], dbg["t0"], dbg["d"])
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    exp = Cr.jac_to_affine(Cr.scalar_mul(sum(parts) % FF.R_MOD, Cr.generator()))
    got = Cr.jac_to_affine(np.ascontiguousarray(dbg["final"]))
    q.put((rank, bool(np.array_equal(got, exp)), res["Mpoints_per_s"], res["workload"], res["ranks_seen"], res["result_checked"]))
    dist.barrier()
    dist.destroy_process_group()


def test_bench_config4_leg_four_ranks_on_one_gpu():
    """bench.py's configs[4] leg as `--gpus N` runs it (2^24 points split over the ranks, prepared MSM per rank, all_gather of the 96-byte
    partials, fold), with 4 processes of 2^22 points each on this box's one GPU (the pool allows at most 6 processes on the card, so the
    8 x 2^21 split runs as 8 shards inside one process instead: test_config4_rehearsal_8_shards_of_2p21); every rank's folded result must
    be the structured-SRS point of the whole 2^24-point MSM"""
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 4
    procs = [ctx.Process(target=_config4_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(r[:2] for r in res) == [(r, True) for r in range(world)]
    assert "2^22 points per GPU x 4" in res[0][3]
    # the leg's own evidence (round 4): the rank count seen by the collective, and on rank 0 the three result checks -- every rank's partial
    # against the structured identity of its slice, the gathered slots, the fold
    assert all(r[4] == world for r in res)
    checked = [r[5] for r in res if r[0] == 0][0]
    assert checked["ok"] and checked["every_rank_partial_equals_its_structured_identity"] and checked["gathered_slots_are_the_ranks_partials"] and checked["fold_equals_sum_of_gathered_partials"]


def test_bench_multi_gpu_control_flow_on_rccl_with_one_rank():
    """bench.py's N > 1 control flow -- init_process_group("nccl", device_id=...), the gloo side group, dist.barrier(), the all_gather_into_tensor
    of the 96-byte partial on device tensors inside the timed step, the device-side all_reduce(MAX) of the elapsed time, destroy_process_group --
    on RCCL itself with ONE rank (ZKHIP_BENCH_FORCE_DIST=1): everything of the multi-GPU bench path that a one-GPU box can execute.  (The
    world-size-4 rehearsal above substitutes gloo, because RCCL refuses several ranks on one device.)"""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ZKHIP_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(sk.getsockname()[1])
    run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "1", "--full", "--no-extras", "--no-cpu-baseline", "--no-general-path"],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    line = [l for l in run.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["rccl_rehearsal"] is True and rec["n_gpus"] == 1 and rec["value"] > 100.0
    assert "all_gather" in rec["config"]["parallelism"]
    # the self-verification keys of an N-rank line (round 4), here with N = 1 on RCCL
    assert rec["ranks_seen"] == 1 and rec["exchange_backend"] == "nccl" and rec["distinct_devices"] is True
    assert len(rec["devices"]) == 1 and rec["devices"][0]["rank"] == 0 and rec["devices"][0]["name"]
    assert rec["result_checked"]["ok"] and rec["result_checked"]["fold_equals_sum_of_gathered_partials"]
    assert rec["value_cold"] > 100.0

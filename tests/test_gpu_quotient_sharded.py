"""GPU (-m gpu): the quotient numerator sharded by rows (zkhip_fr_eval_rows_sharded_device).  Its output must be,
byte for byte, what the one-device composition writes -- zkhip_coeff_to_extended_device on every COEFF column, then
zkhip_fr_eval_rows_device over the extended columns -- for every device count.  The box has one card: S devices are S contexts of card 0
(ZKHIP_TEST_DUPLICATE_DEVICES, the pattern of tests/test_gpu_ntt_fanout.py), which runs the real event / peer-copy / window machinery."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import zksnap_circuits_halo2_amd as Z
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F

pytestmark = pytest.mark.gpu
R = F.R_MOD


class _Contexts:
    """zkhip_init over `ndev` contexts of card 0; restores the default single-device state on exit"""

    def __init__(self, lib, ndev):
        self.lib, self.ndev = lib, ndev

    def __enter__(self):
        self.lib.zkhip_shutdown()
        if self.ndev > 1:
            os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
        _lib.check(self.lib.zkhip_init((C.c_int * self.ndev)(*([0] * self.ndev)), self.ndev))
        assert self.lib.zkhip_device_count() == self.ndev
        return self

    def __exit__(self, *exc):
        self.lib.zkhip_shutdown()
        os.environ.pop("ZKHIP_TEST_DUPLICATE_DEVICES", None)
        _lib.check(self.lib.zkhip_init(None, 0))
        return False


def _rand(rows, g):
    t = torch.randint(0, 1 << 62, (rows, 4), dtype=torch.int64, generator=g)
    t[:, 3] &= (1 << 61) - 1
    return t.cuda()


class _Case:
    """the halo2-lib shape's quotient program with the proving key's columns EXTENDED and the proof's columns COEFF"""

    def __init__(self, k, ek, seed, gate_cols=2, coeff_only=None):
        self.k, self.ek = k, ek
        self.cs = E.halo2_lib_shape(gate_cols, 1)
        self.qc = qc = E.quotient_columns(self.cs)
        rng = random.Random(seed)
        self.ch = tuple(rng.randrange(R) for _ in range(4))
        self.prog = E.evaluate_h_program(self.cs, k, ek, *self.ch)
        self.dom = Z.EvaluationDomain(4, k)
        assert self.dom.extended_k == ek
        key = set(range(qc.fixed, qc.advice)) | {qc.l0, qc.l_last, qc.l_active_row} | set(range(qc.sigma, qc.perm_product))
        self.forms = [E.COL_EXTENDED if i in key else E.COL_COEFF for i in range(qc.total)]
        if coeff_only is not None:
            self.forms = [E.COL_COEFF if i in coeff_only else E.COL_EXTENDED for i in range(qc.total)]
        g = torch.Generator().manual_seed(seed)
        self.cols = [_rand(1 << (ek if f == E.COL_EXTENDED else k), g) for f in self.forms]

    def columns(self):
        return [(c.data_ptr(), f) for c, f in zip(self.cols, self.forms)]

    def extended(self, lib):
        """the extended columns through zkhip_coeff_to_extended_device (the composition's first half)"""
        out = []
        for c, f in zip(self.cols, self.forms):
            if f == E.COL_EXTENDED:
                out.append(c)
                continue
            e = torch.empty((1 << self.ek, 4), dtype=torch.int64, device="cuda")
            _lib.check(lib.zkhip_coeff_to_extended_device(c.data_ptr(), 1 << self.k, self.k, e.data_ptr(), 1 << self.ek, self.ek, 1,
                                                          self.dom.extended_omega.ctypes.data, self.dom.g_coset.ctypes.data, None))
            out.append(e)
        return out

    def composition(self, lib):
        ext = self.extended(lib)
        out = torch.zeros((1 << self.ek, 4), dtype=torch.int64, device="cuda")
        self.prog.run_device([t.data_ptr() for t in ext], self.ek, out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy(), [t.cpu().numpy() for t in ext]

    def sharded(self, stream=0, out=None):
        if out is None:
            out = torch.full((1 << self.ek, 4), 7, dtype=torch.int64, device="cuda")
        E.evaluate_rows_sharded_device(self.prog, self.columns(), self.k, self.ek, self.dom, out.data_ptr(), stream=stream)
        return out


@pytest.mark.parametrize("k,ek", [(3, 5), (6, 8), (10, 12), (14, 16)])
def test_sharded_is_the_composition_on_every_device_count(lib, k, ek):
    case = _Case(k, ek, 40 + k)
    with _Contexts(lib, 1):
        exp, ext = case.composition(lib)
    if ek <= 8:
        cs, qc = case.cs, case.qc
        cols = [F.fr_decode(e) for e in ext]
        sets = cs.num_permutation_sets
        ref = O.evaluate_h_direct(
            cs, k, ek, cols[qc.fixed:qc.fixed + cs.num_fixed], cols[qc.advice:qc.advice + cs.num_advice],
            cols[qc.instance:qc.instance + cs.num_instance], cols[qc.l0], cols[qc.l_last], cols[qc.l_active_row],
            cols[qc.sigma:qc.sigma + len(cs.permutation_columns)], cols[qc.perm_product:qc.perm_product + sets],
            [tuple(cols[qc.lookup + 3 * i + j] for j in range(3)) for i in range(len(cs.lookups))], *case.ch)
        assert F.fr_decode(exp) == ref
    for S in (1, 2, 3, 8):
        with _Contexts(lib, S):
            got = case.sharded()
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), exp), S


def _phases(lib):
    ms = (C.c_double * 32)()
    names = ((C.c_char * 64) * 32)()
    n = lib.zkhip_profile_read(ms, names, 32)
    return [names[i].value.decode() for i in range(n)]


def test_large_windows_take_the_compiled_executor_by_default(lib):
    """ext_k 20 over 3 devices: windows of about 349 k rows (>= 2^18) run as compiled code unless ZKHIP_VM_JIT says otherwise"""
    case = _Case(18, 20, 7)
    with _Contexts(lib, 1):
        exp, _ = case.composition(lib)
    with _Contexts(lib, 3):
        _lib.check(lib.zkhip_profile_enable(1))
        try:
            got = case.sharded()
            phases = _phases(lib)
        finally:
            lib.zkhip_profile_enable(0)
        assert np.array_equal(got.cpu().numpy(), exp)
    mode = os.environ.get("ZKHIP_VM_JIT", "1")
    assert phases == ["transform", "exchange", "rows_interpreted" if mode == "0" else "rows_compiled", "gather"], phases


def test_devices_that_own_no_column(lib):
    case = _Case(6, 8, 9, coeff_only={2, 5})
    with _Contexts(lib, 1):
        exp, _ = case.composition(lib)
    with _Contexts(lib, 8):
        got = case.sharded()
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), exp)


def test_inputs_written_on_a_side_stream_just_before_the_call(lib):
    """the COEFF columns come out of an iNTT enqueued on a non-default stream; the sharded call follows on that stream with no sync"""
    case = _Case(10, 12, 13)
    dom = case.dom
    lagrange = [c.clone() for c in case.cols]
    with _Contexts(lib, 1):
        for c, f in zip(case.cols, case.forms):
            if f == E.COL_COEFF:
                _lib.check(lib.zkhip_ifft_scaled_device(c.data_ptr(), dom.omega_inv.ctypes.data, case.k, dom.ifft_divisor.ctypes.data, None))
        exp, _ = case.composition(lib)
    with _Contexts(lib, 3):
        for c, l in zip(case.cols, lagrange):
            c.copy_(l)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        out = torch.zeros((1 << case.ek, 4), dtype=torch.int64, device="cuda")
        with torch.cuda.stream(side):
            for c, f in zip(case.cols, case.forms):
                if f == E.COL_COEFF:
                    _lib.check(lib.zkhip_ifft_scaled_device(c.data_ptr(), dom.omega_inv.ctypes.data, case.k, dom.ifft_divisor.ctypes.data, side.cuda_stream))
            case.sharded(stream=side.cuda_stream, out=out)
        side.synchronize()
        assert np.array_equal(out.cpu().numpy(), exp)


def test_back_to_back_calls_without_a_sync(lib):
    a, b = _Case(10, 12, 21), _Case(10, 12, 22)
    with _Contexts(lib, 1):
        exp_a, _ = a.composition(lib)
        exp_b, _ = b.composition(lib)
    with _Contexts(lib, 3):
        s = torch.cuda.current_stream().cuda_stream
        out_a = a.sharded(stream=s)
        out_b = b.sharded(stream=s)
        torch.cuda.synchronize()
        assert np.array_equal(out_a.cpu().numpy(), exp_a)
        assert np.array_equal(out_b.cpu().numpy(), exp_b)


def test_bad_arguments_are_rejected_and_a_correct_call_follows(lib):
    case = _Case(6, 8, 31)
    with _Contexts(lib, 1):
        exp, _ = case.composition(lib)
    with _Contexts(lib, 3):
        out = torch.zeros((1 << 8, 4), dtype=torch.int64, device="cuda")
        prog, keep = case.prog._marshal()
        n = len(case.cols)
        ptrs = (C.c_void_p * n)(*[c.data_ptr() for c in case.cols])
        forms = (C.c_uint32 * n)(*case.forms)
        om, ze = case.dom.extended_omega.ctypes.data, case.dom.g_coset.ctypes.data

        def call(prog=C.byref(prog), ptrs=ptrs, forms=forms, k=6, ek=8, om=om, ze=ze, out=out.data_ptr()):
            return lib.zkhip_fr_eval_rows_sharded_device(prog, ptrs, forms, n, k, ek, om, ze, out, None)

        assert call(prog=None) == -1
        assert call(ptrs=None) == -1
        assert call(forms=None) == -1
        assert call(om=None) == -1 and call(ze=None) == -1 and call(out=None) == -1
        assert call(forms=(C.c_uint32 * n)(*([2] + list(case.forms[1:])))) == -1
        assert call(k=9) == -1  # k > ext_k
        assert call(k=6, ek=29) == -1
        bad, keep2 = case.prog._marshal()
        bad.result_reg = 99
        assert call(prog=C.byref(bad)) == -1
        assert call() == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), exp)
        del keep, keep2


def test_one_device_calls_on_two_streams_at_once(lib):
    """S = 1 (the default single-GPU setup): two callers on two non-blocking streams, no sync between their calls -- each call's cosets
    live in its own stream's scratch, so neither can overwrite what the other's row kernel reads"""
    cases = [_Case(14, 16, 51), _Case(14, 16, 52)]
    with _Contexts(lib, 1):
        exps = [c.composition(lib)[0] for c in cases]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [torch.zeros((1 << 16, 4), dtype=torch.int64, device="cuda") for _ in cases]
        torch.cuda.synchronize()
        for _ in range(3):                                     # several rounds: the later calls run against the earlier ones
            for c, st, o in zip(cases, streams, outs):
                c.sharded(stream=st.cuda_stream, out=o)
        for st in streams:
            st.synchronize()
        for o, e in zip(outs, exps):
            assert np.array_equal(o.cpu().numpy(), e)


def test_one_device_records_the_four_phases(lib):
    case = _Case(6, 8, 61)
    with _Contexts(lib, 1):
        exp, _ = case.composition(lib)
        _lib.check(lib.zkhip_profile_enable(1))
        try:
            got = case.sharded()
            phases = _phases(lib)
        finally:
            lib.zkhip_profile_enable(0)
        assert np.array_equal(got.cpu().numpy(), exp)
    mode = os.environ.get("ZKHIP_VM_JIT", "1")
    assert phases == ["transform", "exchange", "rows_compiled" if mode == "2" else "rows_interpreted", "gather"], phases

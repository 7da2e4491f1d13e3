"""GPU (-m gpu): the sharded quotient numerator with the proving key's cosets as row-shard sets (ZKHIP_COL_ROW_SHARDS,
zkhip_fr_eval_rows_sharded_device).  Every device reads its own windows of the key where they lie; the output must still be, byte for byte,
the one-device composition (coeff_to_extended of the COEFF columns, then the whole-domain launch) for every device count and any mix of the
three column forms.  S devices are S contexts of card 0 (ZKHIP_TEST_DUPLICATE_DEVICES)."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F

pytestmark = pytest.mark.gpu
R = F.R_MOD


class _Contexts:
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
    """the halo2-lib shape's quotient program: the key's columns 2^ext_k coset values, the proof's columns COEFF"""

    def __init__(self, k, ek, seed, gate_cols=2):
        self.k, self.ek = k, ek
        self.cs = E.halo2_lib_shape(gate_cols, 1)
        qc = E.quotient_columns(self.cs)
        rng = random.Random(seed)
        self.prog = E.evaluate_h_program(self.cs, k, ek, *(rng.randrange(R) for _ in range(4)))
        self.dom = Z.EvaluationDomain(4, k)
        assert self.dom.extended_k == ek
        self.key = sorted(set(range(qc.fixed, qc.advice)) | {qc.l0, qc.l_last, qc.l_active_row} | set(range(qc.sigma, qc.perm_product)))
        g = torch.Generator().manual_seed(seed)
        self.cols = [_rand(1 << (ek if i in self.key else k), g) for i in range(qc.total)]

    def composition(self, lib):
        ext = []
        for i, c in enumerate(self.cols):
            if i in self.key:
                ext.append(c)
                continue
            e = torch.empty((1 << self.ek, 4), dtype=torch.int64, device="cuda")
            _lib.check(lib.zkhip_coeff_to_extended_device(c.data_ptr(), 1 << self.k, self.k, e.data_ptr(), 1 << self.ek, self.ek, 1,
                                                          self.dom.extended_omega.ctypes.data, self.dom.g_coset.ctypes.data, None))
            ext.append(e)
        out = torch.zeros((1 << self.ek, 4), dtype=torch.int64, device="cuda")
        self.prog.run_device([t.data_ptr() for t in ext], self.ek, out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def shards(self, extra=(0, 0), stream=0):
        """the key's columns scattered into one set (column order = self.key), halos = the program's + extra"""
        lo, hi = self.prog.halos(self.ek)
        rs = E.RowShards(self.ek, len(self.key), lo + extra[0], hi + extra[1])
        for c, i in enumerate(self.key):
            rs.scatter_device(c, self.cols[i].data_ptr(), stream)
        return rs

    def columns(self, rs, extended=()):
        """key columns as ZKHIP_COL_ROW_SHARDS (those in `extended` as ZKHIP_COL_EXTENDED), the others COEFF"""
        out = []
        for i, c in enumerate(self.cols):
            if i in extended:
                out.append((c.data_ptr(), E.COL_EXTENDED))
            elif i in self.key:
                out.append((rs.ref(self.key.index(i)), E.COL_ROW_SHARDS))
            else:
                out.append((c.data_ptr(), E.COL_COEFF))
        return out

    def run(self, columns, stream=0, out=None):
        if out is None:
            out = torch.full((1 << self.ek, 4), 7, dtype=torch.int64, device="cuda")
        E.evaluate_rows_sharded_device(self.prog, columns, self.k, self.ek, self.dom, out.data_ptr(), stream=stream)
        return out


@pytest.mark.parametrize("k,ek", [(3, 5), (6, 8), (10, 12), (14, 16)])
def test_row_shard_key_is_the_composition_on_every_device_count(lib, k, ek):
    case = _Case(k, ek, 70 + k)
    with _Contexts(lib, 1):
        exp = case.composition(lib)
    for S in (1, 2, 3, 8):
        with _Contexts(lib, S):
            with case.shards(extra=(3, 1)) as rs:                 # wider halos than the program's: the windows are read at an offset
                got = case.run(case.columns(rs))
                torch.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy(), exp), S
                mixed = case.run(case.columns(rs, extended=set(case.key[::2])))   # every form at once
                torch.cuda.synchronize()
                assert np.array_equal(mixed.cpu().numpy(), exp), S


def test_narrow_halos_and_raw_pointers_are_rejected_and_a_correct_call_follows(lib):
    case = _Case(6, 8, 33)
    with _Contexts(lib, 1):
        exp = case.composition(lib)
    lo, hi = case.prog.halos(8)
    assert lo > 0 and hi > 0
    for S in (1, 3):
        with _Contexts(lib, S):
            out = torch.zeros((1 << 8, 4), dtype=torch.int64, device="cuda")
            p, keep = case.prog._marshal()

            def call(columns, ek=8):
                ptrs = (C.c_void_p * len(columns))(*[c[0] for c in columns])
                forms = (C.c_uint32 * len(columns))(*[c[1] for c in columns])
                return lib.zkhip_fr_eval_rows_sharded_device(C.byref(p), ptrs, forms, len(columns), 6, ek, case.dom.extended_omega.ctypes.data,
                                                             case.dom.g_coset.ctypes.data, out.data_ptr(), None)

            for extra in ((-1, 0), (0, -1)):
                with case.shards(extra=extra) as narrow:
                    assert call(case.columns(narrow)) == -1 and b"halo" in lib.zkhip_last_error()
            with case.shards() as rs:
                cols = case.columns(rs)
                raw = [(case.cols[case.key[0]].data_ptr(), E.COL_ROW_SHARDS) if i == case.key[0] else c for i, c in enumerate(cols)]
                assert call(raw) == -1                                                    # a device address with form 2
                assert call(cols, ek=9) == -1                                             # the set's ext_k differs from the call's
                assert call(cols) == 0
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), exp)
            del keep


def test_back_to_back_calls_and_a_key_written_on_a_side_stream(lib):
    a, b = _Case(10, 12, 41), _Case(10, 12, 42)
    with _Contexts(lib, 1):
        exp_a, exp_b = a.composition(lib), b.composition(lib)
    with _Contexts(lib, 3):
        side = torch.cuda.Stream()
        s = side.cuda_stream
        with torch.cuda.stream(side):
            rs_a, rs_b = a.shards(stream=s), b.shards(stream=s)                 # the sets are written on `side` ...
            out_a = a.run(a.columns(rs_a), stream=s)                             # ... and read on it, no host sync between
            out_b = b.run(b.columns(rs_b), stream=s)
        side.synchronize()
        assert np.array_equal(out_a.cpu().numpy(), exp_a)
        assert np.array_equal(out_b.cpu().numpy(), exp_b)
        rs_a.destroy()
        rs_b.destroy()


def _phases(lib):
    ms = (C.c_double * 32)()
    names = ((C.c_char * 64) * 32)()
    n = lib.zkhip_profile_read(ms, names, 32)
    return [names[i].value.decode() for i in range(n)]


@pytest.mark.parametrize("S", [1, 3])
def test_profile_phases_and_the_compiled_executor_on_large_windows(lib, S):
    """ext_k 20: windows of >= 2^18 rows run as compiled code unless ZKHIP_VM_JIT says otherwise; the four phases are recorded"""
    case = _Case(18, 20, 8)
    with _Contexts(lib, 1):
        exp = case.composition(lib)
    with _Contexts(lib, S):
        with case.shards() as rs:
            torch.cuda.synchronize()
            _lib.check(lib.zkhip_profile_enable(1))
            try:
                got = case.run(case.columns(rs))
                phases = _phases(lib)
            finally:
                lib.zkhip_profile_enable(0)
            assert np.array_equal(got.cpu().numpy(), exp)
    mode = os.environ.get("ZKHIP_VM_JIT", "1")
    assert phases == ["transform", "exchange", "rows_interpreted" if mode == "0" else "rows_compiled", "gather"], phases

"""GPU (-m gpu): the device-resident proving key with its extended cosets as a row-shard set (keygen_device(..., row_shards=True),
DeviceProvingKey.from_host(..., row_shards=True)) and the proof flow that reads them where they lie (prove_flow.run(sharded_key=True)).
Gathered back, the key must be the default key byte for byte, and the proof must give the default run's quotient commitments.  Several
devices are contexts of card 0 (ZKHIP_TEST_DUPLICATE_DEVICES)."""
import ctypes as C
import io
import os
import random

import numpy as np
import pytest

import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F, keygen as KG

pytestmark = pytest.mark.gpu
R = F.R_MOD


def _on_contexts(lib, S, fn):
    lib.zkhip_shutdown()
    if S > 1:
        os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
    try:
        _lib.check(lib.zkhip_init((C.c_int * S)(*([0] * S)), S))
        return fn()
    finally:
        lib.zkhip_shutdown()
        os.environ.pop("ZKHIP_TEST_DUPLICATE_DEVICES", None)
        _lib.check(lib.zkhip_init(None, 0))


def _circuit(k, seed):
    """three fixed columns, two advice, a gate reading rotations -1 / +1 and a permutation of two sets (its -(blinding + 1) rotation)"""
    rng = random.Random(seed)
    n = 1 << k
    gates = [[E.Fixed(0) * (E.Advice(0, -1) + E.Advice(1, 1) - E.Advice(0))]]
    perm = [("advice", 0), ("advice", 1), ("fixed", 1), ("fixed", 2)]
    cs = E.ConstraintSystem(num_fixed=3, num_advice=2, gates=gates, permutation_columns=perm, blinding_factors=4, degree=4)
    fixed = [F.fr_encode([rng.randrange(R) for _ in range(n)]) for _ in range(3)]
    asm = KG.Assembly(n, len(perm))
    for _ in range(12):
        asm.copy(rng.randrange(len(perm)), rng.randrange(n - 5), rng.randrange(len(perm)), rng.randrange(n - 5))
    return cs, fixed, asm


def _key_bytes(pk):
    buf = io.BytesIO()
    pk.write(buf, KG.RAW_BYTES)
    return buf.getvalue()


@pytest.mark.parametrize("S", [1, 3])
def test_row_shard_keygen_writes_the_default_key(lib, S):
    k = 7
    cs, fixed, asm = _circuit(k, 5 + S)
    with Z.ParamsKZG.setup(k, 0xBEEF) as params:
        with KG.keygen_device(params, cs, fixed, asm) as dpk:
            ref = _key_bytes(dpk.to_host())

    def sharded():                                        # the SRS is registered again under the new device list (same seed)
        with Z.ParamsKZG.setup(k, 0xBEEF) as params, KG.keygen_device(params, cs, fixed, asm, row_shards=True) as spk:
            assert spk.row_shards and spk.shards.n_cols == 3 + 3 + 4
            assert (spk.shards.halo_lo, spk.shards.halo_hi) == E.quotient_halos(cs, k, spk.shards.ext_k)
            host = spk.to_host()
            got = _key_bytes(host)
            with KG.DeviceProvingKey.from_host(host, cs, row_shards=True) as back:       # straight from host memory into the windows
                again = _key_bytes(back.to_host())
            return got, again
    got, again = _on_contexts(lib, S, sharded)
    assert got == ref
    assert again == ref


def test_sharded_key_proof_matches_the_default_run(lib):
    from tools import prove_flow

    default = prove_flow.run(10, 3, seed=17, verbose=False)
    assert all(default["checks"].values()), default["checks"]
    sharded = _on_contexts(lib, 3, lambda: prove_flow.run(10, 3, seed=17, sharded_quotient=True, sharded_key=True, verbose=False))
    assert all(sharded["checks"].values()), sharded["checks"]
    assert sharded["h_commitments"] == default["h_commitments"]
    with pytest.raises(ValueError):
        prove_flow.run(10, 3, seed=17, sharded_key=True, verbose=False)


def test_sharded_key_catches_a_broken_gate(lib):
    from tools import prove_flow

    bad = _on_contexts(lib, 3, lambda: prove_flow.run(10, 3, seed=17, corrupt="gate", sharded_quotient=True, sharded_key=True, verbose=False))
    assert not bad["checks"]["quotient_is_a_polynomial"]

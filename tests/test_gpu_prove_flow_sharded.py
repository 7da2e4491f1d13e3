"""GPU (-m gpu): tools/prove_flow.py with the quotient numerator sharded by rows (sharded_quotient=True: the proving key's cosets go in
EXTENDED, the proof's columns COEFF, zkhip_fr_eval_rows_sharded_device transforms and evaluates) over three contexts of card 0.  The proof's
checks must hold and the quotient's commitments must be those of the default one-device run with the same seed."""
import ctypes as C
import os

import pytest

from zksnap_circuits_halo2_amd import _lib

pytestmark = pytest.mark.gpu


def _on_three_contexts(lib, fn):
    lib.zkhip_shutdown()
    os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"
    try:
        _lib.check(lib.zkhip_init((C.c_int * 3)(0, 0, 0), 3))
        return fn()
    finally:
        lib.zkhip_shutdown()
        os.environ.pop("ZKHIP_TEST_DUPLICATE_DEVICES", None)
        _lib.check(lib.zkhip_init(None, 0))


def test_sharded_quotient_proof_matches_the_default_run(lib):
    from tools import prove_flow

    default = prove_flow.run(10, 3, seed=17, verbose=False)
    assert all(default["checks"].values()), default["checks"]
    sharded = _on_three_contexts(lib, lambda: prove_flow.run(10, 3, seed=17, sharded_quotient=True, verbose=False))
    assert all(sharded["checks"].values()), sharded["checks"]
    assert sharded["h_commitments"] == default["h_commitments"]
    assert len(sharded["h_commitments"]) == 3


def test_sharded_quotient_of_a_broken_gate_is_not_a_polynomial(lib):
    from tools import prove_flow

    bad = _on_three_contexts(lib, lambda: prove_flow.run(10, 3, seed=17, corrupt="gate", sharded_quotient=True, verbose=False))
    assert not bad["checks"]["quotient_is_a_polynomial"]

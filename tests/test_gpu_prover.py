"""GPU (-m gpu): the package's prover (zksnap_circuits_halo2_amd/prover.py) on its own -- `create_proof` without laps, so that nothing waits
for the device between phases, against the timed flow of tools/prove_flow.py, whose every phase ends in a synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import keygen as KG, prover as P, verifier as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_proof_without_laps_writes_the_bytes_of_the_timed_flow():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_flow

    k, gate_cols, lookups, seed = 7, 3, 2, 1
    timed = prove_flow.run(k, gate_cols, lookups=lookups, verbose=False, transcript=True)
    # the same inputs as the flow's defaults: torch's generator and the test SRS's trapdoor from the seed, blinding rows from torch
    torch.manual_seed(seed)
    with Z.ParamsKZG.setup(k, P.SeededChallenges(seed).s) as params:
        blinding = P.TorchBlinding()
        w = P.halo2_lib_witness(k, gate_cols, lookups, blinding)
        with KG.keygen_device(params, w.cs, [f.cpu().numpy().view(np.uint64).reshape(-1, 4) for f in w.fixed], w.assembly) as dpk:
            pv = P.create_proof(params, dpk, w, P.TranscriptChallenges(dpk.vk), blinding, lap=None)
            proof, plan = pv.proof, pv.plan
            assert pv.permutation_closes and pv.lookup_closes and pv.multiopen_ok
            del pv
            assert type(proof) is bytes and proof == timed["proof"]
            assert plan == timed["proof_plan"]
            assert V.verify_transcript_proof(params, dpk.vk, k, proof, timed["proof_shape"], plan) is True
            flipped = proof[:-1] + bytes([proof[-1] ^ 1])
            try:
                assert V.verify_transcript_proof(params, dpk.vk, k, flipped, timed["proof_shape"], plan) is False
            except Z._lib.ZkhipError as e:                                  # H' no longer decodes
                assert e.code == -1

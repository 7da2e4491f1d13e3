"""GPU (-m gpu): public inputs through the flow at k = 7 -- tools/prove_flow.run(7, 3, lookups=2, instances=1, instance_len=5, ...): the mock step,
the prover (the values absorbed behind the key, the instance column carried through the permutation argument and the quotient, never committed
or opened) and the verifier (the values absorbed again, the column evaluated at x on the device inside the identity call).

  1  the honest flow with a transcript: every check passes and the identity's status is 0; the same proof against one changed public value is
     refused; the identity alone, on the honest head's evaluations and challenges, says 1 for the changed value (a changed value also changes
     every challenge: this is the check that isolates the identity)
  2  corrupt="instance": the mock step locates the broken copy; the proof is refused while its openings alone accept
  3  five proofs of one key over different public inputs in one call, two of them handed the wrong inputs
  4  the seeded flow with an instance column verifies; a key with instance columns and no public inputs is a ValueError
  5  instances=0 writes the bytes a run without the keyword writes"""
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

import instance_reference as NR
import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import fields as F, keygen as KG, prover as P, verifier as V
from zksnap_circuits_halo2_amd.transcript import transcript_classes, vk_transcript_repr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = F.R_MOD
K, G, NL, LEN = 7, 3, 2, 5


@pytest.fixture(scope="module")
def flow():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_flow

    return prove_flow


def read_head(vk, proof, shape, plan, instances):
    vk_io = io.BytesIO()
    vk.write(vk_io, KG.RAW_BYTES)
    with transcript_classes("blake2b")[1](bytes(proof)) as r:
        return V._read_proof_head(r, vk_transcript_repr(vk_io.getvalue()), shape, plan, instances=instances)


def changed(instances, column=0, row=2):
    out = [list(c) for c in instances]
    out[column][row] = (out[column][row] + 1) % R
    return out


def observed(flow, **how):
    """run(K, G, lookups=NL, transcript=True, verify=True, **how) with the verifier watched while the parameters and the key are alive"""
    seen, real = {}, flow.verify_transcript_proof

    def spy(params, vk, k, proof, shape, plan, *rest, instances=None):
        seen["instances"] = instances
        seen["verdict"] = real(params, vk, k, proof, shape, plan, *rest, instances=instances)
        wrong = changed(instances)
        seen["verdict_wrong_inputs"] = real(params, vk, k, proof, shape, plan, *rest, instances=wrong)
        seen["openings_alone"] = V.verify_transcript_proofs(params, vk, k, [proof], shape, plan, identity=False, instances=[instances])[0]
        _, challenges, evals = read_head(vk, proof, shape, plan, instances)
        seen.update(cs=vk.cs, plan=list(plan), challenges=challenges, evals=evals)
        seen["status"] = int(V.identity_statuses(vk, k, plan, [evals], [challenges], [instances])[0])
        seen["status_wrong_inputs"] = int(V.identity_statuses(vk, k, plan, [evals], [challenges], [wrong])[0])
        seen["reference_wrong_inputs"] = NR.identity_value(vk.cs, plan, k, evals, challenges, wrong)
        with pytest.raises(ValueError, match="instance columns"):
            V.verify_transcript_proofs(params, vk, k, [proof], shape, plan)
        with pytest.raises(ValueError, match="instance columns"):
            V.identity_statuses(vk, k, plan, [evals], [challenges])
        return seen["verdict"]

    flow.verify_transcript_proof = spy
    try:
        res = flow.run(K, G, lookups=NL, verbose=False, transcript=True, verify=True, instances=1, instance_len=LEN, **how)
    finally:
        flow.verify_transcript_proof = real
    return res, seen


def test_the_honest_flow_verifies_against_its_public_inputs_and_against_no_others(flow):
    res, seen = observed(flow, mock=True)
    assert all(res["checks"].values()) and res["checks"]["proof_verifies"] is True and seen["verdict"] is True
    assert res["instances"] == seen["instances"] and [len(c) for c in res["instances"]] == [LEN] and len(set(res["instances"][0])) == LEN
    assert seen["cs"].num_instance == 1 and seen["cs"].permutation_columns[-1] == ("instance", 0)
    assert not any(kind == "instance" for kind, _, _ in seen["plan"])                 # never opened
    assert seen["status"] == 0 and NR.identity_value(seen["cs"], seen["plan"], K, seen["evals"], seen["challenges"], seen["instances"]) == 0
    assert seen["verdict_wrong_inputs"] is False
    assert seen["status_wrong_inputs"] == 1 and seen["reference_wrong_inputs"] != 0   # the identity alone, challenges unchanged


def test_a_broken_public_copy_is_located_by_the_mock_and_refused_by_the_identity(flow):
    with pytest.raises(AssertionError, match="copy"):
        flow.run(K, G, lookups=NL, verbose=False, transcript=True, verify=True, mock=True, instances=1, instance_len=LEN, corrupt="instance")
    res, seen = observed(flow, corrupt="instance")
    checks = res["checks"]
    assert checks["proof_verifies"] is False and seen["verdict"] is False and checks["permutation_product_closes"] is False
    assert checks["multiopen_linearisation_vanishes"] is True
    assert seen["openings_alone"] is True, "the openings are consistent: it is the identity that refuses the proof"
    assert seen["status"] == 1


def test_five_proofs_of_one_key_over_different_public_inputs_in_one_call():
    proofs, publics, fixed, plan = [], [], None, None
    rng = random.Random("public-inputs")
    with Z.ParamsKZG.setup(K, P.SeededChallenges(1).s) as params:
        dpk = None
        try:
            for seed in range(1, 6):
                torch.manual_seed(1)                                               # one circuit: the constants column is drawn from torch's generator
                blinding = P.DeviceBlinding(random.Random(seed).randbytes(32))
                w = P.halo2_lib_witness(K, G, NL, blinding, instances=1, instance_len=LEN, public_inputs=[[rng.randrange(R) for _ in range(LEN)]])
                if dpk is None:
                    fixed = [f.clone() for f in w.fixed]
                    dpk = KG.keygen_device(params, w.cs, [f.cpu().numpy().view(np.uint64).reshape(-1, 4) for f in w.fixed], w.assembly)
                assert all(torch.equal(a, b) for a, b in zip(fixed, w.fixed))
                pv = P.create_proof(params, dpk, w, P.TranscriptChallenges(dpk.vk), blinding, lap=None)
                proofs.append(pv.proof)
                publics.append([list(c) for c in w.instance_values])
                plan = pv.plan
                del pv, w
            assert len({tuple(p[0]) for p in publics}) == 5
            shape = {"advice": G + NL, "lookups": NL, "permutation_sets": dpk.vk.cs.num_permutation_sets, "random_poly": True}
            handed = [publics[0], publics[3], publics[2], changed(publics[3], row=LEN - 1), publics[4]]      # another proof's inputs; one value off
            assert V.verify_transcript_proofs(params, dpk.vk, K, proofs, shape, plan, instances=handed) == [True, False, True, False, True]
            assert V.verify_transcript_proofs(params, dpk.vk, K, proofs, shape, plan, instances=publics) == [True] * 5
            assert V.verify_transcript_proof(params, dpk.vk, K, proofs[1], shape, plan, instances=publics[1]) is True
            with pytest.raises(ValueError, match="same lengths"):
                V.verify_transcript_proofs(params, dpk.vk, K, proofs[:2], shape, plan, instances=[publics[0], [publics[1][0][:-1]]])
        finally:
            if dpk is not None:
                dpk.free()


def test_the_seeded_flow_with_an_instance_column_verifies(flow):
    good = flow.run(K, G, lookups=NL, verbose=False, verify=True, mock=True, instances=1, instance_len=LEN)
    assert all(good["checks"].values()) and good["checks"]["proof_verifies"] is True and len(good["instances"][0]) == LEN
    bad = flow.run(K, G, lookups=NL, verbose=False, verify=True, instances=1, instance_len=LEN, corrupt="instance")["checks"]
    assert bad["proof_verifies"] is False and bad["multiopen_linearisation_vanishes"] is True


def test_without_instance_columns_the_proof_bytes_are_unchanged(flow):
    plain = flow.run(K, G, lookups=NL, verbose=False, transcript=True, verify=True, device_randomness=True)
    keyword = flow.run(K, G, lookups=NL, verbose=False, transcript=True, verify=True, device_randomness=True, instances=0, instance_len=LEN)
    assert plain["proof"] == keyword["proof"] and plain["checks"] == keyword["checks"] and all(plain["checks"].values())
    assert "instances" not in keyword and plain["columns"] == keyword["columns"]
    public = flow.run(K, G, lookups=NL, verbose=False, transcript=True, verify=True, device_randomness=True, instances=1, instance_len=LEN)
    assert public["proof"] != plain["proof"] and all(public["checks"].values())
    assert not any(kind == "instance" for kind, _, _ in public["proof_plan"])          # the column is neither committed nor opened
    assert public["proof_shape"]["advice"] == plain["proof_shape"]["advice"]

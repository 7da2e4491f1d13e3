"""GPU (-m gpu): the quotient identity at x -- `zkhip_fr_domain_points_device`, `zkhip_verify_identity_device` and the verifiers built on them
(verifier.verify_transcript_proofs, tools/prove_flow.py) -- against tests/identity_reference.py, which evaluates the identity on Python integers
from the ConstraintSystem directly.

  1  the domain values at 1, 63, 64, 65 and 257 points, the edge points of the host check among them
  2  synthetic records (no prover): random evaluations and challenges with h_0 solved so that the record is accepted, some perturbed (status 1),
     some with x in the domain (status 2); batches of 1, 15, 16, 17 (either side of the transpose's tile), 63, 64, 65, 257; every status and the
     report against the reference; a batch where all pass and one where only the last record fails
  3  an honest transcript proof of the flow at (7, 3, 2) and (7, 1, 1): the reference identity holds on the proof's own evaluations (this pins the
     restatement against the prover's independent extended-coset quotient) and the device says 0
  4  soundness: the flow over a witness broken with corrupt="gate" / "copy" does not verify, with a transcript and seeded, while the openings alone
     still accept -- the identity is what refused it
  5  five proofs of one key in one call, two of them of broken witnesses; a truncated proof rejects that proof alone
  6  the voter's shape (13, 256, 8): an honest proof verifies, the same proof with one evaluation's bytes swapped for another's is refused by the
     identity call"""
import functools
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

import identity_reference as IR
import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import evaluation as E, fields as F, keygen as KG, multiopen as MO, prover as P, verifier as V
from zksnap_circuits_halo2_amd.transcript import transcript_classes, vk_transcript_repr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = F.R_MOD
NONE = (1 << 64) - 1
DEV = torch.device("cuda", 0)


def words(values, *shape):
    if not values:
        return torch.zeros(shape + (4,), dtype=torch.int64, device=DEV)
    return torch.from_numpy(F.fr_encode(values).view(np.int64).reshape(*shape, 4)).to(DEV)


# ---- 1: the domain values ------------------------------------------------------------------------------------------------------------------------
DOMAINS = [(1, 1), (3, 2), (7, 122), (7, 64), (13, (1 << 13) - 6), (28, (1 << 28) - 1), (28, (1 << 28) - 6)]      # (7, 64): the longest tail the call takes


@functools.lru_cache(None)
def domain_points(k, u):
    """257 points: the edge points of the host check first, then seeded random ones and powers of omega"""
    n, w, rng = 1 << k, F.omega_for(k), random.Random(f"points-{k}-{u}")
    points = [0, 1, w, pow(w, u, R), pow(w, n - 1, R), 2, R - 1, pow(w, (u + 1) % n, R)]
    while len(points) < 257:
        points.append(pow(w, rng.randrange(n), R) if len(points) % 16 == 9 else rng.randrange(R))
    return points


@functools.lru_cache(None)
def domain_reference(k, u, x):
    return IR.device_domain_values(x, k, u)


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 257])
def test_domain_values_agree_with_the_reference(n_points):
    for k, u in DOMAINS:
        if n_points > 65 and (1 << k) - u > 8:
            continue                                                               # the long-tail reference is computed for 65 points, not 257
        points = domain_points(k, u)[:n_points] if n_points > 1 else [domain_points(k, u)[5 + k % 3]]
        got = E.domain_points_device(k, u, words(points, len(points)))
        got = F.fr_decode(got.cpu().numpy().view(np.uint64).reshape(-1, 4))
        want = [domain_reference(k, u, x) for x in points]
        for j in range(4):
            assert got[j * len(points):(j + 1) * len(points)] == [w_[j] for w_ in want], (k, u, j)
        if n_points >= 63:
            assert sum(1 for w_, x in zip(want, points) if w_ == (0, 0, 0, 0) and x) >= 5      # points of the domain are among them


# ---- 2: synthetic records ------------------------------------------------------------------------------------------------------------------------
K = 7
U = (1 << K) - 6


@functools.lru_cache(None)
def synthetic(gate_cols, lookups):
    """(cs, plan, program, 257 records (evals, challenges), their reference statuses): record i is accepted, but i % 7 == 3 has one evaluation
    perturbed and i % 11 == 5 has x = omega^j"""
    cs = E.halo2_lib_shape(gate_cols, lookups)
    plan = P.opening_plan(cs, gate_cols, lookups, U, True, "halo2")
    rng = random.Random(f"records-{gate_cols}-{lookups}")
    used = [i for i, t in enumerate(plan) if t[0] != "random"]
    records = []
    for i in range(257):
        evals, challenges = [rng.randrange(R) for _ in plan], [rng.randrange(R) for _ in range(5)]
        if i % 11 == 5:
            challenges[4] = pow(F.omega_for(K), rng.randrange(1 << K), R)
        else:
            evals = IR.solve_h0(cs, plan, K, evals, tuple(challenges))
            if i % 7 == 3:
                at = rng.choice(used)
                evals[at] = (evals[at] + 1 + rng.randrange(R - 1)) % R
        records.append((evals, tuple(challenges)))
    statuses = [IR.status(cs, plan, K, e, c) for e, c in records]
    return cs, plan, E.identity_program(cs, plan, K)._marshal(), records, statuses


def run_records(prog, plan, records):
    evals = words([e for rec in records for e in rec[0]], len(records), len(plan))
    challenges = words([c for rec in records for c in rec[1]], len(records), 5)
    status, report = E.verify_identity_device(prog, evals, challenges, K, U)
    return [int(s) for s in status], report


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 63, 64, 65, 257])
@pytest.mark.parametrize("gate_cols, lookups", [(1, 1), (3, 2)])
def test_synthetic_records_get_the_reference_status_and_report(gate_cols, lookups, batch):
    cs, plan, prog, records, statuses = synthetic(gate_cols, lookups)
    got, report = run_records(prog, plan, records[:batch])
    assert got == statuses[:batch]
    assert report == IR.report(statuses[:batch])
    if batch >= 17:
        assert set(got) == {0, 1, 2}
    else:
        assert got[0] == 0


@pytest.mark.parametrize("gate_cols, lookups", [(1, 1), (3, 2)])
def test_a_batch_that_passes_and_a_batch_whose_last_record_fails(gate_cols, lookups):
    cs, plan, prog, records, statuses = synthetic(gate_cols, lookups)
    good = [rec for rec, s in zip(records, statuses) if s == 0][:65]
    bad = next(rec for rec, s in zip(records, statuses) if s == 1)
    assert len(good) == 65
    assert run_records(prog, plan, good) == ([0] * 65, (0, NONE))
    assert run_records(prog, plan, good[:64] + [bad]) == ([0] * 64 + [1], (1, 64))
    assert run_records(prog, plan, [bad] + good[:16]) == ([1] + [0] * 16, (1, 0))
    assert run_records(prog, plan, []) == ([], (0, NONE))


# ---- 3, 4, 6: proofs of the flow -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flow():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_flow

    return prove_flow


def read_head(vk, proof, shape, plan):
    vk_io = io.BytesIO()
    vk.write(vk_io, KG.RAW_BYTES)
    with transcript_classes("blake2b")[1](bytes(proof)) as r:
        return V._read_proof_head(r, vk_transcript_repr(vk_io.getvalue()), shape, plan)


_OBSERVED = {}


def observed(flow, gate_cols, lookups, k=7, inside=None, **how):
    """run(k, gate_cols, lookups=lookups, transcript=True, verify=True, **how) once per argument set, with the verifier watched: (result, what was
    seen while the parameters and the key were alive -- the verdict, the openings' verdict alone, the proof's evaluations and challenges, the
    device's status of the identity; `inside(params, vk, k, proof, shape, plan)` may add to it)"""
    key = (gate_cols, lookups, k, tuple(sorted(how.items())))
    if key in _OBSERVED:
        return _OBSERVED[key]
    seen, real = {}, flow.verify_transcript_proof

    def spy(params, vk, k_, proof, shape, plan):
        seen["verdict"] = real(params, vk, k_, proof, shape, plan)
        seen["openings_alone"] = V.verify_transcript_proofs(params, vk, k_, [proof], shape, plan, identity=False)[0]
        _, challenges, evals = read_head(vk, proof, shape, plan)
        seen.update(cs=vk.cs, plan=list(plan), challenges=challenges, evals=evals, status=int(V.identity_statuses(vk, k_, plan, [evals], [challenges])[0]))
        if inside is not None:
            seen["inside"] = inside(params, vk, k_, proof, shape, plan)
        return seen["verdict"]

    flow.verify_transcript_proof = spy
    try:
        res = flow.run(k, gate_cols, lookups=lookups, verbose=False, transcript=True, verify=True, **how)
    finally:
        flow.verify_transcript_proof = real
    _OBSERVED[key] = (res, seen)
    return res, seen


@pytest.mark.parametrize("gate_cols, lookups", [(3, 2), (1, 1)])
def test_the_identity_holds_on_an_honest_proof_of_the_flow(flow, gate_cols, lookups):
    res, seen = observed(flow, gate_cols, lookups)
    assert all(res["checks"].values()) and seen["verdict"] is True
    assert IR.identity_value(seen["cs"], seen["plan"], 7, seen["evals"], seen["challenges"]) == 0
    assert seen["status"] == 0


@pytest.mark.parametrize("corrupt", ["gate", "copy"])
def test_a_proof_of_a_broken_witness_does_not_verify(flow, corrupt):
    res, seen = observed(flow, 3, 2, corrupt=corrupt)
    checks = res["checks"]
    assert checks["proof_verifies"] is False and checks["quotient_is_a_polynomial"] is False
    assert checks["multiopen_linearisation_vanishes"] is True
    assert seen["openings_alone"] is True, "the openings are consistent: it is the identity that refuses the proof"
    assert seen["status"] == 1 and IR.identity_value(seen["cs"], seen["plan"], 7, seen["evals"], seen["challenges"]) != 0


def test_the_seeded_flow_refuses_a_broken_witness_too(flow):
    openings = []

    def on_proof(params, k, queries, vqueries, commit, proof, challenges):
        openings.append(MO.VerifierSHPLONK(params).verify_proof(vqueries, proof[0], proof[1], *challenges))

    bad = flow.run(7, 3, lookups=2, verbose=False, verify=True, corrupt="gate", on_proof=on_proof)["checks"]
    assert bad["proof_verifies"] is False and bad["multiopen_linearisation_vanishes"] is True and openings == [True]
    good = flow.run(7, 3, lookups=2, verbose=False, verify=True)["checks"]
    assert good["proof_verifies"] is True and all(good.values())


def test_five_proofs_of_one_key_in_one_call():
    k, gate_cols, lookups = 7, 3, 2
    proofs, fixed, plan = [], None, None
    with Z.ParamsKZG.setup(k, P.SeededChallenges(1).s) as params:
        dpk = None
        try:
            for seed in range(1, 6):
                torch.manual_seed(1)                                               # one circuit: the constants column is drawn from torch's generator
                blinding = P.DeviceBlinding(random.Random(seed).randbytes(32))    # ... and five proofs: blinding rows and the random polynomial differ
                w = P.halo2_lib_witness(k, gate_cols, lookups, blinding, corrupt="gate" if seed in (2, 4) else None)
                if dpk is None:
                    fixed = [f.clone() for f in w.fixed]
                    dpk = KG.keygen_device(params, w.cs, [f.cpu().numpy().view(np.uint64).reshape(-1, 4) for f in w.fixed], w.assembly)
                assert all(torch.equal(a, b) for a, b in zip(fixed, w.fixed))
                pv = P.create_proof(params, dpk, w, P.TranscriptChallenges(dpk.vk), blinding, lap=None)
                proofs.append(pv.proof)
                plan = pv.plan
                del pv, w
            assert len(set(proofs)) == 5
            shape = {"advice": gate_cols + lookups, "lookups": lookups, "permutation_sets": dpk.vk.cs.num_permutation_sets, "random_poly": True}
            verify = lambda batch, **kw: V.verify_transcript_proofs(params, dpk.vk, k, batch, shape, plan, **kw)
            assert verify(proofs) == [True, False, True, False, True]
            assert verify(proofs, identity=False) == [True] * 5                    # the openings alone accept all five
            cut = list(proofs)
            cut[2] = cut[2][:-40]                                                  # the multi-open's last point is incomplete
            cut[4] = cut[4][:200]                                                  # ... and this one ends among its commitments
            assert verify(cut) == [True, False, False, False, False]
            assert verify([]) == []
            assert V.verify_transcript_proof(params, dpk.vk, k, proofs[0], shape, plan) is True
            assert V.verify_transcript_proof(params, dpk.vk, k, proofs[1], shape, plan) is False
        finally:
            if dpk is not None:
                dpk.free()


def test_the_voters_shape_verifies_and_a_swapped_evaluation_is_refused(flow):
    def inside(params, vk, k, proof, shape, plan):
        first = 32 * (shape["advice"] + 3 * shape["lookups"] + shape["permutation_sets"] + int(shape["random_poly"]) + 3)      # the evaluations follow the commitments
        a, b = plan.index(("advice", 200, 1)), plan.index(("advice", 17, 2))
        ea, eb = proof[first + 32 * a:first + 32 * a + 32], proof[first + 32 * b:first + 32 * b + 32]
        assert ea != eb
        swapped = bytearray(proof)
        swapped[first + 32 * a:first + 32 * a + 32], swapped[first + 32 * b:first + 32 * b + 32] = eb, ea
        _, challenges, evals = read_head(vk, bytes(swapped), shape, plan)
        return len(plan), int(V.identity_statuses(vk, k, plan, [evals], [challenges])[0]), V.verify_transcript_proof(params, vk, k, bytes(swapped), shape, plan)

    res, seen = observed(flow, 256, 8, k=13, inside=inside)
    assert all(res["checks"].values()) and seen["verdict"] is True and seen["status"] == 0
    n_evals, status, verdict = seen["inside"]
    assert n_evals > 1800 and status == 1 and verdict is False
    assert IR.identity_value(seen["cs"], seen["plan"], 13, seen["evals"], seen["challenges"]) == 0

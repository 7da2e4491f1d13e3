#!/usr/bin/env python3
"""A `create_proof` (seeded challenges; with `transcript=True` a Blake2b transcript and a proof as bytes) for a *satisfied* circuit of the halo2-lib shape, device-resident from witness columns to
quotient commitments -- the steps of [DEP] halo2-axiom plonk/prover.rs in the order the reference's prover runs them
(/root/reference/aggregator/src/wrapper.rs:129).  This file is the driver: the witness, the phases, the challenge and blinding sources, the
opening plan are zksnap_circuits_halo2_amd/prover.py, the verifier of proof bytes is verifier.py; here are the arguments, the lap clock, the mock step,
keygen (or the key-file round trip), the corrupt_proof edits, the verify step, the invariants and the result.

  SRS (ParamsKZG.setup, known trapdoor) -> advice commitments (Lagrange basis) -> permutation and lookup arguments (row programs,
  permute_expression_pair, grand products) -> Lagrange -> coefficients (batched iNTT) -> commitments -> extended coset (batched NTT)
  -> fused quotient program -> / (X^n - 1) -> inverse extended transform -> h commitments -> evaluations at x.

Circuit: `gate_cols` advice columns with the vertical gate q (a + b c - d) on rows 0, 4, 8, ..., `lookups` range-lookup columns against a
2^bits-entry table, copy constraints across advice / fixed columns, 5 blinding rows.  The small circuits of the reference size their columns
with `calculate_params(Some(20))` (/root/reference/voter/benches/voter_circuit.rs:49-51,
/root/reference/aggregator/benches/state_transition_circuit.rs:48-50; the browser config is 412 advice + 11 lookup columns at k = 15:
/root/reference/voter/frontend/app/worker.js:95-102): `run(13, 256, lookups=8)` and `run(15, 64, lookups=8)` are those shapes, with all
the columns of a phase committed through ONE batched call (`zkhip_msm_g1_registered_batch_device`) as a Rust host would have to.  Checks (the prover's own invariants): both
grand products close, the quotient is a polynomial (coefficients of degree >= 3n vanish), commit_lagrange(column) = commit(coefficients).
By default there is no transcript: challenges are seeded.  --transcript (run(transcript=True)): Fiat-Shamir challenges from a Blake2b transcript, and
the proof as bytes; --poseidon --gwc: the Poseidon transcript and the GWC multi-open, `gen_snark`'s pair.
Usage: prove_flow.py [k] [gate_cols] [lookups] [--device-randomness] [--mock] [--verify] [--transcript] [--poseidon] [--gwc]   (default 16 4 1).
--mock (run(mock=True)): the witness is checked against the circuit on the device before keygen and the arguments run (lap `mock_prover`).
--device-randomness (run(device_randomness=True)): every blinding tail is drawn by zkhip_fr_random_rows_device, all columns of a step in one
call, and the vanishing argument's random polynomial is filled by zkhip_fr_random_device and committed (lap `vanishing_random_poly`); the
default flow draws its blinding rows with torch and has no such lap."""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch

import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import _lib, fields as F, keygen as KG, multiopen as MO, prover as P, verifier as V
from zksnap_circuits_halo2_amd.verifier import verify_transcript_proof      # run() calls the verifier through this module's name

R = F.R_MOD
NOT_PROVING = ("setup_srs", "witness_columns", "mock_prover", "stack_columns", "pk_file_round_trip", "pk_upload", "verify", "on_proof")      # and keygen_*


class Laps:
    """the lap clock: a lap waits for the device and adds the time since the previous lap to its name"""

    def __init__(self):
        self.ms, self.last = {}, time.perf_counter()

    def restart(self):
        self.last = time.perf_counter()

    def __call__(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.ms[name] = self.ms.get(name, 0.0) + (now - self.last) * 1e3
        self.last = now


def _keygen(params, w, lap, pk_file, sharded_key):
    """the device proving key and, with pk_file, the size of the file it went through"""
    fixed = [f.cpu().numpy().view(np.uint64).reshape(-1, 4) for f in w.fixed]
    if pk_file is None:
        # the key is produced in HBM and stays there (keygen.keygen_device): sigma columns by gather, commitments against the
        # registered g_lagrange, transforms in place
        dpk = KG.keygen_device(params, w.cs, fixed, w.assembly, row_shards=sharded_key)
        del fixed                        # 2^k x 32 bytes of host memory per column: released inside this lap, not inside the prover's first
        lap("keygen_device")
        return dpk, None
    vk = KG.keygen_vk(params, w.cs, fixed, w.assembly)
    lap("keygen_vk")
    pk = KG.keygen_pk(params, vk, w.cs, fixed, w.assembly)
    del fixed
    lap("keygen_pk")
    with open(pk_file, "wb") as fh:
        pk.write(fh, KG.RAW_BYTES_UNCHECKED)
    with open(pk_file, "rb") as fh:
        pk2 = KG.ProvingKey.read(fh, KG.RAW_BYTES_UNCHECKED, w.cs)
    parts = lambda p_: ([p_.l0, p_.l_last, p_.l_active_row, p_.vk.fixed_commitments, p_.vk.permutation_commitments] + p_.fixed_values + p_.fixed_polys + p_.fixed_cosets
                        + p_.permutations + p_.permutation_polys + p_.permutation_cosets)
    assert all(np.array_equal(x, y) for x, y in zip(parts(pk), parts(pk2))), "ProvingKey::read(ProvingKey::write(pk)) differs from pk"
    lap("pk_file_round_trip")
    dpk = KG.DeviceProvingKey.from_host(pk2, w.cs, row_shards=sharded_key)      # the READ key is what the prover uses
    lap("pk_upload")
    return dpk, os.path.getsize(pk_file)


def _verify_seeded(pv, params, corrupt_proof, on_proof, lap):
    """what a verifier holds -- commitments, evaluations, H and H' -- through both halves of `verify_proof`: the identity at x over the
    evaluations and the seeded challenges (one device call, verifier.identity_statuses), then the openings and one pairing check;
    corrupt_proof changes one of them first"""
    vqueries, challenges, ok = pv.verifier_queries(), pv.ch.multiopen_challenges, False
    if pv.multiopen_proof is not None:
        H_mo, Hp_mo = pv.multiopen_proof
        if corrupt_proof == "eval":
            vqueries[len(vqueries) // 2].eval = (vqueries[len(vqueries) // 2].eval + 1) % R
        elif corrupt_proof == "commitment":
            vqueries[0].commitment = vqueries[-1].commitment                  # the first fixed column's opening names a quotient piece's commitment
        elif corrupt_proof == "witness":
            moved = np.zeros(12, dtype=np.uint64)
            both = np.stack([Hp_mo, MO._generator_xyz(params)])
            _lib.check(_lib.load().zkhip_g1_sum(both.ctypes.data, 2, moved.ctypes.data))     # H' + G: another curve point
            Hp_mo = moved
        public = [pv.w.instance_values] if pv.cs.num_instance else None       # the instance columns are evaluated from these, inside the identity call
        holds = V.identity_statuses(pv.dpk.vk, pv.k, pv.plan, [[q.eval for q in vqueries]], [(pv.theta, pv.beta, pv.gamma, pv.y, pv.x)], public)[0] == 0
        ok = bool(holds) and MO.VerifierSHPLONK(params).verify_proof(vqueries, H_mo, Hp_mo, *challenges)
    lap("verify")
    if on_proof is not None and pv.multiopen_proof is not None:
        on_proof(params, pv.k, pv.queries, vqueries, pv.commit_ptr, pv.multiopen_proof, challenges)
        lap("on_proof")
    return ok


def run(k=16, gate_cols=4, seed=1, lookup_bits=8, corrupt=None, verbose=True, pk_file=None, lookups=1, batched=None, sharded_quotient=False,
        sharded_key=False, lookups_one_call=True, device_randomness=False, mock=False, on_witness=None, verify=False, corrupt_proof=None, on_proof=None, transcript=False, multiopen="shplonk", instances=0,
        instance_len=4, fold=False):
    """instances: that many instance columns of `instance_len` public values each (prover.halo2_lib_witness ties every one to a gate input by a
    copy constraint): the mock step checks the witness against them, the prover absorbs them into the transcript behind the key and carries
    their columns through the permutation argument and the quotient without committing or opening them, and the verify step hands the values
    to the verifier, which evaluates the columns at x from them (zkhip_verify_identity_instances_device); the result gains `instances`, the
    values as integers.  corrupt="instance" breaks the copy constraint of the first public value.  With instances=0 nothing of this runs.
    mock: what the reference's `gen_proof` does before it proves (`MockProver::run(..).assert_satisfied()`,
    /root/reference/aggregator/src/wrapper.rs:117-123), over the columns where they lie: `mock.MockProver(..).assert_satisfied()` once the
    witness columns and the copy constraints exist, as lap `mock_prover` (not part of `prove_ms`).  A witness broken with `corrupt=` then raises
    an AssertionError that says where -- ("gate", gate, polynomial, row, rows) / ("copy", column, row, cells) / ("lookup", lookup, row, rows) --
    instead of the proof going on until a product does not close or the quotient is no polynomial.
    verify: the third step of the reference's `gen_proof` (`assert!(verify_proof(..))`, wrapper.rs:140-155): a `VerifierQuery` for every `ProverQuery`
    of the multi-open -- the commitments the flow has (advice, products, quotient pieces, the verifying key's fixed and sigma commitments), the
    evaluations of its `evals` buffer and of the rotated openings -- first through the quotient identity at x (the gate, permutation and lookup
    expressions against h(x)(x^n - 1): zkhip_verify_identity_device), then through `VerifierSHPLONK`, ending in one pairing check on the device:
    check "proof_verifies", lap `verify` (not part of `prove_ms`).  A witness broken with corrupt="gate" / "copy" still proves to the end and its
    openings are consistent: the identity is what makes "proof_verifies" false.  corrupt_proof: "eval" / "commitment" / "witness" change one evaluation, one
    commitment or H' AFTER the prover has run: "proof_verifies" is then false and every other check stays true.
    transcript: the challenges are not seeded but squeezed from a Blake2b transcript (zksnap_circuits_halo2_amd/transcript.py) in halo2
    `create_proof`'s order -- vk repr; advice commitments, theta; the lookups' permuted commitments, beta, gamma; permutation then lookup product
    commitments, the random polynomial's commitment (device_randomness), y; the quotient pieces, x; the evaluations in halo2's order, written from
    the device buffer they were computed into; the SHPLONK multi-open through `create_proof_transcript` -- and the result gains `proof` (bytes),
    `proof_bytes`, `proof_plan` and `proof_shape`; lap `transcript` (part of `prove_ms`).  transcript="poseidon": the same flow under the
    Poseidon transcript (transcript.PoseidonWrite; True and "blake2b" are Blake2b); multiopen="gwc" (transcript flows only): the GWC multi-open
    instead of SHPLONK, lap `multiopen_gwc`.  run(transcript="poseidon", multiopen="gwc") is the pair the reference's `gen_snark` proves under
    (/root/reference/aggregator/src/wrapper.rs:111-158).  With verify as well, `verify_transcript_proof` gets
    (params, vk, the proof bytes, shape and plan) after the prover's tensors are dropped, and checks the identity at x and the openings (fold=True: the openings through the batch verifier, multiopen.fold_check).  corrupt_proof=("byte", i) flips bit 0 of proof byte i
    before that; the three named values belong to the seeded flow.  The mock step keeps the seeded theta.
    on_proof (with verify): a callable handed (params, k, queries, verifier queries, commit, (H, H'), (y, v, u)) after the verdict, while the
    polynomials are still in HBM (tools/verify_time.py measures the verifiers there, on the flow's own plan); its time goes to the lap `verify`.
    on_witness: a callable handed (cs, k, fixed, advice, assembly, theta) at that same point, the columns being device tensors (a hook for a
    caller that wants the flow's witness inside a run; tools/mock_time.py takes its witness from prover.halo2_lib_witness directly).
    device_randomness: blinding tails through E.blind_rows_device (one call per step, whatever the number of columns) and the vanishing argument's
    random polynomial through E.random_fr_device + a commit against params.g (lap vanishing_random_poly); the seed of the stream comes from `seed`.
    lookups_one_call: the lookup argument of every lookup through zkhip_lookup_permute_many_device + zkhip_lookup_products_device (two calls per
    proof); False: one lookup at a time (the single-lookup call, two row programs and a grand product each).  The same bytes either way.
    corrupt: "gate" / "copy" break the witness; "lookup" puts a value outside the table into lookup column 1 (ZkhipError from the lookup phase).
    sharded_quotient: the single-program quotient goes through zkhip_fr_eval_rows_sharded_device (rows cut over the devices of zkhip_init; the
    key's cosets EXTENDED, the proof's columns COEFF, transformed inside the call) instead of coeff_to_extended + the whole-domain launch.
    sharded_key (needs sharded_quotient): the device key keeps its cosets as a row-shard set (keygen_device / from_host with row_shards) and the
    quotient reads them as COL_ROW_SHARDS, where they lie -- nothing of the key crosses between devices during the proof.
    pk_file: path -- the proving key is written there (`ProvingKey::write`, RawBytesUnchecked), read back, and the READ key is what the
    prover uses (the reference's wrapper does the same through build/*_pk.bin: /root/reference/aggregator/src/wrapper.rs:967-989, :1007-1034)"""
    P.check_options(transcript, lookups, lookups_one_call, sharded_quotient, sharded_key)
    tr_hash = "blake2b" if transcript is True else transcript      # False: seeded
    if transcript:
        P.transcript_classes(tr_hash)
    MO.multiopen_classes(multiopen)
    if multiopen != "shplonk" and not transcript:
        raise ValueError("multiopen=\"gwc\" needs a transcript: the seeded flow opens with SHPLONK")
    byte_flip = isinstance(corrupt_proof, tuple) and len(corrupt_proof) == 2 and corrupt_proof[0] == "byte"
    if corrupt_proof not in (None, "eval", "commitment", "witness") and not byte_flip:
        raise ValueError("corrupt_proof: eval, commitment, witness or (\"byte\", i)")
    if transcript and corrupt_proof is not None and not byte_flip:
        raise ValueError("transcript: the proof is bytes, corrupt it with corrupt_proof=(\"byte\", i)")
    if byte_flip and not (transcript and verify):
        raise ValueError("corrupt_proof=(\"byte\", i) needs transcript=True and verify=True")
    _lib.load()
    torch.manual_seed(seed)
    seeded = P.SeededChallenges(seed)    # transcript: only the mock step's theta and the SRS trapdoor come from here, every challenge is squeezed
    # device_randomness: a real prover takes these 32 bytes from its own generator, once per proof
    blinding = P.DeviceBlinding(random.Random(seed ^ 0xB11D).randbytes(32)) if device_randomness else P.TorchBlinding()
    dpk = None
    lap = Laps()
    params = Z.ParamsKZG.setup(k, seeded.s)
    lap("setup_srs")
    try:
        w = P.halo2_lib_witness(k, gate_cols, lookups, blinding, lookup_bits, corrupt, instances, instance_len)
        pv = P.Prover(params, w, blinding, batched, lap, multiopen)
        lap("witness_columns")
        pv.commit_advice()
        if mock:
            from zksnap_circuits_halo2_amd import mock as MK

            with MK.MockProver(w.cs, k, w.fixed, w.advice, w.instance, w.assembly, theta=seeded.theta()) as mock_prover:
                mock_prover.assert_satisfied()
            lap("mock_prover")
        if on_witness is not None:
            on_witness(w.cs, k, w.fixed, w.advice, w.assembly, seeded.theta())
            lap("witness_columns")
        dpk, pk_bytes = _keygen(params, w, lap, pk_file, sharded_key)
        vk = dpk.vk
        pv.prove(dpk, P.TranscriptChallenges(vk, tr_hash) if transcript else seeded, lookups_one_call, sharded_quotient, sharded_key)

        proof_verifies = _verify_seeded(pv, params, corrupt_proof, on_proof, lap) if verify and not transcript else None
        n, ncol = pv.n, pv.qc.total
        checks = {"permutation_product_closes": pv.permutation_closes, "lookup_product_closes": pv.lookup_closes,
                  "quotient_is_a_polynomial": not bool(pv.h_coeff[3 * n:].any().item()) and bool(pv.h_coeff[:3 * n].any().item()),
                  "commit_lagrange_equals_commit_coeff": P.affine(pv.adv_commit[0]) == P.affine(pv.a0_coeff_commit), "multiopen_linearisation_vanishes": pv.multiopen_ok}
        n_proof_cols = sum(hi - lo for lo, hi in pv.proof_ranges)
        n_msm = len(pv.adv_commit) + len(pv.product_kinds()) + 1 + len(pv.h_commit) + 2
        shape = {"advice": gate_cols + lookups, "lookups": lookups, "permutation_sets": w.cs.num_permutation_sets, "random_poly": bool(device_randomness)}
        res = {"timings_ms": lap.ms, "prove_ms": None, "checks": checks, "columns": ncol, "proof_columns": n_proof_cols, "msms": n_msm, "queries": len(pv.queries),
               "program_insns": pv.program_insns, "program_registers": pv.program_registers, "h_commitments": [P.affine(c) for c in pv.h_commit],
               "keygen_ms": None, "pk_file_bytes": pk_bytes,
               "vanishing_random_commitment": P.affine(pv.commitments[("random", 0)]) if device_randomness else None}
        if instances:
            res["instances"] = public = [list(column) for column in w.instance_values]
        if transcript:
            res.update(proof=pv.proof, proof_bytes=len(pv.proof), proof_plan=pv.plan, proof_shape=shape)
        proved, batched, ek = pv.multiopen_proof is not None, pv.batched, pv.dom.extended_k
        if verify and transcript:
            # the verifier gets (params, vk, proof bytes, the query plan) and nothing else: the prover's polynomials, commitments and evaluations
            # are dropped first, so that a verdict cannot lean on them
            torch.cuda.synchronize()
            lap.restart()                                          # the lap `verify` starts here
            proof_verifies = False
            if proved:
                del pv, w
                checked = bytearray(res["proof"])
                if byte_flip:
                    checked[corrupt_proof[1]] ^= 1
                how = () if (tr_hash, multiopen) == ("blake2b", "shplonk") else (tr_hash, multiopen)      # the verifier's defaults
                extra = {"fold": True} if fold else {}                                                     # (the default call is spelled as it always was)
                if instances:
                    proof_verifies = verify_transcript_proof(params, vk, k, bytes(checked), dict(shape), list(res["proof_plan"]), *how, instances=public, **extra)
                else:
                    proof_verifies = verify_transcript_proof(params, vk, k, bytes(checked), dict(shape), list(res["proof_plan"]), *how, **extra)
            lap("verify")
        if verify:
            checks["proof_verifies"] = proof_verifies
        t = lap.ms
        res["prove_ms"] = prove_ms = sum(v for kk, v in t.items() if kk not in NOT_PROVING and not kk.startswith("keygen_"))
        res["keygen_ms"] = t.get("keygen_vk", 0.0) + t.get("keygen_pk", 0.0) + t.get("keygen_device", 0.0)
        if verbose:
            print(f"k={k} gate_cols={gate_cols} lookups={lookups}{' (batched commits)' if batched else ''}: {ncol} columns ({n_proof_cols} witness-dependent, {ncol - n_proof_cols} of the proving key), {n_msm} MSMs of 2^{k}, "
                  f"{n_proof_cols} iNTT 2^{k}, {n_proof_cols} NTT 2^{ek}, 1 iNTT 2^{ek} per proof")
            for name, ms in t.items():
                print(f"  {name:28s} {ms:9.3f} ms")
            print(f"  {'prover steps (no setup/witness)':28s} {prove_ms:9.3f} ms")
            print("  checks:", checks)
        return res
    finally:
        torch.cuda.synchronize()
        if dpk is not None:
            dpk.free()
        params.close()


if __name__ == "__main__":
    dr, mk, vf, tp = "--device-randomness" in sys.argv, "--mock" in sys.argv, "--verify" in sys.argv, "--transcript" in sys.argv
    if "--poseidon" in sys.argv:
        tp = "poseidon"
    mo = "gwc" if "--gwc" in sys.argv else "shplonk"
    sys.argv = [a for a in sys.argv if a not in ("--device-randomness", "--mock", "--verify", "--transcript", "--poseidon", "--gwc")]
    kk = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    gg = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    ll = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    res = run(kk, gg, lookups=ll, device_randomness=dr, mock=mk, verify=vf, transcript=tp, multiopen=mo)
    sys.exit(0 if all(res["checks"].values()) else 1)

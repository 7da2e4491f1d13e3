"""The verifier of proofs written through prover.TranscriptChallenges, given as bytes: `verify_transcript_proofs` over a batch -- the quotient
identity at x of all of them in one device call (`identity_statuses`), then the openings of those that passed, one by one or folded into one
pairing check -- and `verify_transcript_proof`, the batch of one.  It is handed the opening plan (prover.opening_plan: the prover makes it) and
takes everything that depends on the multi-open from that scheme's verifier class (multiopen.VerifierGWC / VerifierSHPLONK): how its part of a
proof is read, its fold plan, its rows of scalars, its one-by-one verdict."""
import contextlib
import io

import numpy as np
import torch

from . import evaluation as E, fields as F, keygen as KG, multiopen as MO, tensors as T
from .transcript import decoded, transcript_classes, vk_transcript_repr

R = F.R_MOD
DEV = torch.device("cuda", 0)


def words(values):
    """python ints -> device tensor of Montgomery words"""
    return T.fr_words(values, device=DEV)


def verifier_queries(plan, commitments, evals, x, k):
    """a VerifierQuery per triple of the plan; commitments: (kind, index) -> Jacobian limbs.  poly_id keeps polynomials with equal commitments
    (two selector columns with the same rows) apart, as the prover does."""
    w = F.omega_for(k)
    return [MO.VerifierQuery(x * pow(w, r, R) % R, commitments[(kind, idx)], e, poly_id=(kind, idx)) for (kind, idx, r), e in zip(plan, evals)]


def key_points(vk):
    """the key's commitments by (kind, index), as the key holds them: affine limbs"""
    com = {("fixed", i): c for i, c in enumerate(vk.fixed_commitments)}
    com.update({("sigma", i): c for i, c in enumerate(vk.permutation_commitments)})
    return com


def key_commitments(vk):
    """the key's commitments by (kind, index) as Jacobian limbs: what `verifier_queries` is handed beside a proof's own"""
    points = key_points(vk)
    return dict(zip(points, MO._points_xyz(points.values())))


def _read_proof_head(r, vk_repr, shape, plan, instances=(), on_device=False):
    """a proof up to its evaluations, in the prover's order: (commitments by (kind, index), (theta, beta, gamma, y, x), the evaluations as
    integers); the reader is left in front of the multi-open's part.  instances: the proof's public inputs, one list of integers per instance
    column, absorbed behind the key.  on_device: the commitments stay in HBM, each an (8,) affine device tensor (the batch verifier's MSMs read
    them there).  ZkhipError(-1): bytes that do not decode"""
    def xyz(points):                                       # device affine points -> Jacobian limbs with z = 1 for the host-side accumulation
        return list(points) if on_device else MO._points_xyz(points.cpu().numpy().view(np.uint64).reshape(-1, 8))

    n_adv, n_lk, n_sets = shape["advice"], shape["lookups"], shape["permutation_sets"]
    r.common_scalar(vk_repr)
    for column in instances:
        for v_ in column:
            r.common_scalar(v_ % R)
    com = {("advice", i): c_ for i, c_ in enumerate(xyz(r.read_points(n_adv)))}
    theta = r.squeeze_challenge()
    if n_lk:
        for j, c_ in enumerate(xyz(r.read_points(2 * n_lk))):
            com[("lookup_pa" if j % 2 == 0 else "lookup_ps", j // 2)] = c_
    beta, gamma = r.squeeze_challenge(), r.squeeze_challenge()
    for j, c_ in enumerate(xyz(r.read_points(n_sets + n_lk))):
        com[("perm", j) if j < n_sets else ("lookup_z", j - n_sets)] = c_
    if shape["random_poly"]:
        com[("random", 0)] = xyz(r.read_points(1))[0]
    y = r.squeeze_challenge()
    for i, c_ in enumerate(xyz(r.read_points(3))):
        com[("h", i)] = c_
    x = r.squeeze_challenge()
    return com, (theta, beta, gamma, y, x), r.read_scalars(len(plan))


def _kept_on(vk, what, key, make):
    """make(), made once per (key object, `what`, `key`) and kept on the key object, so it lives as long as the key does"""
    cache = vk.__dict__.setdefault("_verifier_" + what, {})
    if key not in cache:
        cache[key] = make()
    return cache[key]


def identity_program_of(vk, plan, k):
    """the quotient identity of the key's circuit over `plan` (evaluation.identity_program), compiled and marshalled once per (key, plan).
    ValueError: a key without its constraint system"""
    if getattr(vk, "cs", None) is None:
        raise ValueError("the verifying key carries no constraint system (vk.cs): the verifier cannot state the circuit's identity")
    return _kept_on(vk, "identity_programs", (k, tuple(plan)), lambda: E.identity_program(
        vk.cs, plan, k, instance_queries=E.instance_queries(vk.cs) if vk.cs.num_instance else None)._marshal())


def _check_instances(cs, k, instances, proofs):
    """instances[p][c] = the integers of instance column c of proof p: one entry per proof, one list per column, every proof the same lengths
    (a circuit fixes them), none longer than the usable rows (halo2's `InstanceTooLarge`).  Returns the columns' lengths."""
    if len(instances) != proofs or any(len(per_proof) != cs.num_instance for per_proof in instances):
        raise ValueError(f"instances: {cs.num_instance} columns of public inputs for each of the {proofs} proofs")
    lens = [len(column) for column in instances[0]] if instances else [0] * cs.num_instance
    if any([len(column) for column in per_proof] != lens for per_proof in instances):
        raise ValueError("instances: the proofs of one circuit have instance columns of the same lengths")
    if any(length > (1 << k) - (cs.blinding_factors + 1) for length in lens):
        raise ValueError("instances: a column holds more values than the circuit has usable rows")
    return lens


def identity_statuses(vk, k, plan, evals, challenges, instances=None, d_evals=None):
    """zkhip_verify_identity_device over a batch: evals[i] the integers of proof i in the plan's order, challenges[i] = (theta, beta, gamma, y,
    x); for a circuit with instance columns instances[i] = proof i's public inputs, a list of integers per column, evaluated on the device
    (zkhip_verify_identity_instances_device).  d_evals: the evaluations as a (proofs, len(plan), 4) device tensor where the caller has uploaded
    them already (the batch verifier reads the same records).  An int32 array: 0 the identity holds, 1 it does not, 2 x lies in the domain."""
    n_instance = vk.cs.num_instance if getattr(vk, "cs", None) is not None else 0
    if n_instance and instances is None:
        raise ValueError("identity_statuses: the circuit has instance columns: hand in the proofs' public inputs (instances=)")
    if not evals:
        return np.zeros(0, dtype=np.int32)
    prog = identity_program_of(vk, plan, k)
    if d_evals is None:
        d_evals = words([e_ for row in evals for e_ in row]).reshape(len(evals), len(plan), 4)
    d_challenges = words([c_ for row in challenges for c_ in row]).reshape(len(evals), 5, 4)
    usable = (1 << k) - (vk.cs.blinding_factors + 1)
    if not n_instance:
        return E.verify_identity_device(prog, d_evals, d_challenges, k, usable)[0]
    lens = _check_instances(vk.cs, k, instances, len(evals))
    flat = [v_ % R for per_proof in instances for column in per_proof for v_ in column]
    d_instances = words(flat).reshape(len(evals), sum(lens), 4) if flat else None
    return E.verify_identity_device(prog, d_evals, d_challenges, k, usable, instances=d_instances, column_lens=lens, queries=E.instance_queries(vk.cs))[0]


def _fold_openings(params, fold_plan, k, heads, order, d_evals, rows_of, fold_seed, verdicts, scheme, one_by_one, key_points):
    """The openings of the proofs `order` (their heads read with on_device=True, the readers in front of the multi-open's part) decided by
    multiopen.fold_check.  d_evals: the uploaded evaluations, rows_of[i] the row of proof i in them; scheme: the multi-open's verifier class,
    fold_plan its plan; one_by_one(i, part=None): proof i by the multi-open's own verifier.  A proof whose multi-open part does not decode is
    refused alone; a proof with x = 0 mod r (where the grouping by rotation and halo2's grouping by point differ) is verified one by one, and
    so is a proof that the scheme's scalars call gives a status other than 0.  The rows of the folded proofs are made on the device: the
    host's `gwc_accumulate` and `shplonk_accumulate` run only inside the one-by-one verifier."""
    shared = np.stack([np.asarray(key_points[key_], dtype=np.uint64).reshape(8) for key_ in fold_plan.shared_keys] + [np.asarray(params.g[0], dtype=np.uint64).reshape(8)])
    d_shared = torch.from_numpy(shared.view(np.int64)).to(DEV)
    folded, parts = [], []
    x_of = {i: heads[i][2][4] for i in order}
    for i in order:
        if x_of[i] % R == 0:
            verdicts[i] = one_by_one(i)
            continue
        part = decoded(scheme(params).read_proof, heads[i][0], len(fold_plan.rotations), device=True)
        if part is not None:                               # else the multi-open's own points do not decode
            folded.append(i)
            parts.append(part)
    if not folded:
        return
    d_own = torch.stack([torch.stack(mine + [heads[i][1][key_] for key_ in fold_plan.own_keys]) for i, (mine, _) in zip(folded, parts)]).contiguous()
    index = torch.tensor([rows_of[i] for i in folded], dtype=torch.int64, device=DEV)
    d_points = words([c_ for i, (_, challenges) in zip(folded, parts) for c_ in (x_of[i],) + challenges]).reshape(len(folded), -1, 4)
    d_rows_a, d_rows_c, d_status = scheme.fold_scalars(fold_plan, d_evals.index_select(0, index).contiguous(), d_points, k)
    refused = [j for j, s_ in enumerate(d_status.cpu().tolist()) if s_ != 0] if d_status is not None else []
    if refused:                                            # no row exists for such a proof: the one-by-one verifier decides
        for j in refused:
            verdicts[folded[j]] = one_by_one(folded[j], parts[j])
        kept = [j for j in range(len(folded)) if j not in refused]
        if not kept:
            return
        keep = torch.tensor(kept, dtype=torch.int64, device=DEV)
        folded = [folded[j] for j in kept]
        d_own, d_rows_a, d_rows_c = (t_.index_select(0, keep).contiguous() for t_ in (d_own, d_rows_a, d_rows_c))
    for i, ok in zip(folded, MO.fold_check(params, d_rows_a, d_rows_c, d_own, d_shared, fold_seed)):
        verdicts[i] = bool(ok)


def _decide_carried(params, instances, accumulator_indices, verdicts):
    """the carried accumulators of the proofs accepted so far (accumulator.carried_accumulators): a proof with one that does not decode is
    refused; the rest are decided together and, where that fails, proof by proof"""
    from . import accumulator as A

    carried, status = A.carried_accumulators(instances, accumulator_indices, len(verdicts))
    for i, bad in enumerate((status.reshape(len(verdicts), -1) != 0).any(dim=1).cpu().tolist()):
        verdicts[i] = verdicts[i] and not bad
    live = [i for i, ok in enumerate(verdicts) if ok]
    if not live or A.decide_all(params, carried[live].reshape(-1, 2, 8).contiguous()):
        return
    for i in live:
        verdicts[i] = all(A.decide(params, acc.contiguous()) for acc in carried[i])


def verify_transcript_proofs(params, vk, k, proofs, shape, plan, hash="blake2b", multiopen="shplonk", *, identity=True, instances=None, fold=False,
                             fold_seed=None, accumulator_indices=()):
    """The verifier of a BATCH of proofs of one circuit, each written through TranscriptChallenges: it is handed the parameters, the verifying key
    (with its constraint system, `vk.cs`), the proofs' BYTES, and what a verifier knows of the circuit -- `shape` (how many advice columns,
    lookups, permutation sets, whether a random polynomial is committed) and `plan` (the opened (kind, index, rotation) triples, in the order
    their evaluations were written).  Every proof's head is replayed with reads -- commitments land on the device as affine points, evaluations
    as integers, every challenge is derived here --; then the two halves of halo2's `verify_proof`:
      the identity   the gate, permutation and lookup expressions at x against h(x) (x^n - 1), for ALL proofs in one device call
                     (zkhip_verify_identity_device; the program is compiled once per key and plan); the instance columns are evaluated
                     at x from the public inputs inside that call (zkhip_verify_identity_instances_device);
      the openings   for the proofs whose identity holds, `VerifierSHPLONK.verify_proof_transcript` (multiopen="gwc":
                     `VerifierGWC.verify_proof_transcript`), one pairing check each.
    A proof is accepted when both accept; bytes that do not decode reject that proof alone.  hash: the transcript the proofs were written under
    ("blake2b" or "poseidon").  identity=False leaves the first half out (the openings alone: what a test uses to show WHICH half refused).
    instances: for a circuit with instance columns, instances[i][c] = the integers of column c that proof i is verified AGAINST (the public
    inputs; never part of the proof).  They are absorbed into proof i's transcript behind the key, as the prover absorbed its own, so wrong
    inputs change every challenge, and they enter the identity through the instance columns' evaluations at x.  ValueError: a key whose
    circuit has instance columns and no `instances`; lengths that differ between the proofs or exceed the usable rows.
    fold=True: the openings of the proofs that passed the identity are decided together by multiopen.fold_check (halo2's `BatchVerifier`): the
    commitments stay in HBM, every proof's two accumulated points are rows of scalars -- multiopen="gwc": made by zkhip_gwc_scalars_device from
    the evaluations the identity call read; "shplonk": by zkhip_shplonk_scalars_device from the same records, as [H', H, own polynomials | key
    polynomials, G], one inversion per proof; a proof whose u hits a point outside the first rotation set has no such row (status 1) and is
    verified one by one --,
    and ONE pairing check accepts the batch; a batch that fails is bisected.  The verdicts are those of fold=False (a wrong proof passes a
    folded check with probability about 1 / r).  A proof with x = 0 mod r, a plan that repeats a triple and a plan with two rotations equal mod 2^k take the one-by-one path.
    fold_seed: the 32 bytes the random multipliers are drawn from; None (what a verifier uses) draws them from os.urandom, a fixed seed is for
    tests.
    accumulator_indices: (column, lo) pairs (`with_accumulator_indices`): instances[i][column][lo : lo + 12] are the limbs of a KZG accumulator
    that proof i carries (accumulator.to_limbs).  With them a proof is accepted when its identity holds, its openings hold, and every carried
    accumulator decodes and decides: one accumulator.decide_all over the carried accumulators of the proofs that got that far and, if that
    fails, proof by proof.  With () nothing new runs.
    Not built: committed instance columns, multi-phase challenges; folding across
    different circuits or parameter sets, a batch sharded over devices.  Returns a list of bools."""
    scheme = MO.multiopen_classes(multiopen)[1]
    reader = transcript_classes(hash)[1]
    if identity:
        identity_program_of(vk, plan, k)                   # a key that cannot state its identity is the caller's error, whatever the proofs are
    n_instance = vk.cs.num_instance if getattr(vk, "cs", None) is not None else 0
    if n_instance and instances is None:
        raise ValueError("verify_transcript_proofs: the key's circuit has instance columns: hand in the public inputs of every proof (instances=)")
    if n_instance:
        _check_instances(vk.cs, k, instances, len(proofs))
    vk_io = io.BytesIO()
    vk.write(vk_io, KG.RAW_BYTES)
    vk_repr = vk_transcript_repr(vk_io.getvalue())
    verdicts = [False] * len(proofs)
    fold_plan = _kept_on(vk, "fold_plans", (scheme, tuple(plan)), lambda: scheme.fold_plan(plan)) if fold and proofs else None
    fold = fold_plan is not None and fold_plan.foldable(k)
    points, key_com = key_points(vk), {}                   # the key's commitments: affine for the fold, Jacobian (made when first needed) for the queries
    with contextlib.ExitStack() as stack:
        heads = {}
        for i, proof in enumerate(proofs):
            r = stack.enter_context(reader(bytes(proof)))
            head = decoded(_read_proof_head, r, vk_repr, shape, plan, instances[i] if n_instance else (), on_device=fold)
            if head is not None:
                heads[i] = (r,) + head

        def one_by_one(i, part=None):
            """proof i by the multi-open's own verifier: its part read from its reader here, or `part`, what the fold path has read of it"""
            r, com, challenges, evals = heads[i]
            host = dict(zip(com, MO._points_xyz(com.values()))) if fold else com
            if not key_com:
                key_com.update(zip(points, MO._points_xyz(points.values())))
            queries = verifier_queries(plan, {**host, **key_com}, evals, challenges[4], k)
            if part is None:
                return bool(decoded(scheme(params).verify_proof_transcript, queries, r))
            return bool(scheme(params).verify_proof_read(queries, *part))

        order = sorted(heads)
        rows_of = {i: row for row, i in enumerate(order)}
        d_evals = None
        if fold and order:                                 # uploaded once: the identity call and the multi-open's scalars read the same records
            d_evals = words([e_ for i in order for e_ in heads[i][3]]).reshape(len(order), len(plan), 4)
        if identity:
            status = identity_statuses(vk, k, plan, [heads[i][3] for i in order], [heads[i][2] for i in order], [instances[i] for i in order] if n_instance else None,
                                       d_evals=d_evals)
            order = [i for i, s_ in zip(order, status) if s_ == 0]
        if fold:
            _fold_openings(params, fold_plan, k, heads, order, d_evals, rows_of, fold_seed, verdicts, scheme, one_by_one, points)
        else:
            for i in order:
                verdicts[i] = one_by_one(i)
    if tuple(accumulator_indices) and proofs:
        _decide_carried(params, instances, accumulator_indices, verdicts)
    return verdicts


def verify_transcript_proof(params, vk, k, proof, shape, plan, hash="blake2b", multiopen="shplonk", instances=None, fold=False, fold_seed=None):
    """The verifier of one proof given as bytes: `verify_transcript_proofs` over a batch of one -- the identity at x and the openings, accepted
    when both accept.  instances: the proof's public inputs, a list of integers per instance column.  fold, fold_seed: passed on (the openings
    through the batch verifier's path).  ValueError: a verifying key without its constraint system; a circuit with instance columns and no
    `instances`."""
    return verify_transcript_proofs(params, vk, k, [proof], shape, plan, hash, multiopen, instances=None if instances is None else [instances], fold=fold,
                                    fold_seed=fold_seed)[0]

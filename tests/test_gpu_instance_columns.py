"""GPU (-m gpu): instance columns in the verifier -- `zkhip_fr_instance_evals_device` and `zkhip_verify_identity_instances_device` against
tests/instance_reference.py, the defining sum over closed-form Lagrange values on Python integers.

  1  the kernel at k = 7: batches of 1, 15, 16, 17 and 65 proofs (either side of a 16-group block and of a wave), two columns of lengths (0, 33)
     and (17, 1), queries that name one column twice at rotations 0 and n - 1 (and at 1 and n - 3, whose indices wrap below zero), one proof of
     the batch with x in the domain (zeros) and the rest not, one proof whose public values are all r - 1; one case at k = 28 with 70 values
  2  the identity call on synthetic records (no prover; h_0 solved so that a record is accepted): every status and the report at batches of 1, 16,
     17 and 65 for a circuit whose permutation covers an instance column and for one whose gate reads Instance(0, 1); a batch that passes until
     one public value of its last record is changed reports (1, last); with no queries the call answers what zkhip_verify_identity_device answers"""
import functools
import random

import numpy as np
import pytest
import torch

import identity_reference as IR
import instance_reference as NR
from zksnap_circuits_halo2_amd import evaluation as E, fields as F, prover as P

pytestmark = pytest.mark.gpu
R = F.R_MOD
NONE = (1 << 64) - 1
DEV = torch.device("cuda", 0)
K = 7
N = 1 << K
U = N - 6


def words(values, *shape):
    if not values:
        return torch.zeros(shape + (4,), dtype=torch.int64, device=DEV)
    return torch.from_numpy(F.fr_encode(values).view(np.int64).reshape(*shape, 4)).to(DEV)


def decode(t):
    return F.fr_decode(t.cpu().numpy().view(np.uint64).reshape(-1, 4))


# ---- 1: the kernel -----------------------------------------------------------------------------------------------------------------------------
QUERIES = [(1, 0), (0, 0), (1, N - 1), (0, N - 1), (1, 1), (1, N - 3), (0, N - 3)]     # each column more than once; n - 1 is rotation -1


@functools.lru_cache(None)
def kernel_reference(k, lens, queries, proofs):
    """(instances[p][c], xs, e[q][p]) for `proofs` proofs, every x off the domain; proof 0's public values are all r - 1"""
    rng = random.Random(f"instance-kernel-{k}-{lens}")
    instances = [[[R - 1 if p == 0 else rng.randrange(R) for _ in range(length)] for length in lens] for p in range(proofs)]
    xs = [rng.randrange(R) for _ in range(proofs)]
    assert all(pow(x, 1 << k, R) != 1 for x in xs)
    return instances, xs, NR.evaluations(instances, queries, xs, k)


def run_kernel(k, lens, queries, instances, xs):
    flat = [v for proof in instances for column in proof for v in column]
    got = E.instance_evals_device(k, words(xs, len(xs)), words(flat, len(xs), sum(lens)), list(lens), list(queries))
    assert tuple(got.shape) == (len(queries), len(xs), 4)
    got = decode(got)
    return [got[q * len(xs):(q + 1) * len(xs)] for q in range(len(queries))]


@pytest.mark.parametrize("batch, inside", [(1, None), (1, 0), (15, 7), (16, 15), (17, 16), (65, 32)])
@pytest.mark.parametrize("lens", [(0, 33), (17, 1)])
def test_instance_evaluations_agree_with_the_defining_sum(lens, batch, inside):
    instances, xs, want = kernel_reference(K, lens, tuple(QUERIES), 65)
    instances, xs, want = instances[:batch], list(xs[:batch]), [list(row[:batch]) for row in want]
    if inside is not None:                                                             # this proof's x is a point of the domain: zeros, the others untouched
        xs[inside] = pow(F.omega_for(K), 5 + inside, R)
        for row in want:
            row[inside] = 0
    got = run_kernel(K, lens, QUERIES, instances, xs)
    assert got == want
    empty = lens.index(0) if 0 in lens else None
    for q, (c, _) in enumerate(QUERIES):
        if c == empty:
            assert got[q] == [0] * batch                                               # an empty column evaluates to zero
        else:
            assert all(e != 0 for p, e in enumerate(got[q]) if p != inside)


def test_instance_evaluations_at_k_28_with_seventy_values():
    k, n = 28, 1 << 28
    queries = ((0, 0), (0, n - 1), (0, 1), (0, n - 3))
    instances, xs, want = kernel_reference(k, (70,), queries, 17)
    xs, want = list(xs), [list(row) for row in want]
    xs[9] = pow(F.omega_for(k), 123456789, R)
    for row in want:
        row[9] = 0
    assert run_kernel(k, (70,), queries, instances, xs) == want


def test_no_queries_and_no_proofs_write_nothing():
    out = torch.full((2, 3, 4), -1, dtype=torch.int64, device=DEV)
    E.instance_evals_device(K, words([5, 6, 7], 3), words([1] * 6, 3, 2), [2], [], out=out)
    E.instance_evals_device(K, words([], 0), words([], 0, 2), [2], [(0, 0), (0, 1)], out=out)
    torch.cuda.synchronize()
    assert bool((out == -1).all())


# ---- 2: the identity call ------------------------------------------------------------------------------------------------------------------------
def systems(which):
    if which == "permutation":
        return E.halo2_lib_shape(1, 1, instances=1), (1, 1), (30,)
    cs = E.halo2_lib_shape(3, 2, instances=2)
    cs.gates = cs.gates + [[E.Fixed(0) * (E.Advice(0) - E.Instance(0, 1)) + E.Instance(1) * E.Advice(1, 1)]]
    return cs, (3, 2), (5, 70)


@functools.lru_cache(None)
def synthetic(which):
    """(cs, plan, queries, lens, program, 65 records (evals, challenges, instances), their reference statuses): record i is accepted, but
    i % 7 == 3 has one evaluation perturbed, i % 11 == 5 has x = omega^j and i % 13 == 7 has one public value changed after h_0 was solved"""
    cs, (gate_cols, lookups), lens = systems(which)
    plan = P.opening_plan(cs, gate_cols, lookups, U, True, "halo2")
    queries = E.instance_queries(cs)
    rng = random.Random(f"instance-records-{which}")
    used = [i for i, t in enumerate(plan) if t[0] != "random"]
    records = []
    for i in range(65):
        evals, challenges = [rng.randrange(R) for _ in plan], [rng.randrange(R) for _ in range(5)]
        instances = [[rng.randrange(R) for _ in range(length)] for length in lens]
        if i % 11 == 5:
            challenges[4] = pow(F.omega_for(K), rng.randrange(N), R)
        else:
            evals = NR.solve_h0(cs, plan, K, evals, tuple(challenges), instances)
            if i % 7 == 3:
                at = rng.choice(used)
                evals[at] = (evals[at] + 1 + rng.randrange(R - 1)) % R
            if i % 13 == 7:
                c = rng.randrange(len(lens))
                instances[c][rng.randrange(lens[c])] += 1
        records.append((evals, tuple(challenges), instances))
    statuses = [NR.status(cs, plan, K, e, c, inst) for e, c, inst in records]
    return cs, plan, queries, lens, E.identity_program(cs, plan, K, instance_queries=queries)._marshal(), records, statuses


def run_records(prog, plan, lens, queries, records):
    evals = words([e for rec in records for e in rec[0]], len(records), len(plan))
    challenges = words([c for rec in records for c in rec[1]], len(records), 5)
    instances = words([v % R for rec in records for column in rec[2] for v in column], len(records), sum(lens))
    status, report = E.verify_identity_device(prog, evals, challenges, K, U, instances=instances, column_lens=lens, queries=queries)
    return [int(s) for s in status], report


@pytest.mark.parametrize("batch", [1, 16, 17, 65])
@pytest.mark.parametrize("which", ["permutation", "gate"])
def test_synthetic_records_with_public_inputs_get_the_reference_status_and_report(which, batch):
    cs, plan, queries, lens, prog, records, statuses = synthetic(which)
    assert set(statuses) == {0, 1, 2} and statuses[7] == 1 and statuses[0] == 0        # record 7: only a public value differs
    got, report = run_records(prog, plan, lens, queries, records[:batch])
    assert got == statuses[:batch]
    assert report == IR.report(statuses[:batch])


@pytest.mark.parametrize("which", ["permutation", "gate"])
def test_one_changed_public_value_of_the_last_record_is_reported(which):
    cs, plan, queries, lens, prog, records, statuses = synthetic(which)
    good = [rec for rec, s in zip(records, statuses) if s == 0]
    for batch in (1, 16, 17, len(good)):
        assert run_records(prog, plan, lens, queries, good[:batch]) == ([0] * batch, (0, NONE))
        evals, challenges, instances = good[batch - 1]
        changed = [list(column) for column in instances]
        changed[-1][-1] = (changed[-1][-1] + 1) % R
        assert run_records(prog, plan, lens, queries, good[:batch - 1] + [(evals, challenges, changed)]) == ([0] * (batch - 1) + [1], (1, batch - 1))


def test_without_queries_the_call_answers_what_the_plain_call_answers():
    cs = E.halo2_lib_shape(3, 2)
    plan = P.opening_plan(cs, 3, 2, U, True, "halo2")
    prog = E.identity_program(cs, plan, K)._marshal()
    rng = random.Random("no-queries")
    records = []
    for i in range(33):
        evals, challenges = [rng.randrange(R) for _ in plan], [rng.randrange(R) for _ in range(5)]
        if i % 5 == 2:
            challenges[4] = pow(F.omega_for(K), i, R)
        elif i % 3:
            evals = IR.solve_h0(cs, plan, K, evals, tuple(challenges))
        records.append((evals, tuple(challenges)))
    evals = words([e for rec in records for e in rec[0]], len(records), len(plan))
    challenges = words([c for rec in records for c in rec[1]], len(records), 5)
    plain_status, plain_report = E.verify_identity_device(prog, evals, challenges, K, U)
    status, report = E.verify_identity_device(prog, evals, challenges, K, U, instances=None, column_lens=[], queries=[])
    assert list(status) == list(plain_status) == [IR.status(cs, plan, K, e, c) for e, c in records] and report == plain_report
    assert set(int(s) for s in status) == {0, 1, 2}
    # ... and with public inputs that no query reads
    status, report = E.verify_identity_device(prog, evals, challenges, K, U, instances=words([3] * 33 * 4, 33, 4), column_lens=[4], queries=[])
    assert list(status) == list(plain_status) and report == plain_report

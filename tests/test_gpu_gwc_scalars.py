"""GPU (-m gpu): zkhip_gwc_scalars_device against `multiopen.gwc_accumulate` over `verifier.verifier_queries`, that function's per-query scalars
summed per polynomial (tests/gwc_reference.py): every column of both rows, for the plans of (1, 1) and (3, 2) at k = 7 and (256, 8) at k = 13 (the
voter's shape, 1996 queries), B in {1, 17, 65}.  Evaluations and (x, v, u) are synthetic: no proof is made.  x, v and u are each also taken from
{1, r - 1}, and v = 0; a plan whose longest set has one query; the refusals of the C call."""
import ctypes as C
import functools
import random

import pytest
import torch

import gwc_reference as GR
from test_gwc_fold_host import _gwc_call
from zksnap_circuits_halo2_amd import _lib, fields as F, multiopen as MO, tensors as T

pytestmark = pytest.mark.gpu
R = F.R_MOD
DEV = torch.device("cuda", 0)
EINVAL = -1


def device_rows(gp, k, evals, points):
    B = len(evals)
    d_evals = T.fr_words([e for row in evals for e in row], DEV).reshape(B, gp.n_evals, 4)
    d_points = T.fr_words([c for p in points for c in p], DEV).reshape(B, 3, 4)
    rows_a, rows_c = MO.gwc_scalars_device(gp, d_evals, d_points, k)
    torch.cuda.synchronize()
    a, c = T.fr_ints(rows_a), T.fr_ints(rows_c)
    n_cols = gp.n_sets + gp.n_slots + 1
    return [a[i * n_cols:(i + 1) * n_cols] for i in range(B)], [c[i * gp.n_sets:(i + 1) * gp.n_sets] for i in range(B)]


def special_points(rng, B):
    """(x, v, u) per proof: random, with x, v, u each also from {1, r - 1} and v = 0 among the first proofs"""
    fixed = [(1, 1, 1), (R - 1, R - 1, R - 1), (rng.randrange(1, R), 0, rng.randrange(R)), (1, rng.randrange(R), R - 1), (R - 1, 1, rng.randrange(R)),
             (rng.randrange(1, R), R - 1, 1)]
    points = [tuple(rng.randrange(1, R) for _ in range(3)) for _ in range(B)]
    for i, p in enumerate(fixed):
        if 1 + i < B:
            points[1 + i] = p
    return points


@functools.lru_cache(None)
def plan_of_shape(shape):
    triples = GR.plan_for(*shape)
    return triples, MO.gwc_plan(triples)


@pytest.mark.parametrize("B", [1, 17, 65])
@pytest.mark.parametrize("shape", GR.SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-k{s[2]}")
def test_every_column_of_both_rows_equals_gwc_accumulate(shape, B):
    k = shape[2]
    triples, gp = plan_of_shape(shape)
    assert shape[0] != 256 or gp.n_evals == 1996
    rng = random.Random(f"gwc-{shape}-{B}")
    evals = [GR.pick(rng, gp.n_evals) for _ in range(B)]
    points = special_points(rng, B) if B > 1 else [(R - 1, rng.randrange(R), 1)]
    got_a, got_c = device_rows(gp, k, evals, points)
    for i in range(B):
        want_a, want_c = GR.gwc_rows(triples, gp, k, evals[i], *points[i])
        assert got_a[i] == want_a and got_c[i] == want_c, (shape, B, i)


def test_special_points_on_a_batch_of_one():
    """every special (x, v, u) as a batch of its own: proof 0 of a launch"""
    triples, gp = plan_of_shape(GR.SHAPES[1])
    rng = random.Random("one")
    for point in special_points(rng, 7)[1:]:
        evals = [GR.pick(rng, gp.n_evals)]
        got_a, got_c = device_rows(gp, 7, evals, [point])
        assert (got_a[0], got_c[0]) == GR.gwc_rows(triples, gp, 7, evals[0], *point), point


def test_a_plan_whose_longest_set_has_one_query():
    triples = [("advice", 0, 0), ("advice", 0, 1), ("fixed", 0, 5), ("advice", 1, -1)]
    gp = MO.gwc_plan(triples)
    assert gp.n_sets == 4 and max(gp.query_pos) == 0 and gp.own_keys == [("advice", 0), ("advice", 1)] and gp.shared_keys == [("fixed", 0)]
    rng = random.Random("short")
    evals = [GR.pick(rng, 4) for _ in range(17)]
    points = special_points(rng, 17)
    got_a, got_c = device_rows(gp, 7, evals, points)
    for i in range(17):
        assert (got_a[i], got_c[i]) == GR.gwc_rows(triples, gp, 7, evals[i], *points[i]), i


def test_the_refusals_of_the_call_with_a_device_present(lib):
    buf = torch.zeros((64, 4), dtype=torch.int64, device=DEV)
    real = dict(evals=buf.data_ptr(), points=buf.data_ptr(), rows_a=buf.data_ptr(), rows_c=buf.data_ptr())
    call = lambda **kw: _gwc_call(lib, **dict(real, **kw))
    assert call(n_sets=65) == EINVAL and call(n_evals=65528) == EINVAL and call(k=29) == EINVAL and call(rot=(0, 1, 128)) == EINVAL
    assert call(sets=(0, 1, 3, 0)) == EINVAL and call(pos=(0, 0, 0, 4)) == EINVAL and call(slots=(0, 1, 3, 0)) == EINVAL
    assert call(proofs=(1 << 24) + 1) == EINVAL and call(evals=buf.data_ptr() + 8) == EINVAL and call(rows_c=None) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0).all())                                   # nothing was enqueued
    assert call(proofs=0) == 0

"""GPU (-m gpu): zkhip_shplonk_scalars_device against `multiopen.shplonk_accumulate` over `verifier.verifier_queries`, laid out as a row
(tests/shplonk_reference.py): every column of both rows and the status, for the plans of (1, 1) and (3, 2) at k = 7 in both plan orders (set 0 is
the one-point set in the seeded order and the four-point set in the halo2 order), B in {1, 17, 65}, and (256, 8) at k = 13 (the voter's shape,
1996 queries), B in {1, 17}.  Evaluations and (x, y, v, u) are synthetic: no proof is made.  x, y, v, u are each also taken from {1, r - 1}, y = 0
and v = 0, as a batch of one and inside a batch; hand-made plans (one set only, sets of one point each, a set of three polynomials); degenerate
proofs inside a batch of 17 whose sixteen neighbours stay exact; the refusals of the C call with a device present."""
import functools
import random

import pytest
import torch

import gwc_reference as GR
import shplonk_reference as SR
from test_shplonk_fold_host import HAND_MADE, REFUSED_PLANS, _shplonk_call, degenerate_points, special_points
from zksnap_circuits_halo2_amd import fields as F, multiopen as MO, tensors as T

pytestmark = pytest.mark.gpu
R = F.R_MOD
DEV = torch.device("cuda", 0)
EINVAL = -1


def device_rows(sp, k, evals, points):
    """-> (A rows, C rows, statuses) of the batch, integers"""
    B = len(evals)
    d_evals = T.fr_words([e for row in evals for e in row], DEV).reshape(B, sp.n_evals, 4)
    d_points = T.fr_words([c for p in points for c in p], DEV).reshape(B, 4, 4)
    rows_a, rows_c, status = MO.shplonk_scalars_device(sp, d_evals, d_points, k)
    torch.cuda.synchronize()
    assert rows_a.shape == (B, sp.n_slots + 3, 4) and rows_c.shape == (B, 1, 4) and status.shape == (B,) and status.dtype == torch.int32
    a, c = T.fr_ints(rows_a), T.fr_ints(rows_c)
    n_cols = sp.n_slots + 3
    return [a[i * n_cols:(i + 1) * n_cols] for i in range(B)], [c[i:i + 1] for i in range(B)], status.cpu().tolist()


def batch_points(rng, B):
    """(x, y, v, u) per proof: random, the special ones among the first proofs"""
    points = [tuple(rng.randrange(1, R) for _ in range(4)) for _ in range(B)]
    for i, p in enumerate(special_points(rng)):
        if 1 + i < B:
            points[1 + i] = p
    return points


@functools.lru_cache(None)
def plan_of(shape, order):
    triples = GR.plan_for(*shape, order=order)
    return triples, MO.shplonk_plan(triples)


def check_batch(triples, sp, k, evals, points, degenerate=()):
    got_a, got_c, status = device_rows(sp, k, evals, points)
    for i in range(len(evals)):
        if i in degenerate:
            assert status[i] == 1 and got_a[i] == [0] * (sp.n_slots + 3) and got_c[i] == [0], i
            continue
        want_a, want_c = SR.shplonk_rows(triples, sp, k, evals[i], *points[i])
        assert status[i] == 0 and got_a[i] == want_a and got_c[i] == want_c, (i, [hex(c) for c in points[i]])
    return got_a


SMALL = [(shape, order, B) for shape in GR.SHAPES[:2] for order in ("halo2", "seeded") for B in (1, 17, 65)]
VOTER = [(GR.SHAPES[2], "halo2", B) for B in (1, 17)]


@pytest.mark.parametrize("shape, order, B", SMALL + VOTER, ids=lambda v: "-".join(str(c) for c in v) if isinstance(v, tuple) else str(v))
def test_every_column_of_both_rows_and_the_status_equal_shplonk_accumulate(shape, order, B):
    k = shape[2]
    triples, sp = plan_of(shape, order)
    if shape[0] == 256:
        assert sp.n_evals == 1996 and sp.n_slots == 947
    else:
        assert len(sp.set_points[0]) == (1 if order == "seeded" else 4)
    rng = random.Random(f"shplonk-{shape}-{order}-{B}")
    evals = [GR.pick(rng, sp.n_evals) for _ in range(B)]
    points = batch_points(rng, B) if B > 1 else [(R - 1, rng.randrange(R), 1, rng.randrange(2, R - 1))]
    check_batch(triples, sp, k, evals, points)


@pytest.mark.parametrize("order", ["halo2", "seeded"])
def test_special_points_on_a_batch_of_one(order):
    """every special (x, y, v, u) as a batch of its own: proof 0 of a launch"""
    triples, sp = plan_of(GR.SHAPES[1], order)
    rng = random.Random("one")
    for point in special_points(rng):
        check_batch(triples, sp, 7, [GR.pick(rng, sp.n_evals)], [point])


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_plans(name):
    triples = HAND_MADE[name]
    sp = MO.shplonk_plan(triples)
    rng = random.Random(name)
    check_batch(triples, sp, 7, [GR.pick(rng, sp.n_evals) for _ in range(17)], batch_points(rng, 17))
    check_batch(triples, sp, 7, [GR.pick(rng, sp.n_evals)], [tuple(rng.randrange(1, R) for _ in range(4))])


@pytest.mark.parametrize("shape, order", [(GR.SHAPES[1], "halo2"), (GR.SHAPES[1], "seeded"), (GR.SHAPES[0], "seeded")], ids=lambda v: str(v))
def test_degenerate_proofs_inside_a_batch_of_seventeen(shape, order):
    """x = 0 and u on a point outside set 0: status 1 and zero rows; u on a point of set 0: status 0, the host's rows, an exact zero in the H
    column.  One degenerate proof per batch, at a different row each time; the sixteen neighbours are exact."""
    k = shape[2]
    triples, sp = plan_of(shape, order)
    rng = random.Random(f"degenerate-{shape}-{order}")
    cases = degenerate_points(rng, sp, k)
    assert [c[4] for c in cases] == [1, 1, 0]
    for at, (x, y, v, u, status) in zip((0, 9, 16), cases):
        evals = [GR.pick(rng, sp.n_evals) for _ in range(17)]
        points = batch_points(rng, 17)
        points[at] = (x, y, v, u)
        got_a = check_batch(triples, sp, k, evals, points, degenerate=(at,) if status else ())
        if not status:
            assert got_a[at][1] == 0 and got_a[at][0] == u


def test_the_refusals_of_the_call_with_a_device_present(lib):
    buf = torch.zeros((64, 4), dtype=torch.int64, device=DEV)
    real = dict(evals=buf.data_ptr(), points=buf.data_ptr(), rows_a=buf.data_ptr(), rows_c=buf.data_ptr(), status=buf.data_ptr())
    call = lambda **kw: _shplonk_call(lib, **dict(real, **kw))
    for name, bent in REFUSED_PLANS.items():
        assert call(**bent) == EINVAL, name
    assert call(plan_null=True) == EINVAL and call(omega_null=True) == EINVAL and call(null_array="set_start") == EINVAL
    assert call(proofs=(1 << 24) + 1) == EINVAL and call(evals=buf.data_ptr() + 8) == EINVAL and call(rows_c=None) == EINVAL and call(status=None) == EINVAL
    assert call(status=buf.data_ptr() + 4) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0).all())                                   # nothing was enqueued
    assert call(proofs=0) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0).all())

"""GPU: zkhip_kzg_limbs_encode_device / _decode_device against the library's host forms and Python integers (tests/accumulator_reference.py),
on the coordinates and the refusals of tests/test_kzg_limbs_host.py, for n of {0, 1, 63, 64, 65, 4097} (a workgroup is 64 points)."""
import random

import numpy as np
import pytest
import torch

import accumulator_reference as AR
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import accumulator as A

pytestmark = pytest.mark.gpu
Q, R = O.Q_MOD, O.R_MOD
DEV = torch.device("cuda", 0)
SIZES = [0, 1, 63, 64, 65, 4097]


def words(values, p, shape):
    return np.array([O.limbs4(O.to_mont(v, p)) for v in values], dtype=np.uint64).reshape(shape)


def on_device(a):
    return torch.from_numpy(a.view(np.int64)).to(DEV)


@pytest.mark.parametrize("n", SIZES)
def test_encode_device(lib, n):
    base = AR.encode_cases(random.Random("limbs-gpu"))
    cases = [base[i % len(base)] for i in range(n)]
    pts = words([c for pair in cases for c in pair], Q, (n, 8))
    got = A.to_limbs(on_device(pts)).cpu().numpy().view(np.uint64)
    assert got.shape == (n, 6, 4)
    host = np.zeros((n, 6, 4), dtype=np.uint64)
    assert lib.zkhip_kzg_limbs_encode(pts.ctypes.data if n else None, n, host.ctypes.data if n else None) == 0
    assert np.array_equal(got, host)
    assert np.array_equal(got, words([v for x, y in cases for v in AR.fe_to_limbs(x) + AR.fe_to_limbs(y)], R, (n, 6, 4)))


@pytest.mark.parametrize("n", SIZES)
def test_decode_device(lib, n):
    base = AR.decode_cases(random.Random("limbs-gpu"))
    assert {st for _, (st, _) in base} == {0, 1, 2, 3}
    cases = [base[(i * 7) % len(base)] for i in range(n)]
    limbs = words([v for case, _ in cases for v in case], R, (n, 6, 4))
    points, status = A.from_limbs(on_device(limbs))
    points, status = points.cpu().numpy().view(np.uint64), status.cpu().numpy()
    assert points.shape == (n, 8) and status.shape == (n,)
    host_points, host_status = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    assert lib.zkhip_kzg_limbs_decode(limbs.ctypes.data if n else None, n, host_points.ctypes.data if n else None, host_status.ctypes.data if n else None) == 0
    assert np.array_equal(points, host_points) and status.tolist() == host_status.tolist() == [st for _, (st, _) in cases]
    assert [O.affine_from_limbs([int(w) for w in row]) for row in points] == [point for _, (_, point) in cases]


def test_an_accumulator_round_trips_through_its_twelve_limbs():
    rng = random.Random("limbs-acc")
    accs = [(O.scalar_mul(rng.randrange(1, R), (1, 2)), O.scalar_mul(rng.randrange(1, R), (1, 2))) for _ in range(3)]
    acc = on_device(np.array([O.affine_to_limbs(P) for pair in accs for P in pair], dtype=np.uint64).reshape(3, 2, 8))
    limbs = A.to_limbs(acc)
    assert tuple(limbs.shape) == (3, 2, 6, 4)
    assert np.array_equal(limbs.reshape(3, 12, 4).cpu().numpy().view(np.uint64), words([v for pair in accs for v in AR.accumulator_to_limbs(pair)], R, (3, 12, 4)))
    back, status = A.from_limbs(limbs)
    assert torch.equal(back, acc) and not status.any() and tuple(status.shape) == (3, 2)
    # a non-canonical word is no limb
    raw = limbs.clone()
    raw[1, 0, 2] = torch.from_numpy(np.array(O.limbs4(R), dtype=np.uint64).view(np.int64)).to(DEV)
    back, status = A.from_limbs(raw)
    assert status.cpu().tolist() == [[0, 0], [1, 0], [0, 0]] and not back[1, 0].any() and torch.equal(back[1, 1], acc[1, 1])

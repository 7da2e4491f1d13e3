"""GPU: zkhip_g1_row_msm_device (csrc/row_msm.hip) against one oracle scalar multiplication per row.

The points come from zkhip_g1_gen_walk_device, so every point's logarithm is known: a row's expected sum is [sum_j s_j log_j] G, computed on
Python integers (oracle/bn254.py), and compared exactly on the canonical affine words zkhip_g1_batch_normalize_device leaves.  The kernel's
switches: 64 columns (one lane per column, one wavefront per workgroup, one chunk per workgroup: the same T), 4096 columns (the second stage's
lanes start to take more than one chunk), 2^16 workgroups (a workgroup starts to take more than one chunk or row)."""
import random

import numpy as np
import pytest
import torch

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, accumulator as A, fields as F, multiopen as MO

pytestmark = pytest.mark.gpu
R = O.R_MOD
DEV = torch.device("cuda", 0)
G = (1, 2)
# the kernel's lambda from its lattice vector (a1, b1): a1 + lambda b1 = 0 mod r (csrc/msm.hip, "Decomposition")
LAMBDA = 0x89d3256894d213e3 * pow(0x6f4d8248eeb859fc8211bbeb7d4f1128, -1, R) % R
SPECIAL = [0, 1, R - 1, (1 << 127) - 1, 1 << 127, LAMBDA, (1 << 100) + 3, LAMBDA * ((1 << 100) + 5) % R, R - LAMBDA]      # the last three: halves (k1, 0), (0, k2), (0, -k2)
POOL = 6000
NEG = 64                      # pool[POOL + i] = -pool[i], i < NEG; pool[POOL + NEG] = (0, 0)
ZERO = POOL + NEG


@pytest.fixture(scope="module")
def pool():
    """(points (POOL + NEG + 1, 8) on the device, their logarithms): a walk, the negations of its head, the identity"""
    assert pow(LAMBDA, 3, R) == 1 and LAMBDA != 1
    rng = random.Random("row-msm-pool")
    t0, d = rng.randrange(1, R), rng.randrange(1, R)
    walk = torch.empty((POOL, 8), dtype=torch.int64, device=DEV)
    t0_words, d_words = F.fr_encode([t0])[0], F.fr_encode([d])[0]                 # (kept alive across the call)
    _lib.check(_lib.load().zkhip_g1_gen_walk_device(t0_words.ctypes.data, d_words.ctypes.data, POOL, walk.data_ptr(), None))
    head = walk[:NEG].cpu().numpy().view(np.uint64)
    neg = torch.from_numpy(np.stack([MO.negate_affine(p) for p in head]).view(np.int64)).to(DEV)
    logs = [(t0 + i * d) % R for i in range(POOL)]
    assert O.affine_from_limbs([int(w) for w in head[3]]) == O.scalar_mul(logs[3], G)                # the walk is what the header says
    return torch.cat([walk, neg, torch.zeros((1, 8), dtype=torch.int64, device=DEV)]), logs + [(-v) % R for v in logs[:NEG]] + [0]


def run(pool, scalars, own_idx, shared_idx, n_own, out=None):
    """scalars [B][n_cols] integers, own_idx [B][m] and shared_idx [t] indices into the pool -> (B, 8) affine words of the device's sums"""
    points, _ = pool
    B = len(scalars)
    rows = torch.from_numpy(F.fr_encode([s for row in scalars for s in row]).view(np.int64)).reshape(B, -1, 4).to(DEV)
    own = points[torch.tensor(own_idx, dtype=torch.int64, device=DEV)].contiguous() if own_idx and own_idx[0] else None
    shared = points[torch.tensor(shared_idx, dtype=torch.int64, device=DEV)].contiguous() if shared_idx else None
    xyz = A.row_msm_device(rows, own, shared, n_own=n_own if own is not None else None, out=out)
    aff = torch.empty((B, 8), dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().zkhip_g1_batch_normalize_device(xyz.data_ptr(), B, aff.data_ptr(), None))
    return aff.cpu().numpy().view(np.uint64)


def expected(pool, scalars, own_idx, shared_idx, n_own):
    _, logs = pool
    out = []
    for row, mine in zip(scalars, own_idx):
        idx = list(mine[:n_own]) + list(shared_idx)
        assert len(idx) == len(row)
        out.append(O.affine_to_limbs(O.scalar_mul(sum(s * logs[i] for s, i in zip(row, idx)) % R, G)))
    return np.array(out, dtype=np.uint64)


def draw_case(rng, n_rows, n_cols, n_own, extra):
    """random rows: scalars from SPECIAL and random ones, points anywhere in the pool (negations and the identity included)"""
    pick = lambda: rng.choice(SPECIAL) if rng.random() < 0.5 else rng.randrange(R)
    point = lambda: rng.choice([ZERO, rng.randrange(POOL, POOL + NEG)]) if rng.random() < 0.1 else rng.randrange(POOL)
    scalars = [[pick() for _ in range(n_cols)] for _ in range(n_rows)]
    own_idx = [[point() for _ in range(n_own + extra)] for _ in range(n_rows)]
    shared_idx = [point() for _ in range(n_cols - n_own)]
    return scalars, own_idx, shared_idx


def check(pool, scalars, own_idx, shared_idx, n_own):
    got, exp = run(pool, scalars, own_idx, shared_idx, n_own), expected(pool, scalars, own_idx, shared_idx, n_own)
    assert np.array_equal(got, exp), [i for i in range(len(exp)) if not np.array_equal(got[i], exp[i])][:8]


@pytest.mark.parametrize("n_cols", [1, 2, 33, 63, 64, 65, 127, 128, 129, 954, 4095, 4096, 4097])
def test_row_msm_sizes(pool, n_cols):
    """every n_own of {0, 1, n_cols - 1, n_cols}, both strides, n_rows of {1, 2, 3, 65}: each value with each width, the pairs in turn"""
    rng = random.Random(f"row-msm-{n_cols}")
    owns = sorted({0, 1, n_cols - 1, n_cols})
    combos = [(owns[i % len(owns)], 3 * (i % 2), n_rows) for i, n_rows in enumerate((1, 2, 3, 65))]
    combos += [(owns[(i + 1) % len(owns)], 3 * ((i + 1) % 2), n_rows) for i, n_rows in enumerate((3, 1, 2, 1))]
    assert {c[0] for c in combos} == set(owns) and {c[1] for c in combos} == {0, 3}
    for n_own, extra, n_rows in combos:
        check(pool, *draw_case(rng, n_rows, n_cols, n_own, extra if n_own else 0), n_own)


@pytest.mark.parametrize("scalar", SPECIAL)
def test_row_msm_special_scalars_alone(pool, scalar):
    """one column, one special scalar; and the same scalar in every column of a 65-column row"""
    check(pool, [[scalar]], [[5]], [], 1)
    check(pool, [[scalar] * 65, [scalar] * 65], [[7, 8, 9], [10, 11, 12]], list(range(100, 162)), 3)


def test_row_msm_degenerate_rows(pool):
    rng = random.Random("row-msm-degenerate")
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    # all-zero rows, at one chunk and at several
    for n_cols in (1, 33, 64, 130):
        got = run(pool, [[0] * n_cols, [0] * n_cols], [list(range(n_cols))] * 2, [], n_cols)
        assert not got.any()
    # the identity as a point: alone, in every column, among others
    check(pool, [[a]], [[ZERO]], [], 1)
    check(pool, [[a, b, a]], [[ZERO, ZERO]], [ZERO], 2)
    check(pool, [[a, b, a, b]], [[ZERO, 17]], [ZERO, 18], 2)
    # the same point twice: different scalars, equal scalars (an addition of two equal points in the tree), and scalars that cancel
    check(pool, [[a, b], [a, a], [a, R - a]], [[40, 40], [41, 41], [42, 42]], [], 2)
    check(pool, [[a, b], [a, a], [a, R - a]], [[0, 0]] * 3, [43, 43], 0)
    # P beside -P under equal scalars: the identity
    got = run(pool, [[a, a], [b, b]], [[3, POOL + 3], [POOL + 9, 9]], [], 2)
    assert not got.any()
    check(pool, [[a, a, b]], [[3, POOL + 3]], [60], 2)
    # a wide row whose chunks cancel: chunk 0 holds a P_j, chunk 1 holds a (-P_j)
    got = run(pool, [[a] * 128], [list(range(64)) + list(range(POOL, POOL + 64))], [], 128)
    assert not got.any()


@pytest.mark.parametrize("partner", [32, 1])
@pytest.mark.parametrize("n_cols", [64, 128])
def test_row_msm_tree_meets_a_doubling(pool, n_cols, partner):
    """column j and column j ^ partner hold the same scalar and the same point: with partner 32 every lane's first addition is of two equal
    points, with partner 1 the tree's last addition (lane 0 + lane 1) is, in every chunk"""
    rng = random.Random(f"row-msm-doubling-{n_cols}-{partner}")
    base = [rng.randrange(1, R) for _ in range(n_cols)]
    idx = [rng.randrange(POOL) for _ in range(n_cols)]
    scalars = [base[j & ~partner] for j in range(n_cols)]
    points = [idx[j & ~partner] for j in range(n_cols)]
    check(pool, [scalars], [points], [], n_cols)
    check(pool, [scalars], [[0]], points, 0)


def test_row_msm_c_side_reads_the_head_of_a_wider_array(pool):
    """the batch verifier's C side: rows_c over the first c own points of the A side's (B, m, 8) array, no shared points"""
    rng = random.Random("row-msm-c-side")
    for c, m, n_rows in ((1, 20, 3), (5, 20, 65), (5, 5, 2), (64, 430, 2), (65, 430, 3)):
        scalars, own_idx, _ = draw_case(rng, n_rows, c, c, m - c)
        check(pool, scalars, own_idx, [], c)


def test_row_msm_without_rows_writes_nothing(pool):
    points, _ = pool
    out = torch.full((4, 12), 0x5A5A, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    _lib.check(lib.zkhip_g1_row_msm_device(None, 33, None, 20, 20, points.data_ptr(), 0, None, None))
    _lib.check(lib.zkhip_g1_row_msm_device(points.data_ptr(), 33, points.data_ptr(), 20, 23, points.data_ptr(), 0, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())


@pytest.mark.parametrize("n_cols", [1, 65])
def test_row_msm_more_units_than_workgroups(pool, n_cols):
    """2^16 + 1 rows: the launch has 2^16 workgroups, so one of them takes a second unit (n_cols = 1), and with two chunks per row every
    workgroup of the first stage takes two and one of the second stage takes a second row.  Rows from four patterns over shared points"""
    _, logs = pool
    n_rows = (1 << 16) + 1
    rng = random.Random(f"row-msm-grid-{n_cols}")
    patterns = [[rng.choice([0, 1, 2, R - 1]) for _ in range(n_cols)] for _ in range(3)] + [[rng.randrange(R) for _ in range(n_cols)]]
    which = [rng.randrange(4) for _ in range(n_rows)]
    which[-1], which[0] = 3, 2
    shared_idx = [rng.randrange(POOL) for _ in range(n_cols)]
    points = pool[0]
    rows = torch.from_numpy(F.fr_encode([s for p in patterns for s in p]).view(np.int64).reshape(4, n_cols, 4)[np.array(which)]).to(DEV)
    xyz = A.row_msm_device(rows, None, points[torch.tensor(shared_idx, dtype=torch.int64, device=DEV)].contiguous())
    aff = torch.empty((n_rows, 8), dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().zkhip_g1_batch_normalize_device(xyz.data_ptr(), n_rows, aff.data_ptr(), None))
    got = aff.cpu().numpy().view(np.uint64)
    exp =[np.array(O.affine_to_limbs(O.scalar_mul(sum(s * logs[i] for s, i in zip(p, shared_idx)) % R, G)), dtype=np.uint64) for p in patterns]
    wrong = [i for i, w in enumerate(which) if not np.array_equal(got[i], exp[w])]
    assert not wrong, wrong[:8]

"""GPU (-m gpu): the pairing check kernel (csrc/pairing.hip) and the tower hook `zkhip_test_fq12_op`.  The hook runs every operation through the
quad policy in one quad and through the single-lane policy in one lane: both must give the canonical bytes of the big-integer reference
(tests/pairing_reference.py) on the inputs of the CPU test.  Every expected verdict of `zkhip_pairing_check` comes from the scalars of its
pairs (a_i G, b_i H): the product is one iff sum a_i b_i = 0 mod r; the negatives use seeded scalars, so a false "1" has probability 1 / r."""
import ctypes as C
import random

import numpy as np
import pytest

import pairing_reference as P
import pairing_vectors as V
from zksnap_circuits_halo2_amd import _lib, arithmetic as A

pytestmark = pytest.mark.gpu
R = P.R


def hook(lib, op, a: bytes, b: bytes):
    """-> (quad policy bytes, single-lane policy bytes)"""
    abuf, bbuf = np.frombuffer(a.ljust(384, b"\0"), dtype=np.uint64).copy(), np.frombuffer(b.ljust(384, b"\0"), dtype=np.uint64).copy()
    out = np.full(96, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    _lib.check(lib.zkhip_test_fq12_op(op, abuf.ctypes.data, bbuf.ctypes.data, out.ctypes.data))
    return out[:48].tobytes(), out[48:].tobytes()


def test_tower_operations_both_policies_equal_the_reference(lib):
    for name, op, a, b, want in V.tower_cases():
        quad, single = hook(lib, op, a, b)
        assert quad == single, name                                            # the same canonical bytes
        assert P.from_tower(V.dec12(quad)) == want, name


def test_miller_loop_both_policies_reduce_to_the_reference_pairing(lib):
    for name, a, want in V.miller_cases():
        quad, single = hook(lib, V.OP_MILLER, a, a)
        assert quad == single, name
        assert P.final_exponentiation(P.from_tower(V.dec12(quad))) == want, name


def test_hook_runs_one_policy_alone_and_the_two_pair_check(lib):
    name, op, a, b, want = V.tower_cases()[0]
    abuf, bbuf = np.frombuffer(a, dtype=np.uint64).copy(), np.frombuffer(b, dtype=np.uint64).copy()
    for flag, lo, hi in ((256, slice(0, 48), slice(48, 96)), (512, slice(48, 96), slice(0, 48))):
        out = np.full(96, 7, dtype=np.uint64)
        _lib.check(lib.zkhip_test_fq12_op(op + flag, abuf.ctypes.data, bbuf.ctypes.data, out.ctypes.data))
        assert P.from_tower(V.dec12(out[lo].tobytes())) == want and (out[hi] == 7).all()
    for name, g1, g2, n, want in V.verdict_cases():
        if n == 2:
            quad, single = hook(lib, V.OP_CHECK2, g1 + g2, b"")
            assert quad == single == (b"\x01" if want else b"\x00").ljust(384, b"\0"), name
    bad = np.zeros(48, dtype=np.uint64)
    assert lib.zkhip_test_fq12_op(12, bad.ctypes.data, bad.ctypes.data, np.zeros(96, dtype=np.uint64).ctypes.data) == -1      # ZKHIP_EINVAL


# ---- the check ---------------------------------------------------------------------------------------------------------------------------
def check_both_forms(lib, g1: bytes, g2: bytes, n: int) -> bool:
    """the host form and the `_device` form on the same pairs: the same verdict"""
    import torch

    a = np.frombuffer(g1, dtype=np.uint64).reshape(n, 8).copy()
    b = np.frombuffer(g2, dtype=np.uint64).reshape(n, 16).copy()
    host = A.pairing_check(a, b)
    d_ok = torch.full((1,), 0x55, dtype=torch.int32, device="cuda")
    if n:
        d_a, d_b = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
        pa, pb = d_a.data_ptr(), d_b.data_ptr()
    else:
        pa = pb = None
    _lib.check(lib.zkhip_pairing_check_device(pa, pb, n, d_ok.data_ptr(), None))
    torch.cuda.synchronize()
    dev = int(d_ok.cpu()[0])
    assert dev in (0, 1) and bool(dev) == host
    return host


def closing_scalars(rng, n):
    """n pairs of seeded scalars with sum a_i b_i = 0 mod r"""
    ab = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(n - 1)]
    if n == 1:
        return [(rng.randrange(1, R), 0)]                                      # (a G, identity)
    s = sum(a * b for a, b in ab) % R
    a_last = rng.randrange(1, R)
    return ab + [(a_last, -s * pow(a_last, -1, R) % R)]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 63, 64])
def test_pairing_check_verdicts_from_the_scalars(lib, n):
    """16 quads fill a wave: n = 16 / 17 end and begin a wave, 63 / 64 are one short of the workgroup and the whole of it.  A few distinct points
    are reused with different partners (a multiple of G in 64 big-integer steps each would dominate the test otherwise): the scalars of pair i
    are (a_i, b_i) = (alpha_{i mod 4} , beta_i) for 4 seeded alphas and as many seeded betas as the closing condition needs."""
    rng = random.Random(0xE0 + n)
    alphas = [rng.randrange(1, R) for _ in range(4)]
    betas = [rng.randrange(1, R) for _ in range(6)]
    ab = [(alphas[i % 4], betas[(i * 5 + i // 4) % 6]) for i in range(n - 1)]
    s = sum(a * b for a, b in ab) % R
    ab.append((alphas[(n - 1) % 4], -s * pow(alphas[(n - 1) % 4], -1, R) % R) if n > 1 else (alphas[0], 0))
    g1, g2, want = V.pairs_from_scalars(ab)
    assert want and check_both_forms(lib, g1, g2, n)
    bump = {0, n - 1, n // 2} | ({16} if n == 17 else set())
    for i in sorted(bump):
        if n == 1:
            bad = [(ab[0][0], 1)]                                              # identity + 1: a real pair, not one
        else:
            bad = ab[:i] + [(ab[i][0], (ab[i][1] + 1) % R)] + ab[i + 1:]
        g1, g2, want = V.pairs_from_scalars(bad)
        assert not want and not check_both_forms(lib, g1, g2, n), i


def test_pairing_check_identities_repeats_and_permutations(lib):
    rng = random.Random(0x1DE)
    ab = closing_scalars(rng, 5)
    # identity pairs on either side interleaved with a true product: (0 G, b H) and (a G, 0 H) contribute 1
    mixed = [ab[0], (0, 12345), ab[1], (6789, 0), ab[2], (0, 0), ab[3], ab[4]]
    g1, g2, want = V.pairs_from_scalars(mixed)
    assert want and check_both_forms(lib, g1, g2, len(mixed))
    mixed[2] = (mixed[2][0], (mixed[2][1] + 1) % R)
    g1, g2, want = V.pairs_from_scalars(mixed)
    assert not want and not check_both_forms(lib, g1, g2, len(mixed))
    # repeated pairs: (a, b) three times and (-3ab, 1)
    a, b = ab[0]
    rep = [(a, b)] * 3 + [(-3 * a * b % R, 1)]
    g1, g2, want = V.pairs_from_scalars(rep)
    assert want and check_both_forms(lib, g1, g2, 4)
    g1, g2, want = V.pairs_from_scalars([(a, b)] * 2 + [(-3 * a * b % R, 1)])
    assert not want and not check_both_forms(lib, g1, g2, 3)
    # the pairs of a true product permuted
    perm = list(ab)
    random.Random(5).shuffle(perm)
    assert perm != ab
    g1, g2, want = V.pairs_from_scalars(perm)
    assert want and check_both_forms(lib, g1, g2, 5)
    # nothing at all
    assert check_both_forms(lib, b"", b"", 0)


def test_pairing_check_argument_errors(lib):
    ok = C.c_int(7)
    g1, g2 = np.zeros((65, 8), dtype=np.uint64), np.zeros((65, 16), dtype=np.uint64)
    assert lib.zkhip_pairing_check(g1.ctypes.data, g2.ctypes.data, _lib.ZKHIP_MAX_PAIRS + 1, C.byref(ok)) == -1
    assert lib.zkhip_pairing_check(None, g2.ctypes.data, 1, C.byref(ok)) == -1
    assert lib.zkhip_pairing_check(g1.ctypes.data, None, 1, C.byref(ok)) == -1
    assert lib.zkhip_pairing_check_device(None, None, 1, None, None) == -1
    import torch

    buf = torch.zeros(64, dtype=torch.int64, device="cuda")                      # 16-byte aligned; + 8 bytes is not
    d_ok = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    assert lib.zkhip_pairing_check_device(buf.data_ptr() + 8, buf.data_ptr() + 128, 1, d_ok.data_ptr(), None) == -1
    assert lib.zkhip_pairing_check_device(buf.data_ptr(), buf.data_ptr() + 136, 1, d_ok.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert int(d_ok.cpu()[0]) == 5                                               # nothing was enqueued
    assert ok.value == 7

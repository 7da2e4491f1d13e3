"""Shared inputs of the PLUME tests: seeded voters generated once with tests/plume_reference.py, and the edge lists of the field, the group and
the joint ladder.  Nothing here imports the package under test."""
import functools
import hashlib
import random

import plume_reference as R

P, N, G = R.P, R.N, R.G
FULL = 2**256 - 1
MSG = bytes([1, 0])                        # the reference's proposal


def rng(tag):
    return random.Random(int.from_bytes(hashlib.sha256(f"plume-{tag}".encode()).digest()[:8], "big"))


@functools.lru_cache(maxsize=None)
def voters(count, msg=MSG, tag="voters"):
    """`count` valid voters (pk, nullifier, s, c) over `msg`, the same for every caller"""
    r = rng(f"{tag}-{msg.hex()}")
    return tuple(R.gen(r.randrange(1, N), msg, r.randrange(1, N)) for _ in range(count))


@functools.lru_cache(maxsize=None)
def points(count, tag="points"):
    r = rng(tag)
    return tuple(R.mul(r.randrange(1, N), G) for _ in range(count))


def small_x_point():
    """the curve point with the smallest x: x + p still fits 256 bits, a second, non-canonical spelling of a valid point"""
    x = next(x for x in range(1, 100) if pow(x**3 + 7, (P - 1) // 2, P) == 1)
    return (x, pow(x**3 + 7, (P + 1) // 4, P))


def off_curve_points():
    """malformed points: x >= p, y >= p, off the curve, the pair (0, 0)"""
    gx, gy = G
    sx, sy = small_x_point()
    assert R.on_curve((sx, sy)) and sx + P <= FULL
    return [(sx + P, sy), (P, gy), (gx, P), (FULL, gy), (gx, FULL), (FULL, FULL), (gx, gy + 1), (gx + 1, gy), (gy, gx), (1, 1), (0, 0), (0, 1), (gx, 0)]


def lincomb_edges():
    """(a, P, b, Q) at the joint ladder's corners: zero scalars, n - 1, n, 2^256 - 1, P = Q, P = -Q, a P = -b Q"""
    r = rng("lincomb-edges")
    A, B = points(2, "lincomb-edge-points")
    k = r.randrange(2, N)
    kA = R.mul(k, A)
    x, y = r.randrange(1, N), r.randrange(1, N)
    cases = [(0, A, y, B), (x, A, 0, B), (0, A, 0, B), (N - 1, A, y, B), (x, A, N - 1, B), (N, A, y, B), (N, A, N, B), (FULL, A, y, B), (FULL, A, FULL, B),
             (x, A, y, A), (x, A, x, A), (x, A, y, R.neg(A)), (x, A, x, R.neg(A)), (1, A, 1, A), (1, A, 1, R.neg(A)), (1, G, 1, G), (2, G, 0, G), (N, G, 0, G),
             (x * k % N, A, N - x, kA), (x * k % N + N if x * k % N + N <= FULL else x * k % N, A, N - x, kA), (1, A, N - 1, A), (1 << 255, A, 1 << 255, B),
             (1, A, 1 << 255, B), (N - 1, G, 1, G)]
    return cases

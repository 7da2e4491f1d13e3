"""KZG accumulators on Python integers, over the oracle's curve (a helper: no tests in it).  Limbs as csrc/kzg_limbs.hpp states them, `KzgAs`
without blinding over tests/poseidon_reference.Transcript.  Points are the oracle's: (x, y) tuples of canonical integers, None the identity."""
import poseidon_reference as PR
from oracle import bn254 as O

Q, R = O.Q_MOD, O.R_MOD
LIMBS, BITS = 3, 88
MASK = (1 << BITS) - 1


def fe_to_limbs(x):
    return [(x >> (BITS * i)) & MASK for i in range(LIMBS)]


def point_to_limbs(P):
    """six integers below r: x's limbs, then y's; the identity is (0, 0)"""
    x, y = (0, 0) if P is None else P
    return fe_to_limbs(x) + fe_to_limbs(y)


def accumulator_to_limbs(acc):
    return point_to_limbs(acc[0]) + point_to_limbs(acc[1])


def coordinate_status(limbs):
    """(status, value) of three integers that stand for Fr values: 1 a limb >= 2^88 (a value >= r can be no limb), 2 the coordinate >= q"""
    if any(v >= R or v > MASK for v in limbs):
        return 1, None
    x = sum(v << (BITS * i) for i, v in enumerate(limbs))
    return (2, None) if x >= Q else (0, x)


def point_from_limbs(limbs):
    """-> (status, point): 0 accepted, 1 a limb >= 2^88, 2 a coordinate >= q, 3 not on the curve ((0, 0) included); x is judged before y; a
    refused point is the identity"""
    sx, x = coordinate_status(limbs[:LIMBS])
    if sx:
        return sx, None
    sy, y = coordinate_status(limbs[LIMBS:])
    if sy:
        return sy, None
    if (x, y) == (0, 0) or not O.on_curve((x, y)):
        return 3, None
    return 0, (x, y)


EDGE_COORDINATES = [0, 1, (1 << 88) - 1, 1 << 88, (1 << 176) - 1, 1 << 176, Q - 1]


def encode_cases(rng, random_count=8):
    """(x, y) pairs of canonical coordinates: encode splits whatever it is given, so most of these are no points"""
    pairs = [(1, 2), (0, 0)] + [(a, b) for a in EDGE_COORDINATES for b in (a, EDGE_COORDINATES[-1 - EDGE_COORDINATES.index(a)])]
    pairs += [(rng.randrange(Q), rng.randrange(Q)) for _ in range(random_count)]
    return pairs + [O.scalar_mul(rng.randrange(1, R), (1, 2)) for _ in range(4)]


def decode_cases(rng, random_count=6):
    """(six integers below r, (status, point)): honest points, and every refusal -- a limb of 2^88 in each position, a top limb that makes the
    value q, the value 2^254, a value of 2^256 or more, off the curve, (0, 0)"""
    split = lambda v: [(v >> (BITS * i)) & MASK for i in range(LIMBS - 1)] + [v >> (BITS * (LIMBS - 1))]     # the top limb keeps what is left
    G = (1, 2)
    honest = [G, O.neg(G)] + [O.scalar_mul(rng.randrange(1, R), G) for _ in range(random_count)]
    cases = [point_to_limbs(P) for P in honest]
    for pos in range(2 * LIMBS):
        limbs = point_to_limbs(G)
        limbs[pos] = 1 << BITS
        cases.append(limbs)
    for bad in (Q, 1 << 254, (1 << 256) + 5, (1 << 264) - 1):
        cases += [split(bad) + fe_to_limbs(2), fe_to_limbs(1) + split(bad)]
    cases += [fe_to_limbs(1) + fe_to_limbs(3), fe_to_limbs(Q - 1) + fe_to_limbs(2), [0] * 6, fe_to_limbs(0) + fe_to_limbs(2), fe_to_limbs(honest[2][0]) + fe_to_limbs(honest[3][1])]
    return [(limbs, point_from_limbs(limbs)) for limbs in cases]


def msm(scalars, points):
    acc = None
    for s, P in zip(scalars, points):
        acc = O.add(acc, O.scalar_mul(s % R, P))
    return acc


def accumulate(accs):
    """`KzgAs::create_proof` without blinding over a fresh Poseidon transcript -> ((lhs, rhs), r); one accumulator is returned as it is (r = 1)"""
    if len(accs) == 1:
        return accs[0], 1
    tr = PR.Transcript()
    for lhs, rhs in accs:
        tr.common_point(*lhs)
        tr.common_point(*rhs)
    r = tr.squeeze()
    powers = [pow(r, i, R) for i in range(len(accs))]
    return (msm(powers, [a[0] for a in accs]), msm(powers, [a[1] for a in accs])), r

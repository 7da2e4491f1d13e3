"""CPU: the verifiers' equations in Python integers.  On an SRS whose trapdoor s is known every point is its discrete logarithm: a commitment
is p(s), the accumulated pair (L, R) of a verifier must satisfy dlog(L) = s dlog(R) -- checked here for a 3-set GWC plan and a 3-set SHPLONK plan
with the witnesses computed from the polynomials by the oracle's arithmetic, so that the set construction and the coefficients of
multiopen.VerifierGWC / VerifierSHPLONK are right before any GPU is involved (tests/test_gpu_verify.py runs them on points)."""
import random

import numpy as np
import pytest

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, multiopen as M

R = O.R_MOD
N = 16


def tag(i):
    """a stand-in commitment: 12 limbs that only have to be distinct"""
    return np.array([1000 + i] + [0] * 11, dtype=np.uint64)


def key(i):
    return tag(i).tobytes()


def poly_sub_const(p, c):
    return [(p[0] - c) % R] + list(p[1:])


def lincomb(polys, coeffs):
    out = [0] * N
    for p, c in zip(polys, coeffs):
        for t, v in enumerate(p):
            out[t] = (out[t] + c * v) % R
    return out


def divide(p, roots):
    for z in roots:
        assert O.eval_polynomial(p, z) == 0
        p = O.kate_division(p, z) + [0]
    return p


def plan(rng):
    """7 polynomials over 3 points: sets {a, c} x 3 polynomials, {b} x 2, {a, b, c} x 1, one polynomial queried twice at a point"""
    a, b, c = (rng.randrange(R) for _ in range(3))
    polys = {i: [rng.randrange(R) for _ in range(N)] for i in range(7)}
    order = [(0, c), (0, a), (1, b), (2, a), (2, c), (3, b), (4, a), (4, b), (4, c), (5, c), (5, a), (0, a)]
    return polys, order


def test_gwc_accumulated_pair_satisfies_the_pairing_equation_in_scalars():
    rng = random.Random(0x6C7)
    polys, order = plan(rng)
    s, v, u = (rng.randrange(1, R) for _ in range(3))
    queries = [M.VerifierQuery(z, tag(i), O.eval_polynomial(polys[i], z)) for i, z in order]
    # the prover's witnesses, as polynomials: one per distinct point, in order of first appearance
    sets = M.construct_intermediate_sets(queries)
    assert len(sets) == 3
    witnesses = []
    for z, qs in sets:
        pw = [pow(v, j, R) for j in range(len(qs))]
        batch = lincomb([polys[next(i for i in polys if key(i) == q.poly)] for q in qs], pw)
        witnesses.append(divide(poly_sub_const(batch, sum(p * q.eval for p, q in zip(pw, qs)) % R), [z]))
    w_dlog = [O.eval_polynomial(w, s) for w in witnesses]
    left, right, commitments = M.gwc_accumulate(queries, len(witnesses), v, u)
    assert len(left) == 3 and len(right) == 3 + len(commitments) + 1 and len(commitments) == len(order)
    c_dlog = [O.eval_polynomial(polys[next(i for i in polys if key(i) == c)], s) for c in commitments]
    L = sum(a * b for a, b in zip(left, w_dlog)) % R
    Rv = sum(a * b for a, b in zip(right, w_dlog + c_dlog + [1])) % R
    assert L * s % R == Rv
    # a changed evaluation, a changed challenge: the equation fails
    bad = [M.VerifierQuery(q.point, q.commitment, q.eval) for q in queries]
    bad[4].eval = (bad[4].eval + 1) % R
    _, right_bad, _ = M.gwc_accumulate(bad, 3, v, u)
    assert sum(a * b for a, b in zip(right_bad, w_dlog + c_dlog + [1])) % R != L * s % R
    _, right_bad, _ = M.gwc_accumulate(queries, 3, (v + 1) % R, u)
    assert sum(a * b for a, b in zip(right_bad, w_dlog + c_dlog + [1])) % R != L * s % R


def test_shplonk_accumulated_pair_satisfies_the_pairing_equation_in_scalars():
    rng = random.Random(0x5A9)
    polys, order = plan(rng)
    s, y, v, u = (rng.randrange(1, R) for _ in range(4))
    queries = [M.VerifierQuery(z, tag(i), O.eval_polynomial(polys[i], z)) for i, z in order]
    sets, super_points = M.construct_rotation_sets(queries)
    assert [len(rs.points) for rs in sets] == [2, 1, 3] and [len(rs.polys) for rs in sets] == [3, 2, 1]
    of = lambda k: polys[next(i for i in polys if key(i) == k)]
    # h(X) = sum_i v^i (sum_j y^j (P_ij - R_ij)) / Z_i
    h = [0] * N
    for i, rs in enumerate(sets):
        acc = [0] * N
        for j, k in enumerate(rs.polys):
            low = M._interpolate(rs.points, rs.evals[j]) + [0] * (N - len(rs.points))
            acc = lincomb([acc, of(k), low], [1, pow(y, j, R), -pow(y, j, R) % R])
        h = lincomb([h, divide(acc, rs.points)], [1, pow(v, i, R)])
    # L(X) = sum_i v^i Z_{T \ S_i}(u) sum_j y^j (P_ij(X) - R_ij(u)) - Z_T(u) h(X), normalised; h'(X) = L(X) / (X - u)
    zd = [M._vanishing_at([p for p in super_points if p not in rs.points], u) for rs in sets]
    norm = pow(zd[0], -1, R)
    Lx = [0] * N
    for i, rs in enumerate(sets):
        for j, k in enumerate(rs.polys):
            c = pow(v, i, R) * zd[i] % R * pow(y, j, R) % R * norm % R
            Lx = lincomb([Lx, poly_sub_const(of(k), M._eval_small(M._interpolate(rs.points, rs.evals[j]), u))], [1, c])
    Lx = lincomb([Lx, h], [1, -M._vanishing_at(super_points, u) * norm % R])
    hp = divide(Lx, [u])
    scalars, commitments = M.shplonk_accumulate(queries, y, v, u)
    assert len(commitments) == 6 and len(scalars) == 6 + 3
    dlogs = [O.eval_polynomial(of(k), s) for k in commitments] + [1, O.eval_polynomial(h, s), O.eval_polynomial(hp, s)]
    left = sum(a * b for a, b in zip(scalars, dlogs)) % R
    assert left == s * O.eval_polynomial(hp, s) % R                              # e(Lc + u H', g2) = e(H', [s]_2)
    bad = [M.VerifierQuery(q.point, q.commitment, q.eval) for q in queries]
    bad[2].eval = (bad[2].eval + 1) % R
    scalars_bad, _ = M.shplonk_accumulate(bad, y, v, u)
    assert sum(a * b for a, b in zip(scalars_bad, dlogs)) % R != left
    scalars_bad, _ = M.shplonk_accumulate(queries, y, v, (u + 1) % R)
    assert sum(a * b for a, b in zip(scalars_bad, dlogs)) % R != s * O.eval_polynomial(hp, s) % R


def test_verifier_queries_group_like_prover_queries():
    """the set construction is the provers' own, keyed by the commitment's bytes"""
    qs = [M.VerifierQuery(5, tag(0), 1), M.VerifierQuery(7, tag(1), 2), M.VerifierQuery(5, tag(1), 3), M.VerifierQuery(7, tag(0).copy(), 4)]
    sets = M.construct_intermediate_sets(qs)
    assert [p for p, _ in sets] == [5, 7] and [[q.eval for q in g] for _, g in sets] == [[1, 3], [2, 4]]
    rsets, pts = M.construct_rotation_sets(qs)
    assert pts == [5, 7] and len(rsets) == 1 and rsets[0].polys == [key(0), key(1)] and rsets[0].evals == [[1, 4], [3, 2]]
    # equal commitments of different polynomials (two equal selector columns) are told apart by poly_id, as halo2 does by address
    same = [M.VerifierQuery(5, tag(0), 1, poly_id="a"), M.VerifierQuery(5, tag(0), 2, poly_id="b"), M.VerifierQuery(7, tag(0), 3, poly_id="a")]
    rsets, _ = M.construct_rotation_sets(same)
    assert [rs.polys for rs in rsets] == [["a"], ["b"]] and [rs.points for rs in rsets] == [[5, 7], [5]]
    assert [c.tolist() for c in M.commitment_points(same, ["b", "a"])] == [tag(0).tolist(), tag(0).tolist()]
    assert _lib.ZKHIP_MAX_PAIRS == 64


def test_a_changed_claim_cannot_hide_behind_a_repeated_query():
    """The plan's last query repeats (polynomial 0, point a).  The set construction keeps the FIRST evaluation of a (polynomial, point) pair, so a
    changed evaluation on the repetition would leave SHPLONK's scalars as they were: check_queries refuses it, for both verifiers, and likewise
    two commitments under one poly_id."""
    rng = random.Random(0x77E)
    polys, order = plan(rng)
    assert order[-1] == order[1]                                               # the repeated query
    y, v, u = (rng.randrange(1, R) for _ in range(3))
    queries = [M.VerifierQuery(z, tag(i), O.eval_polynomial(polys[i], z)) for i, z in order]
    M.check_queries(queries)                                                   # an agreeing repetition is fine
    scalars, _ = M.shplonk_accumulate(queries, y, v, u)
    bad = [M.VerifierQuery(q.point, q.commitment, q.eval) for q in queries]
    bad[-1].eval = (bad[-1].eval + 1) % R                                      # exactly the repetition
    sets_good, _ = M.construct_rotation_sets(queries)
    sets_bad, _ = M.construct_rotation_sets(bad)
    assert [rs.evals for rs in sets_bad] == [rs.evals for rs in sets_good]     # what the set construction alone would have let through
    for accumulate in (lambda q: M.shplonk_accumulate(q, y, v, u), lambda q: M.gwc_accumulate(q, 3, v, u)):
        with pytest.raises(M.InconsistentQueries):
            accumulate(bad)
    bad = [M.VerifierQuery(q.point, q.commitment, q.eval) for q in queries]
    bad[1].eval = (bad[1].eval + 1) % R                                        # the first of the two: the same conflict
    with pytest.raises(M.InconsistentQueries):
        M.shplonk_accumulate(bad, y, v, u)
    # with poly_id: one query of a polynomial opened several times carries another polynomial's commitment
    ided = [M.VerifierQuery(z, tag(i), O.eval_polynomial(polys[i], z), poly_id=i) for i, z in order]
    assert M.shplonk_accumulate(ided, y, v, u)[0] == scalars
    ided[7].commitment = tag(5)                                                # polynomial 4 is opened at a, b and c
    for accumulate in (lambda q: M.shplonk_accumulate(q, y, v, u), lambda q: M.gwc_accumulate(q, 3, v, u)):
        with pytest.raises(M.InconsistentQueries):
            accumulate(ided)
    # poly_id on some queries only: the keys are not comparable
    mixed = [M.VerifierQuery(z, tag(i), O.eval_polynomial(polys[i], z), poly_id=i if t else None) for t, (i, z) in enumerate(order)]
    with pytest.raises(ValueError) as err:
        M.shplonk_accumulate(mixed, y, v, u)
    assert not isinstance(err.value, M.InconsistentQueries)

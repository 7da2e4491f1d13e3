"""The quotient identity at x on Python integers: what `zkhip_verify_identity_device` and `evaluation.identity_program` are compared with.  A helper
module (no tests).  It walks the `ConstraintSystem` and its `Expr` trees directly -- none of `Graph`, `compile_graph`, `RowProgram` or
`_evaluate_h_terms` is used -- in the order of [DEP] halo2-axiom plonk/verifier.rs `verify_proof`: the gates' polynomials, the permutation
argument's expressions (plonk/permutation/verifier.rs `Evaluated::expressions`), each lookup's five (plonk/lookup/verifier.rs), folded with y,
against h(x) (x^n - 1).  The domain values are the Lagrange basis by its defining property on the domain and by the closed form off it."""
from zksnap_circuits_halo2_amd import fields as F

R = F.R_MOD
DELTA = pow(7, 1 << 28, R)                     # generator of the cosets the permutation columns are told apart by (7 generates Fr*, 2-adicity 28)
STATUS_HOLDS, STATUS_FAILS, STATUS_IN_DOMAIN = 0, 1, 2


def inv(a):
    return pow(a % R, R - 2, R)


def lagrange(i, x, k):
    """l_i(x) over the domain of 2^k rows: 1 at omega^i, 0 at the other powers of omega, omega^i (x^n - 1) / (n (x - omega^i)) elsewhere"""
    n, w = 1 << k, pow(F.omega_for(k), i, R)
    if pow(x, n, R) == 1:
        return 1 if x % R == w else 0
    return w * (pow(x, n, R) - 1) % R * inv(n * (x - w)) % R


def domain_values(x, k, u):
    """(x^n, l_0, l_last, l_active, x in the domain) with l_last = l_u and l_active = 1 - l_last - sum_{i > u} l_i"""
    n = 1 << k
    l_last = lagrange(u, x, k)
    blind = sum(lagrange(i, x, k) for i in range(u + 1, n)) % R
    return pow(x, n, R), lagrange(0, x, k), l_last, (1 - l_last - blind) % R, pow(x, n, R) == 1


def device_domain_values(x, k, u):
    """what the library writes: the four values, zeros for a point of the domain"""
    xn, l0, l_last, l_active, inside = domain_values(x, k, u)
    return (0, 0, 0, 0) if inside else (xn, l0, l_last, l_active)


def evaluate(e, at):
    """an Expr over at(kind, index, rotation)"""
    if e.kind == "constant":
        return e.a % R
    if e.kind in ("fixed", "advice", "instance"):
        return at(e.kind, e.a, e.b or 0)
    if e.kind == "neg":
        return -evaluate(e.a, at) % R
    if e.kind == "sum":
        return (evaluate(e.a, at) + evaluate(e.b, at)) % R
    if e.kind == "product":
        return evaluate(e.a, at) * evaluate(e.b, at) % R
    if e.kind == "scaled":
        return evaluate(e.a, at) * e.b % R
    raise ValueError(e.kind)


def _terms(cs, at, theta, beta, gamma, x, l0, l_last, l_active):
    terms = [evaluate(poly, at) for polys in cs.gates for poly in polys]
    sets, chunk = cs.num_permutation_sets, cs.chunk_len
    if cs.permutation_columns:
        z = lambda s, rot=0: at("perm", s, rot)
        terms.append(l0 * (1 - z(0)) % R)
        terms.append(l_last * (z(sets - 1) ** 2 - z(sets - 1)) % R)
        terms += [l0 * (z(s) - z(s - 1, -(cs.blinding_factors + 1))) % R for s in range(1, sets)]
        for s in range(sets):
            left, right = z(s, 1), z(s)
            for j, (kind, idx) in enumerate(cs.permutation_columns[s * chunk:(s + 1) * chunk]):
                v = at(kind, idx, 0)
                left = left * (v + beta * at("sigma", s * chunk + j, 0) + gamma) % R
                right = right * (v + pow(DELTA, s * chunk + j, R) * beta * x + gamma) % R
            terms.append(l_active * (left - right) % R)
    for li, lk in enumerate(cs.lookups):
        compress = lambda exprs: sum(evaluate(e, at) * pow(theta, len(exprs) - 1 - i, R) for i, e in enumerate(exprs)) % R
        zl, zl_next = at("lookup_z", li, 0), at("lookup_z", li, 1)
        a, a_prev, s_ = at("lookup_pa", li, 0), at("lookup_pa", li, -1), at("lookup_ps", li, 0)
        terms.append(l0 * (1 - zl) % R)
        terms.append(l_last * (zl * zl - zl) % R)
        terms.append(l_active * (zl_next * (a + beta) * (s_ + gamma) - zl * (compress(lk.input_expressions) + beta) * (compress(lk.table_expressions) + gamma)) % R)
        terms.append(l0 * (a - s_) % R)
        terms.append(l_active * (a - s_) * (a - a_prev) % R)
    return terms


def _opening(plan, k, evals):
    n = 1 << k
    slot = {}
    for (kind, idx, rot), e in zip(plan, evals):
        slot.setdefault((kind, idx, rot % n), e % R)
    return lambda kind, idx, rot=0: slot[(kind, idx, rot % n)]


def expected_quotient(cs, plan, k, evals, challenges):
    """the y-fold of every term at x (the left-hand side of the identity), x outside the domain"""
    theta, beta, gamma, y, x = challenges
    _, l0, l_last, l_active, inside = domain_values(x, k, (1 << k) - (cs.blinding_factors + 1))
    assert not inside
    acc = 0
    for t in _terms(cs, _opening(plan, k, evals), theta, beta, gamma, x, l0, l_last, l_active):
        acc = (acc * y + t) % R
    return acc


def identity_value(cs, plan, k, evals, challenges):
    """0 exactly when the identity holds: the fold minus (h_0 + x^n h_1 + x^2n h_2)(x^n - 1)"""
    at, xn = _opening(plan, k, evals), pow(challenges[4], 1 << k, R)
    h = (at("h", 0) + xn * at("h", 1) + xn * xn * at("h", 2)) % R
    return (expected_quotient(cs, plan, k, evals, challenges) - h * (xn - 1)) % R


def status(cs, plan, k, evals, challenges):
    if pow(challenges[4], 1 << k, R) == 1:
        return STATUS_IN_DOMAIN
    return STATUS_HOLDS if identity_value(cs, plan, k, evals, challenges) == 0 else STATUS_FAILS


def solve_h0(cs, plan, k, evals, challenges):
    """`evals` with the evaluation of h_0 replaced so that the identity holds (x outside the domain): the identity is linear in it"""
    at, xn = _opening(plan, k, evals), pow(challenges[4], 1 << k, R)
    h0 = (expected_quotient(cs, plan, k, evals, challenges) * inv(xn - 1) - xn * at("h", 1) - xn * xn * at("h", 2)) % R
    out = list(evals)
    out[plan.index(("h", 0, 0))] = h0
    return out


def report(statuses):
    bad = [i for i, s in enumerate(statuses) if s != 0]
    return len(bad), (bad[0] if bad else (1 << 64) - 1)

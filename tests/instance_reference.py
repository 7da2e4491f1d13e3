"""Instance columns at x on Python integers: what `zkhip_fr_instance_evals_device`, `zkhip_verify_identity_instances_device`, csrc/instance_evals.hpp
and `evaluation.identity_program(..., instance_queries=...)` are compared with.  A helper module (no tests).  The evaluation is the defining sum
over `identity_reference.lagrange` -- one closed-form Lagrange value per public input, each with an inversion of its own -- never the running
fraction the library carries.  The identity is `identity_reference._terms` with `at("instance", c, r)` answered by that sum."""
import identity_reference as IR

R = IR.R


def evaluation(values, rot, x, k):
    """sum_i values[i] l_((i - rot) mod n)(x): the instance polynomial (zeros behind the values) at x omega^rot"""
    n = 1 << k
    assert len(values) <= n
    return sum(v * IR.lagrange((i - rot) % n, x, k) for i, v in enumerate(values)) % R


def device_evaluation(values, rot, x, k):
    """what the library writes: zero for a point of the domain, where it divides nothing"""
    return 0 if pow(x, 1 << k, R) == 1 else evaluation(values, rot, x, k)


def evaluations(instances, queries, xs, k):
    """e[q][p] for instances[p][c] = the values of column c of proof p, queries = (column, rotation) pairs, xs[p] the points"""
    return [[device_evaluation(instances[p][c], rot, xs[p], k) for p in range(len(xs))] for c, rot in queries]


def _at(plan, k, evals, instances, x):
    opened = IR._opening(plan, k, evals)
    return lambda kind, idx, rot=0: evaluation(instances[idx], rot, x, k) if kind == "instance" else opened(kind, idx, rot)


def expected_quotient(cs, plan, k, evals, challenges, instances):
    theta, beta, gamma, y, x = challenges
    _, l0, l_last, l_active, inside = IR.domain_values(x, k, (1 << k) - (cs.blinding_factors + 1))
    assert not inside
    acc = 0
    for t in IR._terms(cs, _at(plan, k, evals, instances, x), theta, beta, gamma, x, l0, l_last, l_active):
        acc = (acc * y + t) % R
    return acc


def identity_value(cs, plan, k, evals, challenges, instances):
    """0 exactly when the identity holds for these public inputs (instances[c] = the values of column c)"""
    at, xn = IR._opening(plan, k, evals), pow(challenges[4], 1 << k, R)
    h = (at("h", 0) + xn * at("h", 1) + xn * xn * at("h", 2)) % R
    return (expected_quotient(cs, plan, k, evals, challenges, instances) - h * (xn - 1)) % R


def status(cs, plan, k, evals, challenges, instances):
    if pow(challenges[4], 1 << k, R) == 1:
        return IR.STATUS_IN_DOMAIN
    return IR.STATUS_HOLDS if identity_value(cs, plan, k, evals, challenges, instances) == 0 else IR.STATUS_FAILS


def solve_h0(cs, plan, k, evals, challenges, instances):
    """`evals` with the evaluation of h_0 replaced so that the identity holds (x outside the domain)"""
    at, xn = IR._opening(plan, k, evals), pow(challenges[4], 1 << k, R)
    h0 = (expected_quotient(cs, plan, k, evals, challenges, instances) * IR.inv(xn - 1) - xn * at("h", 1) - xn * xn * at("h", 2)) % R
    out = list(evals)
    out[plan.index(("h", 0, 0))] = h0
    return out

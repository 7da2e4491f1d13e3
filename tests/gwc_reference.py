"""The batch verifier's scalar rows on Python integers (a helper module: no tests, no fixtures).  The GWC rows are `multiopen.gwc_accumulate` over
`verifier.verifier_queries`, that function's per-query scalars summed per polynomial and laid out as include/zkhip.h lays out a row; a fold is the
plain sum.  tests/test_gwc_fold_host.py and the GPU tests of the two calls share it."""
import numpy as np

from zksnap_circuits_halo2_amd import evaluation as E, fields as F, multiopen as MO, prover as P, verifier as V

R = F.R_MOD
SHAPES = [(1, 1, 7), (3, 2, 7), (256, 8, 13)]                 # (gate columns, lookups, k); the last is the voter's shape
_NOTHING = np.zeros(12, dtype=np.uint64)                       # the accumulation groups by poly_id and reads no commitment


def plan_for(gate_cols, lookups, k, order="halo2", random_poly=False):
    cs = E.halo2_lib_shape(gate_cols, lookups)
    return P.opening_plan(cs, gate_cols, lookups, (1 << k) - (cs.blinding_factors + 1), random_poly, order)


def queries_of(triples, evals, x, k):
    return V.verifier_queries(triples, {(kind, idx): _NOTHING for kind, idx, _ in triples}, evals, x, k)


def gwc_rows(triples, gp, k, evals, x, v, u):
    """-> (row of A over [W_0 .. | slots | G], row of C) of one proof, integers"""
    left, right, polys = MO.gwc_accumulate(queries_of(triples, evals, x, k), gp.n_sets, v, u)
    row = right[:gp.n_sets] + [0] * gp.n_slots + [right[-1]]
    slot = {key: i for i, key in enumerate(gp.own_keys + gp.shared_keys)}
    for key, s in zip(polys, right[gp.n_sets:-1]):
        row[gp.n_sets + slot[key]] = (row[gp.n_sets + slot[key]] + s) % R
    return row, left


def fold(rows, n_own, r, negate):
    """-> (out_own as a list of rows, out_shared) of zkhip_fr_fold_rows_device over integer rows"""
    sign = R - 1 if negate else 1
    n_cols = len(rows[0]) if rows else n_own
    own = [[sign * ri * a % R for a in row[:n_own]] for ri, row in zip(r, rows)]
    shared = [sign * sum(ri * row[j] for ri, row in zip(r, rows)) % R for j in range(n_own, n_cols)]
    return own, shared


def pick(rng, n):
    """n elements drawn from {0, 1, r - 1, random}"""
    return [rng.choice([0, 1, R - 1, rng.randrange(R), rng.randrange(R)]) for _ in range(n)]

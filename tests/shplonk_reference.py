"""The batch verifier's SHPLONK rows on Python integers (a helper module: no tests, no fixtures).  A row is `multiopen.shplonk_accumulate` over
`verifier.verifier_queries`, laid out as include/zkhip.h lays out a row of zkhip_shplonk_scalars_device: [H', H | own polynomials | key polynomials
| G] -- what verifier._fold_openings built on the host before that call existed.  The reference is the host function, never the code under test.
tests/test_shplonk_fold_host.py and the GPU tests of the call share it."""
import gwc_reference as GR
from zksnap_circuits_halo2_amd import fields as F, multiopen as MO

R = F.R_MOD


def shplonk_rows(triples, sp, k, evals, x, y, v, u):
    """-> (row of A over [H', H | slots | G], row of C) of one proof, integers; sp: the plan's ShplonkPlan (for the order of the slots)"""
    scalars, keys = MO.shplonk_accumulate(GR.queries_of(triples, evals, x, k), y, v, u)
    by_key = {}
    for key, s in zip(keys, scalars):
        by_key[key] = (by_key.get(key, 0) + s) % R
    g_scalar, h_scalar, hp_scalar = scalars[len(keys):]
    return [hp_scalar, h_scalar] + [by_key[key] for key in sp.own_keys + sp.shared_keys] + [g_scalar], [1]


"""CPU: the opening plan of the halo2-lib shape (zksnap_circuits_halo2_amd/prover.py: opening_plan) -- no device, no library call."""
import pytest

from zksnap_circuits_halo2_amd import evaluation as E
from zksnap_circuits_halo2_amd.prover import BLIND, opening_plan


def plans(gate_cols, lookups, k=7, **kw):
    cs, u = E.halo2_lib_shape(gate_cols, lookups, BLIND), (1 << k) - (BLIND + 1)
    return u, opening_plan(cs, gate_cols, lookups, u, order="halo2", **kw), opening_plan(cs, gate_cols, lookups, u, order="seeded", **kw)


def test_halo2_order_of_one_gate_column_and_one_lookup():
    u, halo2, _ = plans(1, 1)
    assert halo2 == [
        ("advice", 0, 0), ("advice", 0, 1), ("advice", 0, 2), ("advice", 0, 3),      # the gate column: the vertical gate reads four rows
        ("advice", 1, 0),                                                            # the lookup input
        ("fixed", 0, 0), ("fixed", 1, 0), ("fixed", 2, 0),                           # selector, constants, table
        ("sigma", 0, 0), ("sigma", 1, 0), ("sigma", 2, 0),
        ("perm", 0, 0), ("perm", 0, 1), ("perm", 0, u),                              # z(x), z(omega x), and the chaining row of all but the last set
        ("perm", 1, 0), ("perm", 1, 1),
        ("lookup_z", 0, 0), ("lookup_z", 0, 1), ("lookup_pa", 0, 0), ("lookup_pa", 0, -1), ("lookup_ps", 0, 0),
        ("h", 0, 0), ("h", 1, 0), ("h", 2, 0)]
    assert len(halo2) == 24


@pytest.mark.parametrize("gate_cols,lookups", [(1, 1), (3, 2), (2, 0)])
def test_seeded_order_is_a_permutation_of_halo2_order(gate_cols, lookups):
    _, halo2, seeded = plans(gate_cols, lookups)
    assert len(set(halo2)) == len(halo2) and sorted(seeded) == sorted(halo2)
    assert seeded[0] == ("fixed", 0, 0) and halo2[0] == ("advice", 0, 0)              # and not the same order


@pytest.mark.parametrize("order", [0, 1])
def test_random_polynomial_adds_one_opening(order):
    without, with_ = plans(3, 2)[1 + order], plans(3, 2, random_poly=True)[1 + order]
    assert [t for t in with_ if t not in without] == [("random", 0, 0)] and [t for t in with_ if t != ("random", 0, 0)] == without
    if order == 0:
        assert with_[with_.index(("random", 0, 0)) - 1][0] == "fixed" and with_[with_.index(("random", 0, 0)) + 1][0] == "sigma"      # halo2: between fixed and sigma


def test_unknown_order():
    with pytest.raises(ValueError):
        opening_plan(E.halo2_lib_shape(1, 1, BLIND), 1, 1, 122, order="other")

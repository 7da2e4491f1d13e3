"""The closed forms and solved cells of tests/argument_cases.py, pinned on the CPU before a GPU sees them: every family against the
recurrence written out in Python integers at k <= 5, the limbs of the two all-ones words, the zero factors at the cells they name, and
the share of edge-word combinations the reference itself rules out."""
import itertools

import pytest

import argument_cases as AC
from oracle import bn254 as O

R = AC.R
BETA, GAMMA = AC.CHALLENGES["seeded"], AC.CONSTANTS["seeded"]


def halo2_products(values, sigmas, chunk, k, usable, beta, gamma):
    """the reference's loop itself, on field values: the sets chained through z[usable] (usable < n)"""
    n, omega = 1 << k, O.omega_for(k)
    vals, sig = [[AC.dec(w) for w in c] for c in values], [[AC.dec(w) for w in c] for c in sigmas]
    beta, gamma = AC.dec(beta), AC.dec(gamma)
    out, last = [], 1
    for lo in range(0, len(vals), chunk):
        z = [last]
        for i in range(n - 1):
            if i < usable:
                a = b = 1
                for c in range(lo, min(lo + chunk, len(vals))):
                    a = a * (vals[c][i] + pow(O.FR_DELTA, c, R) * beta % R * pow(omega, i, R) + gamma) % R
                    b = b * (vals[c][i] + beta * sig[c][i] + gamma) % R
                z.append(z[-1] * a % R * pow(b, -1, R) % R if b else 0)
            else:
                z.append(z[-1])
        last = z[usable]
        out.append([AC.enc(x) for x in z])
    return out


def usables(n):
    return sorted({u for u in (0, 1, n - 1, n, n - 6) if 0 <= u <= n})


def test_constants_are_the_words_the_issue_names():
    c = AC.CONSTANTS
    assert [AC.dec(c[k]) for k in ("enc0", "enc1", "enc_r_minus_1")] == [0, 1, R - 1]
    assert c["raw1"] == 1 and c["raw_r_minus_1"] == R - 1
    w0, w5 = c["raw_low_limbs_full"], c["raw_low_limbs_full_5"]
    assert w0 < R and w0 + 1 == (R >> 232) << 232 and w5 < R and w5 + 1 == (R >> 227) << 227
    assert AC.limbs(w0)[:8] == [2**29 - 1] * 8
    assert AC.limbs(w5, 5)[0] == 0x1FFFFFE0 and AC.limbs(w5, 5)[1:8] == [2**29 - 1] * 7
    assert sum(l << (29 * i) for i, l in enumerate(AC.limbs(w5, 5))) == w5 << 5           # nine limbs hold the whole shifted word
    assert len(c) == 8 and 1 < c["seeded"] < R - 1
    ch = AC.CHALLENGES
    assert {0, 1, R - 1, R - 2, AC.SEEDED_CHALLENGE} <= set(ch.values())
    assert {AC.dec(w) for w in ch.values()} >= {0, 1, R - 1, R - 2}
    assert {0, 1, R - 1, AC.SEEDED_CHALLENGE} <= set(AC.LOOKUP_CHALLENGES.values())
    assert AC.ints(AC.words(list(c.values()))) == list(c.values())


@pytest.mark.parametrize("k,n_columns,chunk", [(5, 5, 2), (3, 4, 4), (2, 3, 1), (0, 3, 2), (1, 2, 5)])
def test_perm_naive_is_the_reference_loop(k, n_columns, chunk):
    n = 1 << k
    values, sigmas = AC.perm_seeded(11 * k + chunk, n_columns, k, AC.edge_overrides(n_columns, k))
    for u in usables(n):
        got = AC.perm_naive(values, sigmas, chunk, k, u, BETA, GAMMA)
        if u < n:
            assert got == halo2_products(values, sigmas, chunk, k, u, BETA, GAMMA), u
        else:                                      # no row z[n]: set 0 is the loop's, a later set starts from the product over all n rows
            ref = halo2_products(values, sigmas, chunk, k, n - 1, BETA, GAMMA)
            assert got[0] == ref[0]
            num, den = AC.perm_factors(values, sigmas, k, BETA, GAMMA)
            start = 1
            for s in range(AC.set_count(n_columns, chunk)):
                assert AC.dec(got[s][0]) == start, s
                for c in range(s * chunk, min((s + 1) * chunk, n_columns)):
                    for i in range(n):
                        start = start * num[c][i] % R * pow(den[c][i], -1, R) % R


@pytest.mark.parametrize("k,n_columns,chunk", [(5, 5, 2), (4, 9, 1), (3, 4, 4), (1, 5, 4), (0, 2, 1)])
def test_perm_closed_forms_equal_the_recurrence(k, n_columns, chunk):
    n = 1 << k
    consts = (list(AC.CONSTANTS.values()) * 2)[:n_columns]
    for u in usables(n):
        for beta, gamma in ((BETA, GAMMA), (AC.CHALLENGES["raw1"], 0), (AC.CHALLENGES["enc_r_minus_2"], AC.CHALLENGES["raw_r_minus_1"])):
            case = AC.perm_identity(k, n_columns, chunk, k, u, beta, gamma)
            assert case.expected == AC.perm_naive(case.values, case.sigmas, chunk, k, u, beta, gamma), ("identity", u)
            assert all(w == AC.enc(1) for z in case.expected for w in z)
            case = AC.perm_rotation(consts, chunk, k, u, beta, gamma)
            assert case.expected == AC.perm_naive(case.values, case.sigmas, chunk, k, u, beta, gamma), ("rotation", u)
            assert all(len(z) == n for z in case.expected) and len(case.expected) == AC.set_count(n_columns, chunk)


@pytest.mark.parametrize("solve", ["den", "num"])
def test_perm_zero_cells_are_zero_factors_where_they_say(solve):
    k, n_columns, chunk = 5, 5, 2
    n, u = 1 << k, (1 << k) - 6
    base = AC.perm_naive_case(3, n_columns, chunk, k, u, BETA, GAMMA)
    assert all(w for z in base.expected for w in z)
    for cells in ([(0, 0)], [(0, u - 1)], [(2, 0)], [(2, u - 1)], [(1, 7)], [(0, 9), (2, 3)], [(1, 4), (1, 20)]):
        if solve == "den":
            case = AC.perm_zero_den(base, cells, chunk, k, BETA, GAMMA)
        else:
            case = AC.perm_zero_num(base, cells, chunk, k, u, BETA, GAMMA)
        num, den = AC.perm_factors(case.values, case.sigmas, k, BETA, GAMMA)
        factors = den if solve == "den" else num
        zeros = {(c, i) for c in range(n_columns) for i in range(n) if factors[c][i] == 0}
        assert zeros == {(s * chunk, row) for s, row in cells}                         # a zero factor exactly at the cells named
        assert not any(0 in col for col in (num if solve == "den" else den))
        assert case.expected == AC.perm_naive(case.values, case.sigmas, chunk, k, u, BETA, GAMMA), cells
        s0, r0 = min(cells)
        flat, first = list(itertools.chain(*case.expected)), s0 * n + r0
        assert flat[:first + 1] == list(itertools.chain(*base.expected))[:first + 1] and all(flat[:first + 1])
        assert not any(flat[first + 1:]) and len(flat) > first + 1


def test_perm_edge_grid_skips_at_most_one_combination_in_ten():
    total = skipped = 0
    for fill in AC.EDGE_FILLS:
        values, sigmas = AC.perm_edge_fill(fill)
        assert len(values) == len(sigmas) == AC.EDGE_COLUMNS and all(len(c) == 1 << AC.EDGE_K for c in values + sigmas)
        assert all(w in AC.CONSTANTS.values() for c in values + sigmas for w in c)
        if fill in AC.CONSTANTS:
            assert {w for c in values + sigmas for w in c} == {AC.CONSTANTS[fill]}
        else:
            assert {w for c in values + sigmas for w in c} == set(AC.CONSTANTS.values())
        for chunk in AC.EDGE_CHUNKS:
            combos = AC.perm_edge_combinations(fill, chunk)
            assert len(combos) == len(AC.CHALLENGES) ** 2
            for bn, gn, skip in combos:
                _, den = AC.perm_factors(values, sigmas, AC.EDGE_K, AC.CHALLENGES[bn], AC.CHALLENGES[gn])
                assert skip == any(den[c][0] == 0 for c in range(min(chunk, AC.EDGE_COLUMNS))), (fill, chunk, bn, gn)
                total, skipped = total + 1, skipped + skip
    assert total == len(AC.EDGE_FILLS) * len(AC.EDGE_CHUNKS) * 64
    assert 10 * skipped <= total, (skipped, total)
    for fill in ("mixed_3", "mixed_7"):                     # the seeded fills alone meet the cap too
        flags = [s for chunk in AC.EDGE_CHUNKS for _, _, s in AC.perm_edge_combinations(fill, chunk)]
        assert 10 * sum(flags) <= len(flags), fill


@pytest.mark.parametrize("k", [0, 1, 4, 5])
def test_lookup_closed_forms_equal_the_grand_product(k):
    n = 1 << k
    for u in sorted({0, 1, n - 1, n}):
        for beta, gamma in itertools.product(AC.LOOKUP_CHALLENGES.values(), (GAMMA, 0)):
            case = AC.lookup_same(5 * k, k, u, beta, gamma)
            assert case.expected == AC.lookup_naive(case.a, case.s, case.ap, case.sp, u, beta, gamma), ("same", u)
            case = AC.lookup_shift(5 * k, k, u, beta, gamma)
            assert case.expected == AC.lookup_naive(case.a, case.s, case.ap, case.sp, u, beta, gamma), ("shift", u)
            assert case.ap == case.a[1:] + case.a[:1] and case.sp == case.s


def test_lookup_edge_columns_and_zero_denominators():
    k, u = 5, 26
    for (bn, beta), (gn, gamma) in itertools.product(AC.LOOKUP_CHALLENGES.items(), repeat=2):
        cols = AC.lookup_edge_columns(77, k, beta, gamma)
        assert all(w in AC.CONSTANTS.values() for c in cols for w in c)
        base = AC.lookup_naive_case(*cols, u, beta, gamma)
        assert all(base.expected), (bn, gn)                                  # no factor is zero: every row says something
        for row, through in itertools.product((0, 9, u - 1), "as"):
            case = AC.lookup_zero_den(base, row, through, beta, gamma)
            hit = case.ap[row] if through == "a" else case.sp[row]
            assert (AC.dec(hit) + AC.dec(beta if through == "a" else gamma)) % R == 0
            assert case.expected == AC.lookup_naive(case.a, case.s, case.ap, case.sp, u, beta, gamma)
            assert case.expected[:row + 1] == base.expected[:row + 1] and not any(case.expected[row + 1:])


def test_lincomb_expected_is_the_sum_written_out():
    n = 3
    bufs = [AC.constant_words(9 + b, n) for b in range(4)]
    columns = [bufs[j % 4] for j in range(11)]
    coeffs = AC.random_words(5, 9) + [0, AC.enc(R - 1)]
    direct = [sum(AC.dec(c) * col[i] for c, col in zip(coeffs, columns)) % R for i in range(n)]
    assert AC.lincomb_expected(coeffs, columns) == direct
    assert AC.lincomb_expected([AC.enc(1)] * 5, [[R - 1] * n] * 5) == [(R - 5) % R] * n


def test_fe_mul_model_and_the_input_that_needs_the_carry_propagation():
    import random

    rng = random.Random(29)
    for _ in range(200):                            # the model is the Montgomery product, below 2p, inside 64 bits on canonical operands
        a, b = rng.randrange(R), rng.randrange(R)
        limbs, peak = AC.fe_mul_model(AC.fe_limbs(a), AC.fe_limbs(b))
        assert AC.fe_value(limbs) % R == a * b * pow(1 << 261, -1, R) % R and AC.fe_value(limbs) < 2 * R and peak < 1 << 64
    beta, gamma, word = AC.perm_unnormalised_product_input()
    assert 0 < beta < R and 0 < gamma < R and word == AC.CONSTANTS["raw_low_limbs_full_5"]
    a, b = AC.perm_numerator_factor(word, 0, beta, gamma), AC.perm_numerator_factor(word, 1, beta, gamma)
    assert a[1:8] == [3 * (2**29 - 1)] * 7 and a[0] == 0x1FFFFFE0 + 2 * (2**29 - 1)
    for c, f in enumerate((a, b)):                  # the limbs add up to the factor itself
        assert AC.fe_value(f) % R == (word + AC.dec(beta) * pow(AC.DELTA, c, R) % R * (1 << 256) + gamma) * 32 % R
    raw, peak_raw = AC.fe_mul_model(a, b)
    kept, peak_kept = AC.fe_mul_model(AC.fe_limbs(AC.fe_value(a)), b)
    assert peak_raw >= 1 << 64 > peak_kept
    assert AC.fe_value(kept) % R == AC.fe_value(a) * AC.fe_value(b) * pow(1 << 261, -1, R) % R != AC.fe_value(raw) % R

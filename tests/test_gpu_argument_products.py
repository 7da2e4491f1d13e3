"""GPU (-m gpu): the three prover calls of csrc/poly.hip that run on lazily reduced values -- zkhip_permutation_products[_device]
(k_perm_den, k_perm_num_mul, one batch inversion, one flat prefix product), zkhip_lookup_products_device (k_lookup_den, k_lookup_num_mul,
the per-lookup prefix product) and zkhip_fr_linear_combination_device (k_lincomb, k_sum_columns) -- on the words and shapes their
magnitude comments are worst-case statements about: words whose 29-bit limbs are all ones, r - 1, the encodings of 0, 1 and r - 1 in
every cell and as beta and gamma; log_n from 0, usable_rows 0 and n, a chunk longer than the column list; zero factors at the ends of
the usable rows and of the set list; and the column counts at which the linear combination adds a group, a normalisation or a reduction.

Every expectation comes from tests/argument_cases.py (Python integers; pinned on the CPU by tests/test_argument_cases_host.py), none from
the library.  Comparisons are of whole arrays of canonical words, with no tolerance.  Every device output lies between two guards of 8
elements, is filled with 0xA5 bytes first, and the guards must hold the fill afterwards."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import argument_cases as AC
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, evaluation as E

pytestmark = pytest.mark.gpu

R = AC.R
DEV = torch.device("cuda", 0)
GUARD = 8
FILL = 0xA5A5A5A5A5A5A5A5 - (1 << 64)             # 0xA5 in every byte, as the int64 the tensors hold
HOST_FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
BETA, GAMMA = AC.CHALLENGES["seeded"], AC.CONSTANTS["seeded"]


# ---------------------------------------------------------------- plumbing
def dev(column):
    """a list of words -> an (n, 4) int64 device tensor"""
    return torch.from_numpy(AC.words(column).view(np.int64)).to(DEV)


def dev_columns(columns):
    """[column][row] words -> the columns as rows of ONE upload"""
    n = len(columns[0])
    flat = dev([w for col in columns for w in col])
    return [flat[c * n:(c + 1) * n] for c in range(len(columns))]


class Guarded:
    """`elems` elements of device memory between two guards, every byte 0xA5: an element the call never wrote cannot pass"""

    def __init__(self, elems):
        self.elems = elems
        self.t = torch.full((GUARD + elems + GUARD, 4), FILL, dtype=torch.int64, device=DEV)

    @property
    def body(self):
        return self.t[GUARD:GUARD + self.elems]

    def ptr(self):
        return self.t.data_ptr() + 32 * GUARD

    def words(self, what=""):
        """the body as (elems, 4) uint64 on the host, after checking both guards"""
        h = self.t.cpu()
        assert bool((h[:GUARD] == FILL).all()) and bool((h[GUARD + self.elems:] == FILL).all()), f"{what}: an element outside the output was written"
        return h[GUARD:GUARD + self.elems].numpy().view(np.uint64)


def same(got, expected, what=""):
    """word-for-word equality of a (rows, 4) array with a list of words, reporting the first rows that differ"""
    exp = AC.words(expected)
    got = np.asarray(got).reshape(-1, 4)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        pytest.fail(f"{what}: {bad.size} of {got.shape[0]} rows differ, first at {bad[:8].tolist()}")


def flat(expected):
    return list(itertools.chain(*expected))


def word(w):
    return AC.words([w])[0]


def perm_consts(k, beta, gamma):
    return [word(w) for w in (beta, gamma, AC.enc(AC.DELTA), AC.enc(O.omega_for(k)))]


def perm_launch(lib, d_values, d_sigmas, chunk, k, usable, beta, gamma, out, stream=None):
    m = len(d_values)
    vp, sp = (C.c_void_p * m)(*[t.data_ptr() for t in d_values]), (C.c_void_p * m)(*[t.data_ptr() for t in d_sigmas])
    consts = perm_consts(k, beta, gamma)
    _lib.check(lib.zkhip_permutation_products_device(vp, sp, m, chunk, k, usable, *[c.ctypes.data for c in consts], out.ptr(), stream))


def perm_device(lib, d_values, d_sigmas, chunk, k, usable, beta, gamma, what=""):
    """one device call on uploaded columns -> z as ([sets * n], 4) words"""
    out = Guarded(AC.set_count(len(d_values), chunk) << k)
    perm_launch(lib, d_values, d_sigmas, chunk, k, usable, beta, gamma, out)
    torch.cuda.synchronize()
    return out.words(what)


def perm_host(lib, values, sigmas, chunk, k, usable, beta, gamma, what=""):
    m, elems = len(values), AC.set_count(len(values), chunk) << k
    V, S = [AC.words(c) for c in values], [AC.words(c) for c in sigmas]
    vp, sp = (C.c_void_p * m)(*[a.ctypes.data for a in V]), (C.c_void_p * m)(*[a.ctypes.data for a in S])
    z = np.full((GUARD + elems + GUARD, 4), HOST_FILL, dtype=np.uint64)
    consts = perm_consts(k, beta, gamma)
    _lib.check(lib.zkhip_permutation_products(vp, sp, m, chunk, k, usable, *[c.ctypes.data for c in consts], z.ctypes.data + 32 * GUARD))
    assert (z[:GUARD] == HOST_FILL).all() and (z[GUARD + elems:] == HOST_FILL).all(), f"{what}: an element outside the output was written"
    return z[GUARD:GUARD + elems]


def check_perm(lib, case, chunk, k, usable, beta, gamma, what, sets=None):
    n = 1 << k
    got = perm_device(lib, dev_columns(case.values), dev_columns(case.sigmas), chunk, k, usable, beta, gamma, what)
    sets = len(case.expected) if sets is None else sets
    same(got[:sets * n], flat(case.expected[:sets]), what)
    return got


def usables(n):
    return sorted({u for u in (0, 1, n - 1, n) + ((n - 6,) if n >= 8 else ()) if 0 <= u <= n})


# ---------------------------------------------------------------- 1. permutation products: edge words
@pytest.mark.parametrize("chunk", AC.EDGE_CHUNKS)
@pytest.mark.parametrize("fill", AC.EDGE_FILLS)
def test_perm_edge_words_in_every_cell_and_challenge(lib, fill, chunk):
    """k = 6, 5 columns: every cell the one constant (or every cell drawn from the constants), beta and gamma through every edge
    challenge; a combination is left out only when the reference's first denominator is zero (at most one in ten over the grid:
    tests/test_argument_cases_host.py)"""
    k, usable = AC.EDGE_K, (1 << AC.EDGE_K) - 6
    values, sigmas = AC.perm_edge_fill(fill)
    d_values, d_sigmas = dev_columns(values), dev_columns(sigmas)
    ran = skipped = 0
    for bn, gn, skip in AC.perm_edge_combinations(fill, chunk):
        if skip:
            skipped += 1
            continue
        beta, gamma = AC.CHALLENGES[bn], AC.CHALLENGES[gn]
        exp = AC.perm_naive(values, sigmas, chunk, k, usable, beta, gamma)
        same(perm_device(lib, d_values, d_sigmas, chunk, k, usable, beta, gamma), flat(exp), f"beta {bn}, gamma {gn}")
        ran += 1
    print(f"{fill}, chunk {chunk}: {ran} combinations compared, {skipped} skipped")
    assert ran + skipped == len(AC.CHALLENGES) ** 2 and ran


# ---------------------------------------------------------------- 2. permutation products: shapes
SHAPES = [(1, 1), (1, 4), (4, 4), (5, 4), (9, 1), (33, 3), (70, 1)]


@pytest.mark.parametrize("n_columns,chunk", SHAPES)
@pytest.mark.parametrize("k", [0, 1, 2, 3, 7, 8])
def test_perm_shapes_and_usable_rows(lib, k, n_columns, chunk):
    """log_n from 0 (odd and even splits of the omega table), usable_rows 0, 1, n - 1, n (and n - 6), one column, a chunk longer than
    the column list, a ragged last set, 70 sets; edge words at the first and last rows.  With usable_rows = n set 0 is the
    reference's; the later sets start from the product over all n rows, as include/zkhip.h says."""
    n = 1 << k
    values, sigmas = AC.perm_seeded(1000 * k + n_columns, n_columns, k, AC.edge_overrides(n_columns, k))
    d_values, d_sigmas = dev_columns(values), dev_columns(sigmas)
    for u in usables(n):
        exp = AC.perm_naive(values, sigmas, chunk, k, u, BETA, GAMMA)
        got = perm_device(lib, d_values, d_sigmas, chunk, k, u, BETA, GAMMA, f"usable {u}")
        same(got[:n], exp[0], f"usable {u}: set 0")
        same(got, flat(exp), f"usable {u}")
        z = got.reshape(len(exp), n, 4)
        for i in range(u + 1, n):                                      # the tail repeats z[u]
            assert np.array_equal(z[:, i], z[:, u]), (u, i)
        if u == 0:
            same(got, [AC.enc(1)] * len(got), "usable 0: all ones")


# ---------------------------------------------------------------- 3. permutation products: zero factors
@pytest.mark.parametrize("solve", ["den", "num"])
def test_perm_zero_factor_ends_the_product_there(lib, solve):
    """a zero denominator (num: numerator) at row 0, at row u - 1, in the first set, in the last set and in two sets at once: the rows
    up to it are those of the unchanged input, every row after it and every later set is 0"""
    k, n_columns, chunk = 6, 5, 2
    n, u, last = 1 << k, (1 << k) - 6, 2
    base = AC.perm_naive_case(0x2E20, n_columns, chunk, k, u, BETA, GAMMA)
    assert all(flat(base.expected))
    check_perm(lib, base, chunk, k, u, BETA, GAMMA, "no zero")
    for cells in ([(0, 0)], [(0, u - 1)], [(last, 0)], [(last, u - 1)], [(1, 17)], [(0, 40), (last, 3)], [(1, u - 1), (last, 0)]):
        if solve == "den":
            case = AC.perm_zero_den(base, cells, chunk, k, BETA, GAMMA)
        else:
            case = AC.perm_zero_num(base, cells, chunk, k, u, BETA, GAMMA)
        got = check_perm(lib, case, chunk, k, u, BETA, GAMMA, f"zero {solve} at {cells}")
        first = min(cells)[0] * n + min(cells)[1]
        same(got[:first + 1], flat(base.expected)[:first + 1], f"zero {solve} at {cells}: the rows before it")
        assert got[:first + 1].any(axis=1).all() and not got[first + 1:].any(), cells


def test_perm_numerator_factors_with_limbs_at_three_times_2p29(lib):
    """beta, gamma and the word at row 0 of columns 0 and 1 solved so that the first numerator factor's limbs are 3 (2^29 - 1) and the
    second's large enough for their product to overflow fe_mul's accumulator unless the first is carry-propagated
    (argument_cases.perm_unnormalised_product_input; the limbs are pinned in tests/test_argument_cases_host.py)"""
    k, n_columns = 6, 5
    u = (1 << k) - 6
    beta, gamma, w = AC.perm_unnormalised_product_input()
    for chunk in (2, 5):
        case = AC.perm_naive_case(0x3B29, n_columns, chunk, k, u, beta, gamma, [(0, 0, 0, w), (0, 1, 0, w)])
        assert all(flat(case.expected))
        check_perm(lib, case, chunk, k, u, beta, gamma, f"chunk {chunk}")


# ---------------------------------------------------------------- 4. permutation products: one larger closed form
BIG_K, BIG_COLUMNS = 16, 9                         # 9 * 2^16 elements: past 2^19, 8 elements per lane of the inversion, a five-level scan


def named_rows(n, u):
    rows = {0, 1, u - 1, u, u + 1, n - 1} | {(i * 257 + 3) % n for i in range(256)} | {15, 16, 17, 255, 256, 257, 4095, 4096, 4097}
    return sorted(r for r in rows if 0 <= r < n)


def test_perm_identity_at_2p16_is_all_ones(lib):
    k, n, u = BIG_K, 1 << BIG_K, (1 << BIG_K) - 6
    assert BIG_COLUMNS * n > 1 << 19
    values = [AC.constant_words(c, n) if c % 3 == 0 else AC.random_words(0x1DE0 + c, n) for c in range(BIG_COLUMNS)]
    case = AC.perm_identity(0, BIG_COLUMNS, 1, k, u, BETA, GAMMA, values=values)
    got = check_perm(lib, case, 1, k, u, BETA, GAMMA, "identity")
    assert np.array_equal(got, np.tile(word(AC.enc(1)), (BIG_COLUMNS * n, 1)))


def test_perm_rotation_at_2p16_equals_the_closed_form(lib):
    """whole, against one shared inversion in Python; and at 268 named rows per set against the closed form with an inversion each"""
    k, n, u = BIG_K, 1 << BIG_K, (1 << BIG_K) - 6
    consts = (list(AC.CONSTANTS.values()) + [AC.SEEDED_CHALLENGE])[:BIG_COLUMNS]
    case = AC.perm_rotation(consts, 1, k, u, BETA, GAMMA)
    got = check_perm(lib, case, 1, k, u, BETA, GAMMA, "rotation").reshape(BIG_COLUMNS, n, 4)
    rows = named_rows(n, u)
    assert len(rows) >= 256 and {0, 1, u - 1, u, u + 1, n - 1} <= set(rows)
    b, g, pw = AC.dec(BETA), AC.dec(GAMMA), AC.omega_powers(k)
    f = lambda j, i: (AC.dec(consts[j]) + b * pow(AC.DELTA, j, R) % R * pw[i] + g) % R
    start = 1
    for s in range(BIG_COLUMNS):                                       # chunk 1: set s is column s
        exp = [AC.enc(start * f(s, 0) % R * pow(f(s, min(i, u)), -1, R)) for i in rows]
        same(got[s][rows], exp, f"set {s} at the named rows")
        start = start * f(s, 0) % R * pow(f(s, u), -1, R) % R


# ---------------------------------------------------------------- 5. permutation products: forms of the call
FORM_SHAPES = [(0, 1, 4, 1), (3, 5, 4, 8), (7, 33, 3, 122)]          # (k, n_columns, chunk, usable_rows)


@pytest.mark.parametrize("k,n_columns,chunk,usable", FORM_SHAPES)
def test_perm_host_form_returns_the_device_forms_bytes(lib, k, n_columns, chunk, usable):
    case = AC.perm_naive_case(0xF0 + k, n_columns, chunk, k, usable, BETA, GAMMA, AC.edge_overrides(n_columns, k))
    got = check_perm(lib, case, chunk, k, usable, BETA, GAMMA, "device")
    host = perm_host(lib, case.values, case.sigmas, chunk, k, usable, BETA, GAMMA, "host")
    assert np.array_equal(host, got)
    same(host, flat(case.expected), "host")


def test_perm_three_queued_calls_on_one_stream(lib):
    """three calls back to back with no wait between them, over different column sets and challenges, the second one growing the
    stream's workspace: each call's pointer tables and constants are its own"""
    shapes = [(6, 5, 2, 58, BETA, GAMMA), (8, 33, 3, 250, AC.CHALLENGES["enc_r_minus_2"], BETA), (7, 9, 1, 128, GAMMA, AC.CHALLENGES["raw1"])]
    cases = [AC.perm_naive_case(0x3C0 + i, m, chunk, k, u, b, g, AC.edge_overrides(m, k)) for i, (k, m, chunk, u, b, g) in enumerate(shapes)]
    cols = [(dev_columns(c.values), dev_columns(c.sigmas)) for c in cases]
    outs = [Guarded(AC.set_count(m, chunk) << k) for k, m, chunk, u, b, g in shapes]
    torch.cuda.synchronize()
    for (k, m, chunk, u, b, g), (dv, ds), out in zip(shapes, cols, outs):
        perm_launch(lib, dv, ds, chunk, k, u, b, g, out)
    torch.cuda.synchronize()
    for i, (case, out) in enumerate(zip(cases, outs)):
        same(out.words(f"call {i}"), flat(case.expected), f"call {i}")


def test_perm_inputs_from_an_unsynchronised_kernel_on_a_side_stream(lib):
    """the columns are unmasked by a kernel enqueued on the side stream the call runs on, and nobody waits in between"""
    k, m, chunk = 10, 7, 2
    n, u = 1 << k, (1 << k) - 6
    case = AC.perm_naive_case(0x51DE, m, chunk, k, u, BETA, GAMMA, AC.edge_overrides(m, k))
    both = dev([w for col in case.values + case.sigmas for w in col])
    mask = torch.randint(-(1 << 62), 1 << 62, both.shape, dtype=torch.int64, device=DEV)
    masked = both ^ mask
    del both
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        cols = masked ^ mask                                           # produced on `side`, never waited for
        out = Guarded(AC.set_count(m, chunk) * n)
        d = [cols[c * n:(c + 1) * n] for c in range(2 * m)]
        perm_launch(lib, d[:m], d[m:], chunk, k, u, BETA, GAMMA, out, stream=side.cuda_stream)
    torch.cuda.synchronize()
    same(out.words("side stream"), flat(case.expected), "side stream")


# ---------------------------------------------------------------- 6. lookup products
def lookup_device(cases, k, usable, beta, gamma, what="", poison=False):
    """one call over the lookups `cases` -> z as (lookups, n, 4) words.  `poison`: the rows >= usable of a' and s' hold 0xFF bytes"""
    n, L = 1 << k, len(cases)
    inputs, tables = dev_columns([c.a for c in cases]), dev_columns([c.s for c in cases])
    pa = dev([w for c in cases for w in c.ap]).reshape(L, n, 4).contiguous()
    ps = dev([w for c in cases for w in c.sp]).reshape(L, n, 4).contiguous()
    if poison:
        pa[:, usable:] = -1
        ps[:, usable:] = -1
    out = Guarded(L * n)
    E.lookup_products_device(inputs, tables, pa, ps, usable, k, AC.dec(beta), AC.dec(gamma), z=out.body.view(L, n, 4))
    torch.cuda.synchronize()
    return out.words(what).reshape(L, n, 4)


def check_lookups(cases, k, usable, beta, gamma, what):
    n = 1 << k
    got = lookup_device(cases, k, usable, beta, gamma, what)
    if usable == 0:                                                    # usable_rows == 0 returns at once: nothing is written
        assert (got == HOST_FILL).all(), what
        return got
    for l, c in enumerate(cases):
        same(got[l], c.expected, f"{what}: lookup {l}")
    if usable < n:
        assert np.array_equal(lookup_device(cases, k, usable, beta, gamma, what, poison=True), got), f"{what}: rows >= usable_rows of a', s' were read"
    return got


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("bn", list(AC.LOOKUP_CHALLENGES))
def test_lookup_edge_words_in_every_column_and_challenge(lib, bn, L):
    """k = 6: a, s, a', s' drawn from the constants, beta and gamma through the edge challenges, against O.grand_product"""
    k, usable = 6, (1 << 6) - 6
    beta = AC.LOOKUP_CHALLENGES[bn]
    for gn, gamma in AC.LOOKUP_CHALLENGES.items():
        cases = [AC.lookup_naive_case(*AC.lookup_edge_columns(0x100 * l + 7, k, beta, gamma), usable, beta, gamma) for l in range(L)]
        assert all(all(c.expected) for c in cases)
        check_lookups(cases, k, usable, beta, gamma, f"beta {bn}, gamma {gn}")


@pytest.mark.parametrize("k", [1, 4, 5, 9])
def test_lookup_closed_forms(lib, k):
    """a' = a (z = 1) and a'[i] = a[i + 1] (z[i] = (a[0] + beta) / (a[i] + beta)) in one call, on both sides of a prefix-product level"""
    n = 1 << k
    for u in sorted({0, 1, n - 1, n}):
        for beta, gamma in ((BETA, GAMMA), (AC.CHALLENGES["raw_r_minus_1"], 0)):
            cases = [AC.lookup_same(0x5A0 + k, k, u, beta, gamma), AC.lookup_shift(0x5B0 + k, k, u, beta, gamma), AC.lookup_same(0x5C0 + k, k, u, beta, gamma)]
            got = check_lookups(cases, k, u, beta, gamma, f"usable {u}")
            if u:
                assert np.array_equal(got[0], np.tile(word(AC.enc(1)), (n, 1)))
                for i in range(u + 1, n):
                    assert np.array_equal(got[:, i], got[:, u])


@pytest.mark.parametrize("through", ["a", "s"])
@pytest.mark.parametrize("lookup", [0, 2])
def test_lookup_zero_denominator_stays_in_its_lookup(lib, lookup, through):
    """a'[row] = -beta (s: s'[row] = -gamma) in lookup 0, and in lookup 2, of 3: z of that lookup is 0 from the next row on, the other
    lookups of the call are exact -- the scan restarts at every lookup"""
    k = 6
    n, u = 1 << k, (1 << k) - 6
    base = [AC.lookup_naive_case(AC.random_words(0x70 + 4 * l, n), AC.random_words(0x71 + 4 * l, n), AC.random_words(0x72 + 4 * l, n),
                                 AC.random_words(0x73 + 4 * l, n), u, BETA, GAMMA) for l in range(3)]
    assert all(all(c.expected) for c in base)
    for row in (0, 16, u - 1):
        cases = list(base)
        cases[lookup] = AC.lookup_zero_den(base[lookup], row, through, BETA, GAMMA)
        got = check_lookups(cases, k, u, BETA, GAMMA, f"zero at row {row}")
        assert got[lookup][:row + 1].any(axis=1).all() and not got[lookup][row + 1:].any()
        for l in set(range(3)) - {lookup}:
            assert got[l].any(axis=1).all()


# ---------------------------------------------------------------- 7. linear combination
COUNTS = [1, 2, 31, 32, 33, 127, 128, 129, 160, 161, 2047, 2048, 2049, 4096, 4097]
ROWS = [1, 255, 256, 257]
BUFFERS = 8


def lincomb_device(lib, d_columns, coeffs, n, out_ptr):
    count = len(d_columns)
    ptrs = (C.c_void_p * count)(*[t.data_ptr() for t in d_columns])
    cw = AC.words(coeffs)
    _lib.check(lib.zkhip_fr_linear_combination_device(ptrs, cw.ctypes.data, count, n, out_ptr, None))
    torch.cuda.synchronize()


def lincomb_values(count, n):
    """(name, buffers, coefficients): the largest canonical word in every cell under coefficients 1, r - 1 and 0; the constants under
    seeded coefficients"""
    top = [[R - 1] * n]
    mixed = [AC.constant_words(0xC0 + b, n) for b in range(BUFFERS)]
    return [("r - 1 x enc(1)", top, [AC.enc(1)] * count), ("r - 1 x enc(r - 1)", top, [AC.enc(R - 1)] * count), ("r - 1 x 0", top, [0] * count),
            ("constants x seeded", mixed, AC.random_words(0xC8 + count, count))]


@pytest.mark.parametrize("count", COUNTS)
def test_lincomb_group_switches_and_ragged_rows(lib, count):
    """one column more and less than a group of 32, than the 4 groups between normalisations and than the 64 groups between
    reductions; n on both sides of a workgroup of 256"""
    for n in ROWS:
        for name, buffers, coeffs in lincomb_values(count, n):
            d_buffers = dev_columns(buffers)
            columns = [buffers[j % len(buffers)] for j in range(count)]
            exp = AC.lincomb_expected(coeffs, columns)
            if name == "r - 1 x enc(1)":
                assert exp == [(R - count) % R] * n
            out = Guarded(n)
            lincomb_device(lib, [d_buffers[j % len(buffers)] for j in range(count)], coeffs, n, out.ptr())
            same(out.words(name), exp, f"n {n}, {name}")


def test_lincomb_more_groups_than_an_unreduced_sum_can_hold(lib):
    """1400 groups whose partial sums are all r - 32: unreduced their sum is 1400 r, and r 2^-232 ~ 3171407 a time 1355 is past 2^32, the
    top limb.  Up to 1354 groups fe_reduce_soft still brings an unreduced sum back (its quotient comes from the top limb alone), so the
    counts up to 4097 pass without the reduction every 64 groups; this one does not."""
    groups, n = 1400, 3
    assert (groups * R) >> 232 >= 1 << 32 > (1354 * R) >> 232
    count = 32 * groups
    top = [R - 1] * n
    d_top = dev(top)
    coeffs, columns = [AC.enc(1)] * count, [top] * count
    exp = AC.lincomb_expected(coeffs, columns)
    assert exp == [R - count] * n
    out = Guarded(n)
    lincomb_device(lib, [d_top] * count, coeffs, n, out.ptr())
    same(out.words(), exp, f"{count} columns")


@pytest.mark.parametrize("count", [20, 70, 161])
@pytest.mark.parametrize("alias",["last", "listed_three_times", "second_group"])
def test_lincomb_output_is_one_of_the_columns(lib, count, alias):
    """the output is the last column, a column listed three times, a column of the second group (with one group: a middle column) --
    every thread reads its row of every column before the row is written"""
    n = 257
    at = {"last": [count - 1], "listed_three_times": [2, count // 2, count - 3], "second_group": [min(40, count // 2)]}[alias]
    for name, buffers, coeffs in lincomb_values(count, n):
        own = list(buffers[0])                                         # the aliased column: a buffer of its own
        columns = [own if j in at else buffers[j % len(buffers)] for j in range(count)]
        exp = AC.lincomb_expected(coeffs, columns)
        d_buffers = dev_columns(buffers)
        out = Guarded(n)
        out.body.copy_(dev(own))
        d_columns = [out.body if j in at else d_buffers[j % len(buffers)] for j in range(count)]
        lincomb_device(lib, d_columns, coeffs, n, out.ptr())
        same(out.words(name), exp, f"{alias}, {name}")

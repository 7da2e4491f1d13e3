"""Inputs and expectations of the argument-product tests: the permutation argument's products, the lookup argument's products and the
linear combination of many columns (a helper module: no tests, no fixtures; nothing here imports the package under test).

Everything is stated on the external Montgomery-256 WORDS as integers below r: a column is a list of words, a challenge is a word, and an
expectation is a list of words.  The products are not linear, so a family decodes its words (x = w 2^-256), works on the field values in
Python integers and encodes what it returns.  Each family returns its inputs together with the expected product columns;
tests/test_argument_cases_host.py pins the closed forms to the written-out recurrence before a GPU sees them."""
import collections
import functools
import hashlib
import random

import numpy as np

from oracle import bn254 as O

R = O.R_MOD
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R)
DELTA = O.FR_DELTA


def enc(x):
    """the Montgomery-256 word of the field value x"""
    return x % R * MONT % R


def dec(w):
    """the field value of the Montgomery-256 word w"""
    return w * MONT_INV % R


def _seeded(tag):
    return int.from_bytes(hashlib.sha256(b"argument-cases-" + tag).digest(), "big") % R


# ---- edge words --------------------------------------------------------------------------------------------------------------------------------
LIMB = (1 << 29) - 1
LOW_LIMBS_FULL = ((R >> 232) << 232) - 1           # read as it stands (fe_unpack<0>): the eight low 29-bit limbs are all ones
LOW_LIMBS_FULL_5 = ((R >> 227) << 227) - 1         # read shifted left by 5 (fe_unpack<5>): limbs 1 .. 7 all ones, limb 0 = 0x1fffffe0
SEEDED = _seeded(b"word")
CONSTANTS = collections.OrderedDict([
    ("enc0", enc(0)), ("enc1", enc(1)), ("enc_r_minus_1", enc(R - 1)),
    ("raw1", 1), ("raw_r_minus_1", R - 1),
    ("raw_low_limbs_full", LOW_LIMBS_FULL),
    ("raw_low_limbs_full_5", LOW_LIMBS_FULL_5),
    ("seeded", SEEDED),
])
assert all(0 <= w < R for w in CONSTANTS.values()) and len(set(CONSTANTS.values())) == len(CONSTANTS)

# beta and gamma.  "0, 1, r - 1, r - 2" are taken both as raw words and as field values (their encodings): a kernel unpacks the word, the
# formulas see the value.
SEEDED_CHALLENGE = _seeded(b"challenge")
CHALLENGES = collections.OrderedDict([
    ("0", 0), ("raw1", 1), ("raw_r_minus_1", R - 1), ("raw_r_minus_2", R - 2),
    ("enc1", enc(1)), ("enc_r_minus_1", enc(R - 1)), ("enc_r_minus_2", enc(R - 2)),
    ("seeded", SEEDED_CHALLENGE),
])
LOOKUP_CHALLENGES = collections.OrderedDict((k, CHALLENGES[k]) for k in ("0", "raw1", "raw_r_minus_1", "enc1", "enc_r_minus_1", "seeded"))
assert len(set(CHALLENGES.values())) == len(CHALLENGES)


# ---- words <-> numpy ---------------------------------------------------------------------------------------------------------------------------
def words(values):
    """ints below 2^256 -> (n, 4) uint64, the memory of &[Fr]"""
    values = list(values)
    buf = b"".join(v.to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype="<u8").reshape(len(values), 4).astype(np.uint64)


def ints(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def limbs(w, shift=0):
    """the nine 29-bit limbs of w << shift: what fe_unpack<shift> makes of a word"""
    return [((w << shift) >> (29 * i)) & LIMB for i in range(9)]


def random_words(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(count)]


def constant_words(seed, count, avoid=()):
    """`count` words drawn from CONSTANTS, none of them in `avoid`"""
    rng = random.Random(seed)
    pool = [w for w in CONSTANTS.values() if w not in avoid]
    return [rng.choice(pool) for _ in range(count)]


@functools.lru_cache(maxsize=4)
def omega_powers(k):
    w, out, cur = O.omega_for(k), [], 1
    for _ in range(1 << k):
        out.append(cur)
        cur = cur * w % R
    assert cur == 1
    return out


def delta_powers(count):
    out, cur = [], 1
    for _ in range(count):
        out.append(cur)
        cur = cur * DELTA % R
    return out


def batch_inverse(values):
    """the inverses of non-zero field values by ONE inversion (the rotation family at 2^16 rows would spend a minute on one each)"""
    prefix, acc = [], 1
    for v in values:
        prefix.append(acc)
        acc = acc * v % R
    assert acc, "a zero among the values"
    inv, out = pow(acc, -1, R), [0] * len(values)
    for i in range(len(values) - 1, -1, -1):
        out[i] = inv * prefix[i] % R
        inv = inv * values[i] % R
    return out


# ---- permutation argument ----------------------------------------------------------------------------------------------------------------------
PermCase = collections.namedtuple("PermCase", "values sigmas expected")      # [column][row], [column][row], [set][row]: words


def set_count(n_columns, chunk):
    return -(-n_columns // chunk)


def perm_factors(values, sigmas, k, beta, gamma):
    """(num, den), [column][row] field values: v + beta delta^c omega^i + gamma and v + beta sigma + gamma"""
    b, g, pw, dl = dec(beta), dec(gamma), omega_powers(k), delta_powers(len(values))
    num = [[(dec(v) + b * dl[c] % R * pw[i] + g) % R for i, v in enumerate(col)] for c, col in enumerate(values)]
    den = [[(dec(v) + b * dec(s) + g) % R for v, s in zip(col, sig)] for col, sig in zip(values, sigmas)]
    return num, den


def perm_naive(values, sigmas, chunk, k, usable, beta, gamma):
    """[DEP] plonk/permutation/prover.rs written out: per set z[i + 1] = z[i] num[i] / den[i] over the rows below `usable` (a zero
    denominator counts as zero), the rows after `usable` repeat z[usable], and a set starts from the product of the earlier sets' rows:
    z_(s-1)[usable], which with usable = n (no such row) is the product over all n rows"""
    n = 1 << k
    num, den = perm_factors(values, sigmas, k, beta, gamma)
    out, acc = [], 1
    for lo in range(0, len(values), chunk):
        cols = range(lo, min(lo + chunk, len(values)))
        z = []
        for i in range(n):
            z.append(enc(acc))
            if i < usable:
                a = b = 1
                for c in cols:
                    a, b = a * num[c][i] % R, b * den[c][i] % R
                acc = acc * a % R * pow(b, -1, R) % R if b else 0
        out.append(z)
    return out


def perm_first_denominator_is_zero(values, sigmas, chunk, k, beta, gamma):
    """is the denominator of set 0 at row 0 zero: everything after it is, and the combination says nothing"""
    b, g = dec(beta), dec(gamma)
    return any((dec(values[c][0]) + b * dec(sigmas[c][0]) + g) % R == 0 for c in range(min(chunk, len(values))))


def perm_seeded(seed, n_columns, k, overrides=()):
    """seeded values and sigmas; `overrides`: (array 0 = values / 1 = sigmas, column, row, word) cells that hold an edge word"""
    n = 1 << k
    flat = random_words(seed, 2 * n_columns * n)
    values = [flat[c * n:(c + 1) * n] for c in range(n_columns)]
    sigmas = [flat[(n_columns + c) * n:(n_columns + c + 1) * n] for c in range(n_columns)]
    for which, c, i, w in overrides:
        (sigmas if which else values)[c][i] = w
    return values, sigmas


def perm_naive_case(seed, n_columns, chunk, k, usable, beta, gamma, overrides=()):
    values, sigmas = perm_seeded(seed, n_columns, k, overrides)
    return PermCase(values, sigmas, perm_naive(values, sigmas, chunk, k, usable, beta, gamma))


def edge_overrides(n_columns, k):
    """every constant at the first and last row of some column, in the values and in the sigmas"""
    n, out = 1 << k, []
    for j, w in enumerate(CONSTANTS.values()):
        out.append((j & 1, j % n_columns, 0 if j & 2 else n - 1, w))
        out.append((1 - (j & 1), (j + 1) % n_columns, (j * 37 + 5) % n, w))
    return out


def perm_identity(seed, n_columns, chunk, k, usable, beta, gamma, values=None):
    """sigma_j[i] = delta^j omega^i: numerator and denominator are the same product, every z is 1 whatever the values"""
    n, pw, dl = 1 << k, omega_powers(k), delta_powers(n_columns)
    if values is None:
        values = [random_words(seed * 1000 + c, n) for c in range(n_columns)]
    sigmas = [[enc(dl[c] * pw[i]) for i in range(n)] for c in range(n_columns)]
    one = enc(1)
    return PermCase(values, sigmas, [[one] * n for _ in range(set_count(n_columns, chunk))])


def perm_rotation(consts, chunk, k, usable, beta, gamma):
    """column j is the constant word consts[j] and sigma_j[i] = delta^j omega^(i + 1): with f_j(i) = c_j + beta delta^j omega^i + gamma the
    ratio of row i is f_j(i) / f_j(i + 1), the product telescopes:  z_s[i] = P_s prod_{j in s} f_j(0) / f_j(min(i, u)),  P_s the product of
    f_j(0) / f_j(u) over the columns of the earlier sets (indices mod n: with u = n that is 1).  One shared inversion."""
    n, pw, dl = 1 << k, omega_powers(k), delta_powers(len(consts))
    b, g, m = dec(beta), dec(gamma), len(consts)
    top = min(usable, n - 1)                                                # the largest row index min(i, u) takes inside the array
    f = [[(dec(consts[j]) + b * dl[j] % R * pw[i] + g) % R for i in range(top + 1)] for j in range(m)]
    f_u = [(dec(consts[j]) + b * dl[j] % R * pw[usable % n] + g) % R for j in range(m)]
    flat_inv = batch_inverse([x for col in f for x in col] + f_u)
    inv = [flat_inv[j * (top + 1):(j + 1) * (top + 1)] for j in range(m)]
    inv_u = flat_inv[m * (top + 1):]
    expected, start = [], 1
    for lo in range(0, m, chunk):
        cols = range(lo, min(lo + chunk, m))
        head = start
        for j in cols:
            head = head * f[j][0] % R
        z = []
        for i in range(top + 1):
            v = head
            for j in cols:
                v = v * inv[j][i] % R
            z.append(enc(v))
        z += [z[top]] * (n - 1 - top)
        expected.append(z)
        for j in cols:
            start = start * f[j][0] % R * inv_u[j] % R
    values = [[consts[j]] * n for j in range(m)]
    sigmas = [[enc(dl[j] * pw[(i + 1) % n]) for i in range(n)] for j in range(m)]
    return PermCase(values, sigmas, expected)


def _zeros_after(expected, cells):
    """`expected` with every position after the first of `cells` (set, row) zero: z[row] is the product of the rows before it, so the
    positions up to and including (set, row) are those of the unchanged input"""
    s0, r0 = min(cells)
    return [[w if (s, i) <= (s0, r0) else 0 for i, w in enumerate(z)] for s, z in enumerate(expected)]


def perm_zero_den(case, cells, chunk, k, beta, gamma):
    """`case` with sigma solved at the first column of each (set, row) of `cells` so that v + beta sigma + gamma = 0 there: z is 0 from
    the next row on, and in every later set"""
    assert dec(beta)
    sigmas = [list(col) for col in case.sigmas]
    for s, row in cells:
        c = s * chunk
        sigmas[c][row] = enc(-(dec(case.values[c][row]) + dec(gamma)) * pow(dec(beta), -1, R))
    return PermCase(case.values, sigmas, _zeros_after(case.expected, cells))


def perm_zero_num(case, cells, chunk, k, usable, beta, gamma):
    """the same done to a numerator: v solved so that v + beta delta^c omega^row + gamma = 0.  The value also stands in that row's
    denominator, which only positions after (set, row) see."""
    pw = omega_powers(k)
    values = [list(col) for col in case.values]
    for s, row in cells:
        c = s * chunk
        values[c][row] = enc(-(dec(beta) * pow(DELTA, c, R) % R * pw[row] + dec(gamma)))
    return PermCase(values, case.sigmas, _zeros_after(case.expected, cells))


# the edge-word grid of the permutation products: k = 6, 5 columns
EDGE_K, EDGE_COLUMNS, EDGE_CHUNKS = 6, 5, (1, 2, 5)
EDGE_FILLS = tuple(CONSTANTS) + ("mixed_3", "mixed_7")


def perm_edge_fill(fill):
    """(values, sigmas) of one fill: every cell the one constant, or (mixed) every cell drawn from CONSTANTS"""
    n = 1 << EDGE_K
    if fill in CONSTANTS:
        return [[CONSTANTS[fill]] * n for _ in range(EDGE_COLUMNS)], [[CONSTANTS[fill]] * n for _ in range(EDGE_COLUMNS)]
    flat = constant_words(_seeded(fill.encode()), 2 * EDGE_COLUMNS * n)
    cols = [flat[c * n:(c + 1) * n] for c in range(2 * EDGE_COLUMNS)]
    return cols[:EDGE_COLUMNS], cols[EDGE_COLUMNS:]


def perm_edge_combinations(fill, chunk):
    """[(beta name, gamma name, skipped)] over CHALLENGES x CHALLENGES for one fill and chunk length"""
    values, sigmas = perm_edge_fill(fill)
    return [(bn, gn, perm_first_denominator_is_zero(values, sigmas, chunk, EDGE_K, b, g))
            for bn, b in CHALLENGES.items() for gn, g in CHALLENGES.items()]


# ---- lookup argument ---------------------------------------------------------------------------------------------------------------------------
LookupCase = collections.namedtuple("LookupCase", "a s ap sp expected")      # one lookup: four columns and z, [row] words


def lookup_naive(a, s, ap, sp, usable, beta, gamma):
    """z[0] = 1, z[i + 1] = z[i] (a + beta)(s + gamma) / ((a' + beta)(s' + gamma)) over the rows below `usable`, 1 / 1 from there on:
    the oracle's grand product of the two written-out columns"""
    b, g = dec(beta), dec(gamma)
    num = [(dec(x) + b) * (dec(y) + g) % R if i < usable else 1 for i, (x, y) in enumerate(zip(a, s))]
    den = [(dec(x) + b) * (dec(y) + g) % R if i < usable else 1 for i, (x, y) in enumerate(zip(ap, sp))]
    return [enc(z) for z in O.grand_product(num, den)]


def lookup_naive_case(a, s, ap, sp, usable, beta, gamma):
    return LookupCase(a, s, ap, sp, lookup_naive(a, s, ap, sp, usable, beta, gamma))


def lookup_edge_columns(seed, k, beta, gamma):
    """four columns drawn from CONSTANTS; a and a' never hold the word of -beta, s and s' never that of -gamma, so that no factor is zero
    and every row of z says something (the zero factors have cases of their own)"""
    n = 1 << k
    nb, ng = enc(-dec(beta)), enc(-dec(gamma))
    return (constant_words(seed, n, (nb,)), constant_words(seed + 1, n, (ng,)), constant_words(seed + 2, n, (nb,)), constant_words(seed + 3, n, (ng,)))


def lookup_same(seed, k, usable, beta, gamma):
    """a' = a, s' = s: z is 1"""
    n = 1 << k
    a, s = random_words(seed, n), random_words(seed + 1, n)
    return LookupCase(a, s, list(a), list(s), [enc(1)] * n)


def lookup_shift(seed, k, usable, beta, gamma):
    """a'[i] = a[i + 1], s' = s: z[i] = (a[0] + beta) / (a[min(i, u)] + beta)"""
    n = 1 << k
    a, s = random_words(seed, n), random_words(seed + 1, n)
    ap = a[1:] + a[:1]
    b = dec(beta)
    inv = batch_inverse([(dec(x) + b) % R for x in a])
    head = (dec(a[0]) + b) % R
    top = min(usable, n - 1)
    return LookupCase(a, s, ap, list(s), [enc(head * inv[min(i, top)]) for i in range(n)])


def lookup_zero_den(case, row, through, beta, gamma):
    """`case` with a'[row] = -beta (through = "a") or s'[row] = -gamma ("s"): z is 0 from the next row on"""
    ap, sp = list(case.ap), list(case.sp)
    if through == "a":
        ap[row] = enc(-dec(beta))
    else:
        sp[row] = enc(-dec(gamma))
    return LookupCase(case.a, case.s, ap, sp, [w if i <= row else 0 for i, w in enumerate(case.expected)])


# ---- linear combination ------------------------------------------------------------------------------------------------------------------------
def lincomb_expected(coeffs, columns):
    """out[i] = sum_j c_j col_j[i] on the words: the coefficient enters as its value, the column as its word.  Columns that are the same
    list object (the buffers a test cycles through) are summed once, with the sum of their coefficients."""
    total, order = {}, {}
    for c, col in zip(coeffs, columns):
        total[id(col)] = total.get(id(col), 0) + dec(c)
        order[id(col)] = col
    n = len(columns[0]) if columns else 0
    return [sum(t * order[key][i] for key, t in total.items()) % R for i in range(n)]


# ---- the products of k_perm_num_mul on their limbs ---------------------------------------------------------------------------------------------
# csrc/fp29.hpp restated on Python integers, for ONE purpose: to find the input at which the product of two numerator factors needs the
# carry propagation in front of it.  A factor is the limb-wise sum of three 9-limb values (the word shifted left by 5, a Montgomery product,
# the canonical internal form of gamma): limbs up to 3 (2^29 - 1).  A column of fe_mul adds nine products a_i b_j and nine m_i p_j in a
# 64-bit accumulator, so two such operands (9 * 9 * 2^58 > 2^64) can overflow it where a carry-propagated operand (limbs < 2^29) cannot.
P_LIMBS = [(R >> (29 * i)) & LIMB for i in range(8)] + [R >> 232]
P_INV29 = -pow(R, -1, 1 << 29) % (1 << 29)


def fe_limbs(value):
    """the N form of a value: limbs 0 .. 7 below 2^29, limb 8 the rest"""
    return [(value >> (29 * i)) & LIMB for i in range(8)] + [value >> 232]


def fe_value(a):
    return sum(l << (29 * i) for i, l in enumerate(a))


def fe_mul_model(a, b):
    """fe_mul column by column -> (the result's limbs with the accumulator cut to 64 bits as the kernel's is, the largest accumulator)"""
    acc = true_acc = peak = 0
    m, r = [0] * 9, [0] * 9
    for k in range(17):
        lo = max(0, k - 8)
        col = sum(a[i] * b[k - i] for i in range(lo, min(k, 8) + 1)) + sum(m[i] * P_LIMBS[k - i] for i in range(lo, min(k - 1, 8) + 1) if k < 9 or i >= k - 8)
        acc, true_acc = (acc + col) & (2**64 - 1), true_acc + col
        if k < 9:
            m[k] = (acc & 0xFFFFFFFF) * P_INV29 & LIMB
            acc, true_acc = (acc + m[k] * P_LIMBS[0]) & (2**64 - 1), true_acc + m[k] * P_LIMBS[0]
        else:
            r[k - 9] = acc & LIMB
        peak = max(peak, true_acc)
        acc, true_acc = acc >> 29, true_acc >> 29
    r[8] = acc & 0xFFFFFFFF
    return r, peak


def internal(word):
    """the canonical internal form (x 2^261) of an external word (x 2^256)"""
    return word * 32 % R


def perm_numerator_factor(value_word, column, beta, gamma):
    """the limbs of v + (beta delta^c) omega^0 + gamma at row 0 as k_perm_num_mul adds them up: fe_unpack<5> of the word, the product of
    the canonical table entry of beta delta^c with omega^0 = fe_mul(1, 1), the canonical internal gamma"""
    one = fe_limbs(internal(enc(1)))
    x, _ = fe_mul_model(one, one)
    prod, _ = fe_mul_model(fe_limbs(internal(enc(dec(beta) * pow(DELTA, column, R)))), x)
    return [u + p + g for u, p, g in zip(limbs(value_word, 5), prod, fe_limbs(internal(gamma)))]


@functools.lru_cache(maxsize=None)
def perm_unnormalised_product_input():
    """(beta, gamma, word): with `word` at row 0 of columns 0 and 1 of one set, the product of the two factors overflows fe_mul's accumulator
    unless the first is carry-propagated.  beta and gamma are solved so that beta's table entry times omega^0, and gamma's internal form,
    have their eight low limbs all ones -- with the word whose shifted limbs are all ones the first factor's limbs are 3 (2^29 - 1) -- and
    the top limbs are searched until the second factor, whose product term nobody controls, is large enough as well."""
    word = LOW_LIMBS_FULL_5
    for tb in range(1, 400):
        beta = ((tb << 232) - 1) * pow(32, -1, R) % R                   # internal(beta) = (tb << 232) - 1
        f0 = perm_numerator_factor(word, 0, beta, 0)
        if any(l != x + LIMB for l, x in zip(f0[1:8], [LIMB] * 7)):      # the product came out as the residue + p: not all ones
            continue
        for tg in range(1, 40):
            gamma = ((tg << 232) - 1) * pow(32, -1, R) % R
            a, b = perm_numerator_factor(word, 0, beta, gamma), perm_numerator_factor(word, 1, beta, gamma)
            if fe_mul_model(a, b)[1] >= 1 << 64 and fe_mul_model(fe_limbs(fe_value(a)), b)[1] < 1 << 64:
                return beta, gamma, word
    raise AssertionError("no input found")

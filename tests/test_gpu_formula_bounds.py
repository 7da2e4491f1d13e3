"""GPU (-m gpu): the point and field formulas in the shapes the MSM kernels instantiate, at the top of their documented magnitude bounds.

Both MSMs spend their time in a mixed addition that the older parity hooks do not reach: G1's bucket kernels call xyzz_madd<true> (Y3 as one
fused product pair, csrc/ec.hpp), G2's call xyzz2_madd_lazy<true> / xyzz2_add_lazy<true> and its in-memory forms (csrc/ec2.hpp), and all of
them multiply through the asm-block column chains of csrc/mac_blocks.hpp, which no host compilation sees.  The hooks' newer ops run exactly
those instantiations on the device; `op + 256` first lifts every operand to the largest representative below the bound its call site documents
(csrc/fe_lift.hpp).  A lift never changes a residue, so a lifted op must give the plain op's output: every comparison here is bit-exact,
against the oracle, for every row of every call.  Random data sits far below the bounds; the lifted ops are what tells that they close.

The G2 rows include an off-curve equal-x table: a point next to the accumulated one, x2 = x1 + d, y2 = y1 + e with d, e in
{0, (t, t), (t, -t), (t, 0), (0, t)} -- the Fq2 shapes whose square has a vanishing component, where a zero test reading one component of
P^2 would take the doubling / identity branch by mistake.  The formulas never use the curve constant, and neither does the oracle's addition."""
import numpy as np
import pytest

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F

pytestmark = pytest.mark.gpu
LIFT = 256


# ---------------------------------------------------------------------------------------------------------------------------- field
def _field_rows(field, n):
    """operand rows in pairs (i, i ^ 1): the edge list of test_field_ops_vs_oracle, pairs with a b + c d = 0 (c = -a, d = b), random rows; the
    last pair (the two lanes of the last wave at n = 258, the whole call at n = 2) is a zero-sum pair on an edge value"""
    p = O.Q_MOD if field == 0 else O.R_MOD
    g = O.SplitMix64(4100 + 2 * n + field)
    a = [g.fr() % p for _ in range(n)]
    b = [g.fr() % p for _ in range(n)]
    edge = [0, 1, p - 1, p - 2, (p - 1) // 2, O.to_mont(1, p), O.to_mont(p - 1, p), (1 << 253) % p]
    for i, e in enumerate(edge):
        if i < n:
            a[i], b[i] = e, edge[(3 * i + 1) % len(edge)]
    for k, e in enumerate(edge):                       # zero-sum pairs on every edge value, then on random ones
        i = 8 + 2 * k
        if i + 1 < n:
            if k % 2 == 0:
                a[i] = e
            a[i + 1], b[i + 1] = (p - a[i]) % p, b[i]
    a[n - 2], b[n - 2] = p - 1, p - 1
    a[n - 1], b[n - 1] = 1, p - 1
    lim = lambda v: np.array([O.limbs4(x) for x in v], dtype=np.uint64)
    return lim(a), lim(b)


@pytest.mark.parametrize("n", [2, 256, 258])
@pytest.mark.parametrize("field", [0, 1])
def test_field_shapes_at_their_limb_limits(lib, cref, field, n):
    """ops 4 .. 7 and their lifted forms: one workgroup of k_field_op_shapes, and one full group plus a single wave of two lanes"""
    a, b = _field_rows(field, n)
    swap = np.arange(n) ^ 1
    run = lambda op: _field_call(lib, field, op, a, b)
    prod = cref.field_op(field, 0, a, b)
    fused = cref.field_op(field, 1, prod, np.ascontiguousarray(prod[swap]))
    zero_sum = [i for i in range(n) if not fused[i].any()]
    assert len(zero_sum) >= 2 and (n == 2 or len(zero_sum) >= 16)
    want = {4: prod, 5: cref.field_op(field, 3, a, b), 6: fused, 7: fused}
    assert np.array_equal(run(0), want[4]) and np.array_equal(run(3), want[5])      # the compiler's shape, for the row-by-row equality below
    for op in (4, 5, 6, 7):
        for lifted in (0, LIFT):
            got = run(op + lifted)
            bad = np.flatnonzero((got != want[op]).any(axis=1))
            assert bad.size == 0, f"field {field} op {op + lifted} n {n}: rows {bad[:8].tolist()}"


def _field_call(lib, field, op, a, b):
    out = np.full_like(a, 0xA5A5A5A5A5A5A5A5)
    _lib.check(lib.zkhip_test_field_op(field, op, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.shape[0]))
    return out


def test_field_fused_ops_need_an_even_count(lib):
    a = np.zeros((3, 4), dtype=np.uint64)
    out = np.zeros_like(a)
    for op in (6, 7, 6 + LIFT, 7 + LIFT):
        assert lib.zkhip_test_field_op(0, op, a.ctypes.data, a.ctypes.data, out.ctypes.data, 3) == -1
    for op in (8, LIFT, 3 + LIFT, 8 + LIFT, 512 + 4):
        assert lib.zkhip_test_field_op(0, op, a.ctypes.data, a.ctypes.data, out.ctypes.data, 2) == -1


# ---------------------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("n", [1, 128, 129])
def test_g1_chain_shape_mixed_addition(lib, cref, n):
    """ops 5 / 6 (a + b, a - b through xyzz_madd<true> twice) and their lifted forms: the k_g1_op_chain workgroup, full and with one extra lane"""
    A, _, _ = cref.gen_bases(25, max(n, 8))
    B, _, _ = cref.gen_bases(26, max(n, 8))
    neg_of = lambda row: F.g1_encode([O.neg(O.affine_from_limbs([int(x) for x in row]))])[0]
    A[3] = 0; B[4] = 0; A[5] = 0; B[5] = 0          # identities on either / both sides
    B[6] = A[6]                                      # equal points: the doubling inside the mixed addition (a - b: the identity)
    B[7] = neg_of(A[7])                              # opposite points (a - b: the doubling through the negated load)
    if n == 1:
        A[0], B[0] = A[6], B[6]
    else:
        A[n - 1] = A[6]; B[n - 1] = B[6]             # the last lane (alone in its workgroup at n = 129)
        A[n - 2] = A[7]; B[n - 2] = B[7]
    A, B = np.ascontiguousarray(A[:n]), np.ascontiguousarray(B[:n])
    pts = lambda M: [O.affine_from_limbs([int(x) for x in r]) for r in M]
    Pa, Pb = pts(A), pts(B)

    def run(op):
        out = np.full((n, 12), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        _lib.check(lib.zkhip_test_g1_op(op, A.ctypes.data, B.ctypes.data, out.ctypes.data, n))
        return [F.g1_decode_jacobian(r) for r in out]

    want = {5: [O.add(P, Q) for P, Q in zip(Pa, Pb)], 6: [O.add(P, O.neg(Q)) for P, Q in zip(Pa, Pb)]}
    assert run(0) == want[5] and run(2) == want[6]
    for op in (5, 6):
        for lifted in (0, LIFT):
            got = run(op + lifted)
            bad = [i for i in range(n) if got[i] != want[op][i]]
            assert not bad, f"g1 op {op + lifted} n {n}: rows {bad[:8]}"


# ---------------------------------------------------------------------------------------------------------------------------- G2
def enc(points):
    return np.array([O.g2_affine_to_limbs(P) for P in points], dtype=np.uint64).reshape(len(points), 16)


def dec(row):
    return O.g2_jac_from_limbs([int(x) for x in row])


def walk(t0, d, n):
    """[(t0 + i d) G2 for i < n]: one scalar multiplication, then a walk of Jacobian additions (as tests/test_gpu_g2.py)"""
    P, D = O.g2_to_jac(O.g2_scalar_mul(t0, O.G2_GEN)), O.g2_to_jac(O.g2_scalar_mul(d, O.G2_GEN))
    out = []
    for _ in range(n):
        out.append(P)
        P = O.g2_jac_add(P, D)
    return [O.g2_to_affine(J) for J in out]


dbl = lambda P: O.g2_add(P, P)
T_VALUES = (1, O.Q_MOD - 1, 0x1D2C3B4A5968778695A4B3C2D1E0F)
SHAPES = (lambda t: (0, 0), lambda t: (t, t), lambda t: (t, O.Q_MOD - t), lambda t: (t, 0), lambda t: (0, t))


def _table(base, k):
    """the 25 (d, e) neighbours of `base` (off the curve but for d = e = 0): (x + d, y + e)"""
    rows = []
    for di, d in enumerate(SHAPES):
        for ei, e in enumerate(SHAPES):
            t = T_VALUES[(di + ei + k) % len(T_VALUES)]
            Q = (O.f2_add(base[0], d(t)), O.f2_add(base[1], e(t)))
            assert Q[1][0] != 0 and Q[1][1] != 0
            rows.append(Q)
    return rows


@pytest.fixture(scope="module")
def g2_rows():
    """for every row count: a, and b for the three families of ops -- b next to a (ops 7, 8), next to 2a (9, 10) and next to 4a (5 + 256) --
    with the expected outputs, computed once"""
    pool = walk(0x5A4B534E41500002 + 777, 0x9E3779B97F4A7C15F39CC0605CEDC835, 140)
    other = walk(0x1234567, 0xABCDEF0123, 140)
    cases = {}
    for n in (1, 64, 65, 100, 130):
        Pa = list(pool[:n])
        fam = []
        for k in range(3):                                        # base = 2^k a
            base = list(Pa)
            for _ in range(k):
                base = [dbl(P) for P in base]
            Pb = list(other[:n])
            a_rows = list(Pa)
            if n == 1:
                Pb[0] = _table(base[0], k)[5]                     # d = (t, t), e = 0: c0 of P^2 vanishes, the chord sum is expected
            else:
                a_rows[3] = None; Pb[4] = None; a_rows[5] = None; Pb[5] = None       # the identity on either side and on both sides
                Pb[6] = base[6]; Pb[7] = O.g2_neg(base[7])        # b = base, b = -base: under both neg values (ops 7 and 8) for k = 0; b = +-2a for k = 1
                tab = _table(base[8], k)                          # the table in the first wave: the same a, its 25 neighbours
                for j, Qj in enumerate(tab):
                    a_rows[8 + j] = a_rows[8]; Pb[8 + j] = Qj
                tail = n - 64 * ((n - 1) // 64) if n > 64 else 0  # ... and again in the last, partly filled wave (all 25 at n = 100)
                for j in range(min(tail, 25)):
                    r = n - tail + j
                    a_rows[r] = a_rows[8]; Pb[r] = tab[(5 + 6 * j) % 25 if tail < 25 else j]
            fam.append((a_rows, Pb))
        cases[n] = fam
    return cases


G2_OPS = {                                                        # op -> (family, expected)
    7: (0, lambda P, Q: O.g2_add(P, Q)),
    8: (0, lambda P, Q: O.g2_add(P, O.g2_neg(Q))),
    9: (1, lambda P, Q: O.g2_add(dbl(P), Q)),
    10: (1, lambda P, Q: O.g2_add(dbl(P), Q)),
    11: (1, lambda P, Q: dbl(dbl(P))),
    5: (2, lambda P, Q: O.g2_add(dbl(dbl(P)), Q)),
    6: (2, lambda P, Q: dbl(dbl(dbl(dbl(P))))),
}


@pytest.mark.parametrize("n", [1, 64, 65, 100, 130])
def test_g2_lazy_layer_at_its_bounds(lib, g2_rows, n):
    """ops 7 .. 11 and the lifted forms of 5 .. 11: one wave, one wave plus one lane, three waves the last of two lanes, and (n = 100) a last
    wave that holds the whole equal-x table"""
    wants = {}
    for op in (7, 8, 9, 10, 11, 5 + LIFT, 6 + LIFT, 7 + LIFT, 8 + LIFT, 9 + LIFT, 10 + LIFT, 11 + LIFT):
        family, f = G2_OPS[op & 255]
        Pa, Pb = g2_rows[n][family]
        key = (op & 255) if op & 255 != 10 else 9
        if key not in wants:
            wants[key] = [f(P, Q) for P, Q in zip(Pa, Pb)]
        a, b = enc(Pa), enc(Pb)
        out = np.full((n, 24), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        _lib.check(lib.zkhip_test_g2_op(op, a.ctypes.data, b.ctypes.data, out.ctypes.data, n))
        got = [dec(r) for r in out]
        bad = [i for i in range(n) if got[i] != wants[key][i]]
        assert not bad, f"g2 op {op} n {n}: rows {bad[:8]}"


def test_g2_equal_x_rows_take_the_expected_branches(g2_rows):
    """the oracle's outputs for the table rows (no device call): the double for d = e = 0, the identity for d = 0 with e != 0, and a finite
    chord sum other than the double for every d != 0 -- so a device row that took the equal-x branch by mistake cannot match"""
    Pa, Pb = g2_rows[100][0]
    for j in range(25):
        for r in (8 + j, 64 + j):
            got = O.g2_add(Pa[r], Pb[r])
            if j == 0:
                assert got == dbl(Pa[r])
            elif j < 5:
                assert got is None
            else:
                assert got is not None and got != dbl(Pa[r])


def test_g2_op_range(lib):
    a = np.zeros((1, 16), dtype=np.uint64)
    out = np.zeros((1, 24), dtype=np.uint64)
    for op in (12, LIFT, 4 + LIFT, 12 + LIFT, 512 + 7, -1):
        assert lib.zkhip_test_g2_op(op, a.ctypes.data, a.ctypes.data, out.ctypes.data, 1) == -1
    for op in (7, 4 + LIFT, 7 + LIFT):
        assert lib.zkhip_test_g1_op(op, a.ctypes.data, a.ctypes.data, out.ctypes.data, 1) == -1

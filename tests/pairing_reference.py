"""An independent big-integer optimal ate pairing on BN254, for the tests of csrc/pairing.hpp (a plain module, not a conftest).

Fq12 is the FLAT ring Fq[w] / (w^12 - 18 w^6 + 82): with w^6 = xi = 9 + u and u^2 = -1, (w^6 - 9)^2 + 1 = 0.  The Miller loop runs over the plain
bits of 6x + 2 with AFFINE arithmetic on the twist (slopes by a field inversion) and the final exponentiation is one pow(f, (q^12 - 1) / r):
neither the tower, nor the projective line formulas, nor the hard-part addition chain of the code under test appear here.

The fixed basis map between the tower of pairing.hpp and this ring: the tower element sum c[h][i] v^i w^h (h < 2, i < 3, c in Fq2) has
c[h][i] = a + b u at w^(2 i + h), and u = w^6 - 9."""
X_BN = 4965661367192848881
Q = 36 * X_BN**4 + 36 * X_BN**3 + 24 * X_BN**2 + 6 * X_BN + 1
R = 36 * X_BN**4 + 36 * X_BN**3 + 18 * X_BN**2 + 6 * X_BN + 1
ATE = 6 * X_BN + 2
FINAL_EXP = (Q**12 - 1) // R
G1 = (1, 2)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))

ONE = [1] + [0] * 11
ZERO = [0] * 12


# ---- Fq2 (tuples), only for the twist's affine arithmetic -----------------------------------------------------------------------------
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
def f2_add(a, b): return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)
def f2_sub(a, b): return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
def f2_conj(a): return (a[0], -a[1] % Q)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], Q - 2, Q)
    return (a[0] * n % Q, -a[1] * n % Q)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


XI = (9, 1)
TWIST_B = f2_mul((3, 0), f2_inv(XI))


def g2_on_twist(P):
    return P is None or f2_sub(f2_mul(P[1], P[1]), f2_add(f2_mul(f2_mul(P[0], P[0]), P[0]), TWIST_B)) == (0, 0)


def g2_add(P, S):
    if P is None: return S
    if S is None: return P
    if P[0] == S[0]:
        if f2_add(P[1], S[1]) == (0, 0): return None
        lam = f2_mul(f2_mul((3, 0), f2_mul(P[0], P[0])), f2_inv(f2_add(P[1], P[1])))
    else:
        lam = f2_mul(f2_sub(S[1], P[1]), f2_inv(f2_sub(S[0], P[0])))
    x = f2_sub(f2_sub(f2_mul(lam, lam), P[0]), S[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(P[0], x)), P[1]))


def g2_mul(k, P):
    acc = None
    while k:
        if k & 1:
            acc = g2_add(acc, P)
        P = g2_add(P, P)
        k >>= 1
    return acc


def g2_neg(P): return None if P is None else (P[0], (-P[1][0] % Q, -P[1][1] % Q))


def g1_add(P, S):
    if P is None: return S
    if S is None: return P
    if P[0] == S[0]:
        if (P[1] + S[1]) % Q == 0: return None
        lam = 3 * P[0] * P[0] * pow(2 * P[1], Q - 2, Q) % Q
    else:
        lam = (S[1] - P[1]) * pow(S[0] - P[0], Q - 2, Q) % Q
    x = (lam * lam - P[0] - S[0]) % Q
    return (x, (lam * (P[0] - x) - P[1]) % Q)


def g1_mul(k, P):
    acc = None
    while k:
        if k & 1:
            acc = g1_add(acc, P)
        P = g1_add(P, P)
        k >>= 1
    return acc


def g1_neg(P): return None if P is None else (P[0], -P[1] % Q)


# ---- the flat Fq12 ------------------------------------------------------------------------------------------------------------------------
def f12_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):                      # w^12 = 18 w^6 - 82
        c = t[k]
        if c:
            t[k - 6] += 18 * c
            t[k - 12] -= 82 * c
    return [v % Q for v in t[:12]]


def f12_pow(a, e):
    r = ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_from_f2(c, power):
    """(a + b u) w^power with u = w^6 - 9, power < 6"""
    out = [0] * 12
    out[power] = (c[0] - 9 * c[1]) % Q
    out[power + 6] = c[1] % Q
    return out


def from_tower(c):
    """c[h][i] = (a, b): the tower element of pairing.hpp -> flat"""
    out = [0] * 12
    for h in range(2):
        for i in range(3):
            e = f12_from_f2(c[h][i], 2 * i + h)
            out = [(x + y) % Q for x, y in zip(out, e)]
    return out


def to_tower(f):
    """the inverse of from_tower"""
    return [[((f[2 * i + h] + 9 * f[2 * i + h + 6]) % Q, f[2 * i + h + 6] % Q) for i in range(3)] for h in range(2)]


def f12_frobenius(a, k):
    """a^(q^k), by a pow: slow, for tests of single values only"""
    return f12_pow(a, Q**k)


def f12_conj(a):
    """a^(q^6): w -> -w"""
    return [(-v % Q) if i & 1 else v for i, v in enumerate(a)]


def f12_inv(a):
    return f12_pow(a, Q**12 - 2)


# ---- the pairing ---------------------------------------------------------------------------------------------------------------------------
def _line(T, S, P):
    """the line through T and S (twist points, affine, T != -S) at P in E(Fq), and T + S"""
    if T[0] == S[0]:
        lam = f2_mul(f2_mul((3, 0), f2_mul(T[0], T[0])), f2_inv(f2_add(T[1], T[1])))
    else:
        lam = f2_mul(f2_sub(S[1], T[1]), f2_inv(f2_sub(S[0], T[0])))
    # untwist (x, y) -> (x w^2, y w^3): l(P) = yP - lam xP w + (lam xT - yT) w^3
    l = [P[1] % Q] + [0] * 11
    a = f12_from_f2(f2_mul(lam, (-P[0] % Q, 0)), 1)
    b = f12_from_f2(f2_sub(f2_mul(lam, T[0]), T[1]), 3)
    l = [(x + y + z) % Q for x, y, z in zip(l, a, b)]
    x = f2_sub(f2_sub(f2_mul(lam, lam), T[0]), S[0])
    return l, (x, f2_sub(f2_mul(lam, f2_sub(T[0], x)), T[1]))


GAMMA12 = f2_pow(XI, (Q - 1) // 3)      # xi^(2 (q - 1) / 6)
GAMMA13 = f2_pow(XI, (Q - 1) // 2)


def g2_frobenius(S):
    return (f2_mul(f2_conj(S[0]), GAMMA12), f2_mul(f2_conj(S[1]), GAMMA13))


def miller_loop(P, S):
    """P in G1 (affine or None), S in G2 (affine or None) -> flat Fq12, not exponentiated"""
    if P is None or S is None:
        return ONE
    f, T = ONE, S
    for bit in bin(ATE)[3:]:
        l, T2 = _line(T, T, P)
        f = f12_mul(f12_mul(f, f), l)
        T = T2
        if bit == "1":
            l, T = _line(T, S, P)
            f = f12_mul(f, l)
    S1 = g2_frobenius(S)
    S2 = g2_neg(g2_frobenius(S1))
    l, T = _line(T, S1, P)
    f = f12_mul(f, l)
    l, T = _line(T, S2, P)
    return f12_mul(f, l)


def final_exponentiation(f):
    return f12_pow(f, FINAL_EXP)


def pairing(P, S):
    return final_exponentiation(miller_loop(P, S))


def pairing_check(pairs):
    f = ONE
    for P, S in pairs:
        f = f12_mul(f, miller_loop(P, S))
    return final_exponentiation(f) == ONE

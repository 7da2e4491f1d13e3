"""Inputs and expected values shared by tests/test_pairing_host.py (the host build of csrc/pairing.hpp) and tests/test_gpu_pairing.py (the device
hook and the check kernel): a plain module, not a conftest.  Every expected value comes from tests/pairing_reference.py or from the scalars."""
import functools
import random

import pairing_reference as P

Q, R = P.Q, P.R
MONT = 1 << 256
SEEDED = (0x1D4F0C35A2B7E9886F4A31C59E07B2D3A4C1958E6B7F20D3C9A8574E1B2F6D07 % R, 0x0B7A9E42C6D1F3058A4C7E19B3D5F6270819A2B4C6D8E0F1325476981ABCDEF5 % R)
EDGE_SCALARS = (1, 2, R - 1) + SEEDED


# ---- memory formats (Montgomery-256, little-endian words) ---------------------------------------------------------------------------------
def enc_fq(x: int) -> bytes:
    return (x * MONT % Q).to_bytes(32, "little")


def dec_fq(b: bytes) -> int:
    v = int.from_bytes(b, "little")
    assert v < Q, "not canonical"
    return v * pow(MONT, -1, Q) % Q


def enc12(t) -> bytes:
    return b"".join(enc_fq(t[h][i][j]) for h in range(2) for i in range(3) for j in range(2))


def dec12(b: bytes):
    v = [dec_fq(b[32 * k:32 * k + 32]) for k in range(12)]
    return [[(v[6 * h + 2 * i], v[6 * h + 2 * i + 1]) for i in range(3)] for h in range(2)]


def enc_g1(p) -> bytes:
    return bytes(64) if p is None else enc_fq(p[0]) + enc_fq(p[1])


def enc_g2(p) -> bytes:
    return bytes(128) if p is None else enc_fq(p[0][0]) + enc_fq(p[0][1]) + enc_fq(p[1][0]) + enc_fq(p[1][1])


def pair_operand(g1, g2) -> bytes:
    """operand `a` of hook operation 8"""
    return (enc_g1(g1) + enc_g2(g2)).ljust(384, b"\0")


# ---- tower operations ----------------------------------------------------------------------------------------------------------------------
OP_MUL, OP_SQR, OP_INV, OP_FROB1, OP_FROB2, OP_FROB3, OP_CYC, OP_LINE, OP_MILLER, OP_FINAL, OP_CONJ, OP_CHECK2 = range(12)


def _const(v):
    return [[(v, v) for _ in range(3)] for _ in range(2)]


@functools.lru_cache(maxsize=None)
def elements():
    """0, 1 and q - 1 in every coordinate, and seeded values"""
    rng = random.Random(0x50414952)
    rnd = lambda: [[(rng.randrange(Q), rng.randrange(Q)) for _ in range(3)] for _ in range(2)]
    return [_const(0), _const(1), _const(Q - 1), rnd(), rnd(), rnd()]


@functools.lru_cache(maxsize=None)
def cyclotomic_elements():
    """seeded values through the easy part f -> f^((q^6 - 1)(q^2 + 1)) (by the reference's pow)"""
    return [P.to_tower(P.f12_pow(P.from_tower(t), (Q**6 - 1) * (Q**2 + 1))) for t in elements()[3:5]]


@functools.lru_cache(maxsize=None)
def tower_cases():
    """[(name, op, a bytes, b bytes, expected flat Fq12)]: exact comparisons"""
    els = elements()
    flat = [P.from_tower(t) for t in els]
    zero = enc12(_const(0))
    out = []
    for i in range(len(els)):
        j = (i + 1) % len(els)
        out.append((f"mul {i}x{j}", OP_MUL, enc12(els[i]), enc12(els[j]), P.f12_mul(flat[i], flat[j])))
        out.append((f"sqr {i}", OP_SQR, enc12(els[i]), zero, P.f12_mul(flat[i], flat[i])))
        out.append((f"conj {i}", OP_CONJ, enc12(els[i]), zero, P.f12_conj(flat[i])))
    for i in (0, 1, 2, 3, 4):
        out.append((f"inverse {i}", OP_INV, enc12(els[i]), zero, P.f12_inv(flat[i])))
    for i in (1, 2, 3, 5):
        for k, op in ((1, OP_FROB1), (2, OP_FROB2), (3, OP_FROB3)):
            out.append((f"frobenius^{k} {i}", op, enc12(els[i]), zero, P.f12_frobenius(flat[i], k)))
    for i in (1, 2, 3, 4):                                         # the line's coefficients: the first three Fq2 of b
        l = els[(i + 2) % len(els)]
        sparse = [[l[0][0], (0, 0), (0, 0)], [l[0][1], l[0][2], (0, 0)]]
        out.append((f"line {i}", OP_LINE, enc12(els[i]), enc12(l), P.f12_mul(flat[i], P.from_tower(sparse))))
    for i, c in enumerate(cyclotomic_elements()):
        fc = P.from_tower(c)
        out.append((f"cyclotomic square {i}", OP_CYC, enc12(c), zero, P.f12_mul(fc, fc)))
    for i in (1, 3):
        out.append((f"final exponentiation {i}", OP_FINAL, enc12(els[i]), zero, P.final_exponentiation(flat[i])))
    return out


@functools.lru_cache(maxsize=None)
def miller_cases():
    """[(name, a bytes, the reference's REDUCED pairing)]: a Miller value is defined up to a factor of a proper subfield (the projective line
    scalings), so the comparison is after the reference's final exponentiation"""
    out = []
    for a, b in ((1, 1), (SEEDED[0], SEEDED[1])):
        g1, g2 = P.g1_mul(a, P.G1), P.g2_mul(b, P.G2)
        out.append((f"miller {a % 1000}x{b % 1000}", pair_operand(g1, g2), P.pairing(g1, g2)))
    return out


# ---- verdicts --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g1(k):
    return P.g1_mul(k % R, P.G1)


@functools.lru_cache(maxsize=None)
def _g2(k):
    return P.g2_mul(k % R, P.G2)


def pairs_from_scalars(ab):
    """[(a_i, b_i)] -> (g1 bytes, g2 bytes, expected verdict): pairs (a_i G, b_i H); the product is one iff sum a_i b_i = 0 mod r.  A scalar 0
    is the identity."""
    g1 = b"".join(enc_g1(_g1(a)) for a, _ in ab)
    g2 = b"".join(enc_g2(_g2(b)) for _, b in ab)
    return g1, g2, sum(a * b for a, b in ab) % R == 0


@functools.lru_cache(maxsize=None)
def verdict_cases():
    """[(name, g1 bytes, g2 bytes, n, expected)] for the host build: (aG, bH), (-ab G, H) over the edge scalars, one scalar off by one, identities"""
    out = []
    for a, b in zip(EDGE_SCALARS, EDGE_SCALARS[1:] + EDGE_SCALARS[:1]):
        for delta in (0, 1):
            ab = ((a, b), (-(a * b) % R, 1 + delta))
            g1, g2, want = pairs_from_scalars(ab)
            assert want == (delta == 0 or a * b % R == 0)
            out.append((f"({a % 1000} G, {b % 1000} H), (-ab G, {1 + delta} H)", g1, g2, 2, want))
    out.append(("n = 1, identity in G1", enc_g1(None), enc_g2(_g2(5)), 1, True))
    out.append(("n = 1, identity in G2", enc_g1(_g1(5)), enc_g2(None), 1, True))
    out.append(("n = 1, no identity", enc_g1(_g1(5)), enc_g2(_g2(7)), 1, False))
    out.append(("n = 0", b"", b"", 0, True))
    return out

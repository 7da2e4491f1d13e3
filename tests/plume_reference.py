"""A restatement of the PLUME nullifier check of include/zkhip.h ("PLUME nullifiers on secp256k1") in plain Python integers and hashlib,
independent of zksnap_circuits_halo2_amd/plume.py and of every header under csrc/: the tests compare the library with this file.  The group
arithmetic is Jacobian, written from the textbook formulas (one modular inverse per result), so a few hundred voters cost seconds.  The
identity is None inside and the affine pair (0, 0) outside, as the header restates it."""
import hashlib

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
DST = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_"

# RFC 9380 section 8.7 / appendix E.1: the curve E' of the simplified SWU map and the 3-isogeny E' -> secp256k1
ISO_A = 0x3f8731abdd661adca08a5558f0f5d272e953d363cb6f0e5d405447c01a444533
ISO_B = 1771
Z = P - 11
X_NUM = [0x8e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38daaaaa8c7, 0x07d3d4c80bc321d5b9f315cea7fd44c5d595d2fc0bf63b92dfff1044f17c6581,
         0x534c328d23f234e6e2a413deca25caece4506144037c40314ecbd0b53d9dd262, 0x8e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38daaaaa88c]
X_DEN = [0xd35771193d94918a9ca34ccbb7b640dd86cd409542f8487d9fe6b745781eb49b, 0xedadc6f64383dc1df7c4b2d51b54225406d36b641f5e41bbc52a56612a8c6d14, 1]
Y_NUM = [0x4bda12f684bda12f684bda12f684bda12f684bda12f684bda12f684b8e38e23c, 0xc75e0c32d5cb7c0fa9d0a54b12a0a6d5647ab046d686da6fdffc90fc201d71a3,
         0x29a6194691f91a73715209ef6512e576722830a201be2018a765e85a9ecee931, 0x2f684bda12f684bda12f684bda12f684bda12f684bda12f684bda12f38e38d84]
Y_DEN = [0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffff93b, 0x7a06534bb8bdb49fd5e9e6632722c2989467c1bfc8e8d978dfb425d2685c2573,
         0x6484aa716545ca2cf3a70c3fa8fe337e0a3d21162f0d6299a7bf8192bfd2a76f, 1]


# ---- the group: Jacobian (X, Y, Z) with x = X / Z^2, y = Y / Z^3; None is the identity ---------------------------------------------------------
def _jac(pt):
    return None if pt == (0, 0) else (pt[0], pt[1], 1)


def _affine(j):
    if j is None:
        return (0, 0)
    zi = pow(j[2], -1, P)
    return (j[0] * zi * zi % P, j[1] * zi * zi * zi % P)


def _double(j):
    if j is None or j[1] == 0:
        return None
    X, Y, Zz = j
    s = 4 * X * Y * Y % P
    m = 3 * X * X % P
    x3 = (m * m - 2 * s) % P
    return (x3, (m * (s - x3) - 8 * pow(Y, 4, P)) % P, 2 * Y * Zz % P)


def _add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    z1z1, z2z2 = a[2] * a[2] % P, b[2] * b[2] % P
    u1, u2 = a[0] * z2z2 % P, b[0] * z1z1 % P
    s1, s2 = a[1] * b[2] * z2z2 % P, b[1] * a[2] * z1z1 % P
    if u1 == u2:
        return _double(a) if s1 == s2 else None
    h, r = (u2 - u1) % P, (s2 - s1) % P
    h2 = h * h % P
    h3, v = h * h2 % P, u1 * h2 % P
    x3 = (r * r - h3 - 2 * v) % P
    return (x3, (r * (v - x3) - s1 * h3) % P, h * a[2] * b[2] % P)


def _mul(k, j):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = _double(acc)
        if bit == "1":
            acc = _add(acc, j)
    return acc


def on_curve(pt):
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - x * x * x - 7) % P == 0


def add(a, b):
    return _affine(_add(_jac(a), _jac(b)))


def neg(a):
    return (a[0], -a[1] % P)


def mul(k, pt):
    """k * pt for any integer k >= 0 (the group has order N, so k counts mod N)"""
    return _affine(_mul(k, _jac(pt)))


def lincomb(a, p, b, q):
    return _affine(_add(_mul(a, _jac(p)), _mul(b, _jac(q))))


def compress_point(pt):
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


# ---- RFC 9380, suite secp256k1_XMD:SHA-256_SSWU_RO_ ----------------------------------------------------------------------------------------
def expand_message_xmd(msg, dst, length):
    ell = (length + 31) // 32
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    out = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        out.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, out[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(out)[:length]


def map_to_curve_sswu(u):
    """the simplified SWU map to E' (section 6.6.2, the straight-line form), exceptional case included"""
    tv1 = (Z * Z * pow(u, 4, P) + Z * u * u) % P
    if tv1 == 0:
        x1 = ISO_B * pow(Z * ISO_A, -1, P) % P
    else:
        x1 = -ISO_B * pow(ISO_A, -1, P) * (1 + pow(tv1, -1, P)) % P
    gx1 = (pow(x1, 3, P) + ISO_A * x1 + ISO_B) % P
    x2 = Z * u * u * x1 % P
    gx2 = (pow(x2, 3, P) + ISO_A * x2 + ISO_B) % P
    if pow(gx1, (P - 1) // 2, P) in (0, 1):
        x, y = x1, pow(gx1, (P + 1) // 4, P)
    else:
        x, y = x2, pow(gx2, (P + 1) // 4, P)
    assert (y * y - x * x * x - ISO_A * x - ISO_B) % P == 0
    if (u & 1) != (y & 1):
        y = P - y if y else 0
    return (x, y)


def _poly(coeffs, x):
    return sum(c * pow(x, j, P) for j, c in enumerate(coeffs)) % P


def iso_map(pt):
    x, y = pt
    xd, yd = _poly(X_DEN, x), _poly(Y_DEN, x)
    if xd == 0 or yd == 0:
        return (0, 0)
    return (_poly(X_NUM, x) * pow(xd, -1, P) % P, y * _poly(Y_NUM, x) * pow(yd, -1, P) % P)


def map_to_curve(u):
    return iso_map(map_to_curve_sswu(u % P))


def hash_to_curve_bytes(data, dst=DST):
    """RFC 9380 hash_to_curve of a byte string"""
    uniform = expand_message_xmd(data, dst, 96)
    u0, u1 = int.from_bytes(uniform[:48], "big") % P, int.from_bytes(uniform[48:], "big") % P
    return add(map_to_curve(u0), map_to_curve(u1))


def hash_to_curve(msg, pk):
    """H(msg, pk) of the header"""
    return hash_to_curve_bytes(bytes(msg) + compress_point(pk))


# ---- PLUME -----------------------------------------------------------------------------------------------------------------------------
def challenge(pk, h, nullifier, a, b):
    return int.from_bytes(hashlib.sha256(b"".join(compress_point(x) for x in (G, pk, h, nullifier, a, b))).digest(), "big")


def well_formed(pk, nullifier, s, c):
    return on_curve(pk) and on_curve(nullifier) and 0 <= s < N and 0 <= c < N


def verdict(msg, nullifier, pk, s, c):
    """0 accepted, 1 well-formed but refused, 2 malformed"""
    if not well_formed(pk, nullifier, s, c):
        return 2
    h = hash_to_curve(msg, pk)
    a = lincomb(s, G, c, neg(pk))
    b = lincomb(s, h, c, neg(nullifier))
    return 0 if challenge(pk, h, nullifier, a, b) == c else 1


def gen(sk, msg, r):
    """`gen_test_nullifier` with r in place of the random draw -> (pk, nullifier, s, c); a digest >= N is taken mod N here (the reference
    panics on one)"""
    pk = mul(sk, G)
    h = hash_to_curve(msg, pk)
    nullifier = mul(sk, h)
    c = challenge(pk, h, nullifier, mul(r, G), mul(r, h)) % N
    return pk, nullifier, (r + sk * c) % N, c

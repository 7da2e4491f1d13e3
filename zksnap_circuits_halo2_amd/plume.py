"""PLUME nullifiers on secp256k1 (include/zkhip.h, "PLUME nullifiers on secp256k1"): the check the reference makes of every ballot before it
builds a round's inputs -- `verify_nullifier(&[1, 0], &nullifier, &pk_voter[i], &s, &c)`, reference aggregator/src/utils.rs:289-290 -- for a
whole batch in one device call.

`compress_point`, `hash_to_curve`, `verify_native` and `gen_native` are the host forms on Python integers, named after the reference's
(voter_tests/src/lib.rs:25-119); they are this module's own restatement, and tests compare them with the library's C calls and kernels.
`hash_to_curve_host`, `verify_host` and `sign_host` run one voter through the library's host C calls (the headers the kernels run).
`lincomb_device`, `hash_to_curve_many_device`, `verify_many_device` and `sign_many_device` run the kernels over device tensors of canonical integers: a point is `[..., 8]` int64
(x then y, four little-endian words each), a scalar `[..., 4]`.  There is no CPU fallback for the device calls.

A point is a pair of integers (x, y); the identity is (0, 0).
"""
from __future__ import annotations

import hashlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .tensors import from_words, raw_tensor, stream_of, to_words

MAX_MSG = _lib.ZKHIP_PLUME_MAX_MSG
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
DST = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_"
ACCEPTED, REFUSED, MALFORMED = 0, 1, 2

Point = Tuple[int, int]
_IDENTITY = (0, 0)

# RFC 9380 section 8.7 and appendix E.1: E' of the simplified SWU map, and the 3-isogeny's coefficients, lowest power first
_A, _B, _Z = 0x3f8731abdd661adca08a5558f0f5d272e953d363cb6f0e5d405447c01a444533, 1771, P - 11
_ISO = (
    (0x8e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38daaaaa8c7, 0x07d3d4c80bc321d5b9f315cea7fd44c5d595d2fc0bf63b92dfff1044f17c6581,
     0x534c328d23f234e6e2a413deca25caece4506144037c40314ecbd0b53d9dd262, 0x8e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38e38daaaaa88c),
    (0xd35771193d94918a9ca34ccbb7b640dd86cd409542f8487d9fe6b745781eb49b, 0xedadc6f64383dc1df7c4b2d51b54225406d36b641f5e41bbc52a56612a8c6d14, 1),
    (0x4bda12f684bda12f684bda12f684bda12f684bda12f684bda12f684b8e38e23c, 0xc75e0c32d5cb7c0fa9d0a54b12a0a6d5647ab046d686da6fdffc90fc201d71a3,
     0x29a6194691f91a73715209ef6512e576722830a201be2018a765e85a9ecee931, 0x2f684bda12f684bda12f684bda12f684bda12f684bda12f684bda12f38e38d84),
    (0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffff93b, 0x7a06534bb8bdb49fd5e9e6632722c2989467c1bfc8e8d978dfb425d2685c2573,
     0x6484aa716545ca2cf3a70c3fa8fe337e0a3d21162f0d6299a7bf8192bfd2a76f, 1),
)


# ---- the group on the host: affine integers, the chord-and-tangent rule with every case spelt out -------------------------------------------------
def on_curve(pt: Point) -> bool:
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - x * x * x - 7) % P == 0


def neg(pt: Point) -> Point:
    return (pt[0], -pt[1] % P)


def add(a: Point, b: Point) -> Point:
    if a == _IDENTITY:
        return b
    if b == _IDENTITY:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return _IDENTITY
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def mul(k: int, pt: Point) -> Point:
    """k pt for any k >= 0; the group has order N"""
    acc, k = _IDENTITY, int(k) % N
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt, k = add(pt, pt), k >> 1
    return acc


def lincomb(a: int, p: Point, b: int, q: Point) -> Point:
    return add(mul(a, p), mul(b, q))


def compress_point(pt: Point) -> bytes:
    """`compress_point`: 02 | 03 then x big-endian, 03 for an odd y; the identity (0, 0) gives 02 and zeros"""
    return bytes([2 + (pt[1] & 1)]) + int(pt[0]).to_bytes(32, "big")


# ---- RFC 9380 ----------------------------------------------------------------------------------------------------------------------------------
def _expand_message_xmd(msg: bytes, length: int) -> bytes:
    dst_prime = DST + bytes([len(DST)])
    b0 = hashlib.sha256(bytes(64) + msg + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    blocks = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    while 32 * len(blocks) < length:
        mixed = bytes(x ^ y for x, y in zip(b0, blocks[-1]))
        blocks.append(hashlib.sha256(mixed + bytes([len(blocks) + 1]) + dst_prime).digest())
    return b"".join(blocks)[:length]


def _horner(coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def _map_to_curve(u: int) -> Point:
    """simplified SWU on E' (RFC 9380 section 6.6.2), then the 3-isogeny; a zero denominator of the isogeny gives the identity"""
    zu2 = _Z * u * u % P
    tv1 = (zu2 * zu2 + zu2) % P
    x1 = _B * pow(_Z * _A, -1, P) % P if tv1 == 0 else -_B * pow(_A, -1, P) * (1 + pow(tv1, -1, P)) % P
    gx1 = (x1 * x1 * x1 + _A * x1 + _B) % P
    x, y = x1, pow(gx1, (P + 1) // 4, P)
    if y * y % P != gx1:
        x = zu2 * x1 % P
        y = pow((x * x * x + _A * x + _B) % P, (P + 1) // 4, P)
    if (u ^ y) & 1:
        y = -y % P
    xn, xd, yn, yd = (_horner(c, x) for c in _ISO)
    if xd == 0 or yd == 0:
        return _IDENTITY
    return (xn * pow(xd, -1, P) % P, y * yn * pow(yd, -1, P) % P)


def hash_to_curve_bytes(data: bytes) -> Point:
    """RFC 9380 hash_to_curve(data), suite secp256k1_XMD:SHA-256_SSWU_RO_ with the DST of the reference"""
    uniform = _expand_message_xmd(bytes(data), 96)
    return add(_map_to_curve(int.from_bytes(uniform[:48], "big") % P), _map_to_curve(int.from_bytes(uniform[48:], "big") % P))


def hash_to_curve(msg: bytes, pk: Point) -> Point:
    """`hash_to_curve(message, compressed_pk)`: H(msg, pk)"""
    return hash_to_curve_bytes(bytes(msg) + compress_point(pk))


# ---- PLUME -------------------------------------------------------------------------------------------------------------------------------------
def _challenge(pk: Point, h: Point, nullifier: Point, a: Point, b: Point) -> int:
    return int.from_bytes(hashlib.sha256(b"".join(compress_point(x) for x in (G, pk, h, nullifier, a, b))).digest(), "big")


def verify_native(msg: bytes, nullifier: Point, pk: Point, s: int, c: int) -> int:
    """`verify_nullifier` as a verdict: 0 accepted, 1 well-formed but refused, 2 malformed (the reference asserts, this returns)"""
    if not (on_curve(pk) and on_curve(nullifier) and 0 <= s < N and 0 <= c < N):
        return MALFORMED
    h = hash_to_curve(msg, pk)
    a = lincomb(s, G, c, neg(pk))
    b = lincomb(s, h, c, neg(nullifier))
    return ACCEPTED if _challenge(pk, h, nullifier, a, b) == c else REFUSED


def gen_native(sk: int, msg: bytes, r: int) -> Tuple[Point, Point, int, int]:
    """`gen_test_nullifier` with r in place of `Fq::random` -> (pk, nullifier, s, c).  A digest >= N (probability 2^-128) is taken mod N; the
    reference panics on one."""
    pk = mul(sk, G)
    h = hash_to_curve(msg, pk)
    nullifier = mul(sk, h)
    c = _challenge(pk, h, nullifier, mul(r, G), mul(r, h)) % N
    return pk, nullifier, (r + sk * c) % N, c


# ---- tensors -----------------------------------------------------------------------------------------------------------------------------------
def _words(values: Sequence[int]) -> np.ndarray:
    return to_words(list(values), 4)


def encode_scalars(values: Sequence[int], device=None):
    """integers below 2^256 -> an [n, 4] int64 tensor on the current device (or `device`)"""
    return raw_tensor(list(values), 4, device)


def encode_points(points: Sequence[Point], device=None):
    """(x, y) pairs, any 256-bit coordinates -> [n, 8] int64"""
    flat = [int(v) for pt in points for v in pt]
    if len(flat) != 2 * len(points):
        raise ValueError("a point is a pair (x, y)")
    return raw_tensor(flat, 4, device).reshape(len(points), 8)


def decode_scalars(tensor) -> List[int]:
    return from_words(tensor.reshape(-1, 4))


def decode_points(tensor) -> List[Point]:
    return [tuple(pt) for pt in from_words(tensor.reshape(-1, 2, 4))]


def _want(t, words: int, who: str, count: Optional[int] = None):
    import torch

    if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != words or not t.is_cuda:
        raise ValueError(f"{who}: an [n, {words}] int64 tensor on the device (there is no CPU fallback)")
    if count is not None and t.shape[0] != count:
        raise ValueError(f"{who}: the arrays differ in length")
    return t.contiguous()


def _msg(msg, who: str) -> bytes:
    msg = bytes(msg)
    if len(msg) > MAX_MSG:
        raise ValueError(f"{who}: the message is at most {MAX_MSG} bytes")
    return msg


def _ptr(t):
    return t.data_ptr() if t.numel() else None


# ---- one voter through the library's host calls ----------------------------------------------------------------------------------------------
def hash_to_curve_host(msg: bytes, pk: Point) -> Tuple[Point, int]:
    """zkhip_secp256k1_hash_to_curve -> (H(msg, pk), status); ((0, 0), 2) for a malformed pk.  No GPU is touched."""
    import ctypes as C

    msg = _msg(msg, "hash_to_curve_host")
    key, out, status = _words([pk[0], pk[1]]), np.zeros(8, dtype=np.uint64), C.c_uint32(0)
    _lib.check(_lib.load().zkhip_secp256k1_hash_to_curve(msg, len(msg), key.ctypes.data, out.ctypes.data, C.addressof(status)))
    x, y = from_words(out.reshape(2, 4))
    return (x, y), status.value


def verify_host(msg: bytes, nullifier: Point, pk: Point, s: int, c: int) -> Tuple[int, Point]:
    """zkhip_plume_verify -> (verdict, H(msg, pk)).  No GPU is touched."""
    import ctypes as C

    msg = _msg(msg, "verify_host")
    key, nul, sw, cw = _words([pk[0], pk[1]]), _words([nullifier[0], nullifier[1]]), _words([s]), _words([c])
    h, verdict = np.zeros(8, dtype=np.uint64), C.c_uint32(0)
    _lib.check(_lib.load().zkhip_plume_verify(msg, len(msg), key.ctypes.data, nul.ctypes.data, sw.ctypes.data, cw.ctypes.data, C.addressof(verdict), h.ctypes.data))
    x, y = from_words(h.reshape(2, 4))
    return verdict.value, (x, y)


def sign_host(msg: bytes, sk: int, r: int) -> Tuple[Point, Point, int, int, int, Point]:
    """zkhip_plume_sign -> (pk, nullifier, s, c, status, H(msg, pk)): `gen_native` through the headers the kernel runs; status 2 and zeros for
    sk or r outside [1, N).  No GPU is touched."""
    import ctypes as C

    msg = _msg(msg, "sign_host")
    skw, rw = _words([sk]), _words([r])
    pk, nul, h = (np.zeros(8, dtype=np.uint64) for _ in range(3))
    s, c, status = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_uint32(0)
    _lib.check(_lib.load().zkhip_plume_sign(msg, len(msg), skw.ctypes.data, rw.ctypes.data, pk.ctypes.data, nul.ctypes.data, s.ctypes.data, c.ctypes.data,
                                            C.addressof(status), h.ctypes.data))
    pk, nul, h = (tuple(from_words(a.reshape(2, 4))) for a in (pk, nul, h))
    return pk, nul, from_words(s), from_words(c), status.value, h


# ---- the device calls ----------------------------------------------------------------------------------------------------------------------------
def lincomb_device(a, p, b, q, stream=None):
    """a, b: [n, 4] scalars (any 256-bit integers); p, q: [n, 8] points -> ([n, 8] a[i] p[i] + b[i] q[i], [n] int32 status: 2 and (0, 0) where a
    point is malformed); no host wait"""
    import torch

    p = _want(p, 8, "lincomb_device")
    n = p.shape[0]
    a, b, q = _want(a, 4, "lincomb_device", n), _want(b, 4, "lincomb_device", n), _want(q, 8, "lincomb_device", n)
    out = torch.empty((n, 8), dtype=torch.int64, device=p.device)
    status = torch.empty((n,), dtype=torch.int32, device=p.device)
    _lib.check(_lib.load().zkhip_secp256k1_lincomb_device(_ptr(a), _ptr(p), _ptr(b), _ptr(q), n, _ptr(out), _ptr(status), stream_of(stream)))
    return out, status


def hash_to_curve_many_device(msg: bytes, pk, stream=None):
    """pk: [n, 8] -> ([n, 8] H(msg, pk[i]), [n] int32 status); the message is shared by the batch; no host wait"""
    import torch

    msg, pk = _msg(msg, "hash_to_curve_many_device"), _want(pk, 8, "hash_to_curve_many_device")
    n = pk.shape[0]
    out = torch.empty((n, 8), dtype=torch.int64, device=pk.device)
    status = torch.empty((n,), dtype=torch.int32, device=pk.device)
    _lib.check(_lib.load().zkhip_secp256k1_hash_to_curve_device(msg, len(msg), _ptr(pk), n, _ptr(out), _ptr(status), stream_of(stream)))
    return out, status


class Verdicts:
    """what one `verify_many_device` found: `status` is the [n] int32 device tensor of verdicts (0 accepted, 1 refused, 2 malformed), `h` the
    [n, 8] tensor of H(msg, pk[i]) ((0, 0) where pk is malformed), `report` the [2] int64 device tensor behind `failures` and `first`.  The
    two properties wait for the stream's work and read the report back; nothing else here waits."""

    def __init__(self, status, h, report):
        self.status, self.h, self.report = status, h, report

    def _read(self) -> Tuple[int, int]:
        failures, first = (int(v) & (2**64 - 1) for v in self.report.cpu().tolist())
        return failures, first

    @property
    def failures(self) -> int:
        """how many voters have a verdict other than 0"""
        return self._read()[0]

    @property
    def first(self) -> Optional[int]:
        """the lowest index with a verdict other than 0; None when every voter is accepted"""
        failures, first = self._read()
        return first if failures else None


def verify_many_device(msg: bytes, pk, nullifier, s, c, stream=None) -> Verdicts:
    """pk, nullifier: [n, 8]; s, c: [n, 4] -> Verdicts; one launch, two lanes per voter, no host wait"""
    import torch

    msg, pk = _msg(msg, "verify_many_device"), _want(pk, 8, "verify_many_device")
    n = pk.shape[0]
    nullifier, s, c = _want(nullifier, 8, "verify_many_device", n), _want(s, 4, "verify_many_device", n), _want(c, 4, "verify_many_device", n)
    status = torch.empty((n,), dtype=torch.int32, device=pk.device)
    h = torch.empty((n, 8), dtype=torch.int64, device=pk.device)
    report = torch.empty((2,), dtype=torch.int64, device=pk.device)
    _lib.check(_lib.load().zkhip_plume_verify_device(msg, len(msg), _ptr(pk), _ptr(nullifier), _ptr(s), _ptr(c), n, _ptr(status), report.data_ptr(), _ptr(h),
                                                     stream_of(stream)))
    return Verdicts(status, h, report)


class Signatures:
    """what one `sign_many_device` made, device tensors: `pk`, `nullifier` and `h` (H(msg, pk[i])) are [n, 8], `s` and `c` [n, 4], `status` [n]
    int32 (0, or 2 with zeros in every other tensor where sk or r is outside [1, N)).  Nothing here waits for the stream."""

    def __init__(self, pk, nullifier, s, c, status, h):
        self.pk, self.nullifier, self.s, self.c, self.status, self.h = pk, nullifier, s, c, status, h


def sign_many_device(msg: bytes, sk, r, stream=None) -> Signatures:
    """sk, r: [n, 4] scalars in [1, N) -> Signatures: `gen_native` of every voter with its own r; one launch, two lanes per voter, no host wait.
    Meant for generated populations: nothing here is audited for side channels."""
    import torch

    msg, sk = _msg(msg, "sign_many_device"), _want(sk, 4, "sign_many_device")
    n = sk.shape[0]
    r = _want(r, 4, "sign_many_device", n)
    pk, nullifier, h = (torch.empty((n, 8), dtype=torch.int64, device=sk.device) for _ in range(3))
    s, c = (torch.empty((n, 4), dtype=torch.int64, device=sk.device) for _ in range(2))
    status = torch.empty((n,), dtype=torch.int32, device=sk.device)
    _lib.check(_lib.load().zkhip_plume_sign_device(msg, len(msg), _ptr(sk), _ptr(r), n, _ptr(pk), _ptr(nullifier), _ptr(s), _ptr(c), _ptr(status), _ptr(h),
                                                   stream_of(stream)))
    return Signatures(pk, nullifier, s, c, status, h)

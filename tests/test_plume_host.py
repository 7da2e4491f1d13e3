"""CPU (`-m "not gpu"`): the PLUME section where no GPU is needed.  The two vectors of RFC 9380 J.8.1 and the PLUME vector pinned in include/zkhip.h
through plume.py's host functions and through the library's host C calls (the headers the kernels run; the RFC's own messages carry no key, so
they reach the C++ code through tests/test_secp256k1_host.py instead); plume.py against tests/plume_reference.py on seeded voters; the
tensors' word order; the members tree's packing against a hand-written case."""
import hashlib
import os

import pytest

import plume_cases as PC
import plume_reference as R
from zksnap_circuits_halo2_amd import plume as PL, poseidon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, N, G = R.P, R.N, R.G
RFC = {b"": (0xc1cae290e291aee617ebaef1be6d73861479c48b841eaba9b7b5852ddfeb1346, 0x64fa678e07ae116126f08b022a94af6de15985c996c3a91b64c406a960e51067),
       b"abc": (0x3377e01eab42db296b512293120c6cee72b6ecf9f9205760bd9ff11fb3cb2c4b, 0x7f95890f33efebd1044d382a01b1bee0900fb6116f94688d487c6c7b9c8371f6)}
PK = (0x020f475341bdcaa86307f6bc73482e9f97de1eb143c4d377882338e41bd3816c, 0xd9b0bc73ac2ef11aa0d9c7e597a2247fae84397fbcf7c5545ca569c392a43d9d)
H = (0xfc8ad938310804a146d15e27c45dd085890d059a4fe75efb792557945cd4e555, 0x5dff9477353e60cd4f45ced0dadf3646df67bc09aacc29b645ff2338763b8509)
NUL = (0x022e80224208f61d2bd0db01ee45f1ad280afed208073f8cadfea796b62ec66e, 0xeb2167a30ea8a02d40c3a86c93961b7f02664aac622d11d34b9f120eed108c73)
S = 0x2dd6d3be74b08a383e981dac34dda120b5f0d32f9a1e245ab034d00b4d1149a3
C_ = 0x31c5e6a7886d3802ee2e0bc16993e6dda5f9992597c67ee4bfb5acba7bf07535


def test_the_constants_are_the_definition():
    assert (PL.P, PL.N, PL.G, PL.DST) == (2**256 - 2**32 - 977, N, G, b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_") and PL.MAX_MSG == 64
    assert R.on_curve(G) and R.mul(N, G) == (0, 0) and PL.mul(N, G) == (0, 0)


def test_rfc_9380_vectors_through_the_python_host_functions():
    for msg, want in RFC.items():
        assert PL.hash_to_curve_bytes(msg) == want == R.hash_to_curve_bytes(msg)


def test_the_pinned_plume_vector_through_python_and_through_the_host_c_calls(lib):
    msg = bytes([1, 0])
    sk = int.from_bytes(hashlib.sha256(b"sk").digest(), "big") % N
    r = int.from_bytes(hashlib.sha256(b"r").digest(), "big") % N
    assert PL.gen_native(sk, msg, r) == (PK, NUL, S, C_) == R.gen(sk, msg, r)
    assert PL.hash_to_curve(msg, PK) == H and PL.hash_to_curve_host(msg, PK) == (H, 0)
    for verify in (PL.verify_native, lambda *a: PL.verify_host(*a)[0]):
        assert verify(msg, NUL, PK, S, C_) == 0
        assert verify(msg, NUL, PK, S, C_ + 1) == 1
        assert verify(bytes([2, 0]), NUL, PK, S, C_) == 1
    assert PL.verify_host(msg, NUL, PK, S, C_) == (0, H)
    text = " ".join(open(os.path.join(ROOT, "include", "zkhip.h")).read().replace("\n *", " ").split())
    for value in (*PK, *H, *NUL, S, C_, *RFC[b""], *RFC[b"abc"]):
        assert f"0x{value:064x}" in text, hex(value)


def test_plume_py_agrees_with_the_reference_on_seeded_voters():
    rng = PC.rng("py-vs-ref")
    for i in range(6):
        msg = bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 2, 33, 34, 64])))
        sk, r = rng.randrange(1, N), rng.randrange(1, N)
        voter = PL.gen_native(sk, msg, r)
        assert voter == R.gen(sk, msg, r)
        pk, nul, s, c = voter
        assert PL.hash_to_curve(msg, pk) == R.hash_to_curve(msg, pk)
        assert PL.compress_point(pk) == R.compress_point(pk) and len(PL.compress_point(pk)) == 33
        for args in [(msg, nul, pk, s, c), (msg, nul, pk, (s + 1) % N, c), (msg, pk, nul, s, c), (msg + b"x", nul, pk, s, c), (msg, nul, pk, N, c), (msg, nul, pk, s, N),
                     (msg, (0, 0), pk, s, c), (msg, nul, (pk[0], pk[1] ^ 1), s, c), (msg, nul, pk, 0, c), (msg, nul, pk, s, 0)]:
            if len(args[0]) > PL.MAX_MSG:
                continue
            assert PL.verify_native(*args) == R.verdict(*args), args
    assert PL.compress_point((0, 0)) == bytes([2]) + bytes(32)
    for a, p, b, q in PC.lincomb_edges():
        assert PL.lincomb(a, p, b, q) == R.lincomb(a, p, b, q)


def test_the_host_c_calls_agree_with_the_reference_and_never_fail_on_a_malformed_voter(lib):
    rng = PC.rng("c-vs-ref")
    for n in (0, 2, 33, 34, 64):
        msg = bytes(rng.getrandbits(8) for _ in range(n))
        pk, nul, s, c = R.gen(rng.randrange(1, N), msg, rng.randrange(1, N))
        h = R.hash_to_curve(msg, pk)
        assert PL.hash_to_curve_host(msg, pk) == (h, 0)
        assert PL.verify_host(msg, nul, pk, s, c) == (0, h) and PL.verify_host(msg, nul, pk, s, (c + 1) % N) == (1, h)
        assert PL.verify_host(msg, nul, pk, N, c) == (2, h) and PL.verify_host(msg, nul, pk, s, PC.FULL) == (2, h)
    for bad in PC.off_curve_points():
        assert PL.hash_to_curve_host(msg, bad) == ((0, 0), 2), bad
        assert PL.verify_host(msg, nul, bad, s, c) == (2, (0, 0)) and PL.verify_host(msg, bad, pk, s, c) == (2, h), bad
    with pytest.raises(ValueError):
        PL.verify_host(bytes(65), nul, pk, s, c)


def test_points_and_scalars_are_little_endian_words():
    pts = [(1, 2**64), (2**255 + 5, PC.FULL), (0, 0)]
    t = PL.encode_points(pts, device="cpu")
    assert tuple(t.shape) == (3, 8) and PL.decode_points(t) == pts
    assert [int(v) for v in t[0]] == [1, 0, 0, 0, 0, 1, 0, 0] and int(t[1, 3]) == -(2**63) and int(t[1, 7]) == -1
    sc = [0, 1, 2**64, PC.FULL]
    t = PL.encode_scalars(sc, device="cpu")
    assert tuple(t.shape) == (4, 4) and PL.decode_scalars(t) == sc and [int(v) for v in t[2]] == [0, 1, 0, 0]
    assert tuple(PL.encode_points([], device="cpu").shape) == (0, 8) and tuple(PL.encode_scalars([], device="cpu").shape) == (0, 4)
    with pytest.raises(ValueError):
        PL.encode_scalars([1 << 256], device="cpu")
    with pytest.raises(ValueError):
        PL.encode_points([(1, 2, 3)], device="cpu")
    with pytest.raises(ValueError):                            # the device calls take device tensors: there is no CPU fallback
        PL.verify_many_device(b"", t.reshape(2, 8), t.reshape(2, 8), t[:2], t[:2])


def test_member_leaves_packs_x_then_y_in_chunks_of_11_11_10_bytes():
    """the members tree's leaf (reference aggregator/src/utils.rs:224-254): `chunks(11)` of the little-endian bytes of pk.x, then of pk.y"""
    x = int.from_bytes(bytes(range(1, 33)), "little")
    y = int.from_bytes(bytes(range(101, 133)), "little")
    want = [int.from_bytes(bytes(range(1, 12)), "little"), int.from_bytes(bytes(range(12, 23)), "little"), int.from_bytes(bytes(range(23, 33)), "little"),
            int.from_bytes(bytes(range(101, 112)), "little"), int.from_bytes(bytes(range(112, 123)), "little"), int.from_bytes(bytes(range(123, 133)), "little")]
    assert poseidon.pack_member((x, y)) == want
    assert poseidon.pack_member((2**88, 2**176)) == [0, 1, 0, 0, 0, 1] and poseidon.pack_member((0, 0)) == [0] * 6
    packed = poseidon.pack_member((PC.FULL, PC.FULL - 1))
    assert packed == [2**88 - 1, 2**88 - 1, 2**80 - 1, 2**88 - 2, 2**88 - 1, 2**80 - 1]
    with pytest.raises(ValueError):
        poseidon.pack_member((2**256, 0))
    # the leaf is the sponge over the six values: update(x chunks), update(y chunks), squeeze
    assert poseidon.hash(want) == poseidon.hash(want[:3] + want[3:])

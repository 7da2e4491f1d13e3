"""CPU (`-m "not gpu"`): the Paillier section of the C ABI and its Python layer where no GPU is needed.  Every refusal of the three `_device` calls
is decided before the device is touched, so it is returned in a process without one; the host forms agree with the vectors pinned in
include/zkhip.h; an even n takes the Python layer's host path and gives the same tensors; `compress_nullifier` packs a point by the rule
restated here."""
import ctypes as C
import os

import pytest

import abi_header as AH
import paillier_cases as PC
from zksnap_circuits_halo2_amd import _lib, paillier as P, poseidon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = 0x7000_0000_1000           # a non-null, 64-byte aligned address nothing lives at: a refused call never reads it


def _n(n):
    return (C.c_uint64 * 3)(*[(n >> (64 * i)) & (2**64 - 1) for i in range(3)])


G = (C.c_uint64 * 6)(4, 0, 0, 0, 0, 0)


def test_the_header_declares_the_section():
    assert AH.params("zkhip_paillier_mul_device") == ["const uint64_t n[3]", "const void *d_a", "const void *d_b", "size_t count", "void *d_out", "void *stream"]
    assert AH.params("zkhip_paillier_tally_device") == ["const uint64_t n[3]", "const void *d_ballots", "size_t n_ballots", "uint32_t n_cols", "const void *d_init",
                                                        "void *d_running", "void *stream"]
    assert AH.params("zkhip_paillier_encrypt_device") == ["const uint64_t n[3]", "const uint64_t g[6]", "const void *d_m", "const void *d_r", "size_t count", "void *d_out",
                                                          "void *stream"]
    for name in ("zkhip_paillier_mul_device", "zkhip_paillier_tally_device", "zkhip_paillier_encrypt_device"):
        assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported()
        assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"
    assert AH.defines()["ZKHIP_PAILLIER_WORDS"] == _lib.ZKHIP_PAILLIER_WORDS == P.WORDS == 6
    assert AH.defines()["ZKHIP_PAILLIER_MAX_N_BITS"] == _lib.ZKHIP_PAILLIER_MAX_N_BITS == 192
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    assert "[DEP paillier_chip `paillier_enc_native` / `paillier_add_native`" in text
    section = text[text.index("---- Paillier tally"):text.index("---- parity hooks")]
    assert "struct" not in section, "the section adds no struct"


def test_zkhip_error_codes_are_what_this_file_assumes():
    assert AH.defines()["ZKHIP_EINVAL"] == EINVAL


@pytest.mark.parametrize("n", [0, 1, 2, 4, PC.N_176 + 1, (1 << 192) - 238], ids=["0", "1", "2", "4", "even176", "eventop"])
def test_an_even_or_tiny_n_is_refused_by_all_three(lib, n):
    assert lib.zkhip_paillier_mul_device(_n(n), FAKE, FAKE, 4, FAKE, None) == EINVAL
    assert b"odd" in lib.zkhip_last_error()
    assert lib.zkhip_paillier_tally_device(_n(n), FAKE, 4, 5, None, FAKE + (1 << 20), None) == EINVAL
    assert lib.zkhip_paillier_encrypt_device(_n(n), G, FAKE, FAKE + (1 << 20), 4, FAKE + (2 << 20), None) == EINVAL
    # a count of zero does not excuse the modulus
    assert lib.zkhip_paillier_mul_device(_n(n), None, None, 0, None, None) == EINVAL


def test_null_and_misaligned_pointers_are_refused(lib):
    n = _n(PC.N_176)
    far = [FAKE + (k << 24) for k in range(4)]
    assert lib.zkhip_paillier_mul_device(None, far[0], far[1], 4, far[2], None) == EINVAL
    for bad in (None, far[3] + 4, far[3] + 1):
        assert lib.zkhip_paillier_mul_device(n, bad, far[1], 4, far[2], None) == EINVAL
        assert lib.zkhip_paillier_mul_device(n, far[0], bad, 4, far[2], None) == EINVAL
        assert lib.zkhip_paillier_mul_device(n, far[0], far[1], 4, bad, None) == EINVAL
        assert lib.zkhip_paillier_tally_device(n, bad, 4, 5, None, far[2], None) == EINVAL
        assert lib.zkhip_paillier_tally_device(n, far[0], 4, 5, None, bad, None) == EINVAL
        assert lib.zkhip_paillier_tally_device(n, None, 0, 5, None, bad, None) == EINVAL           # row 0 is written for no ballots too
        assert lib.zkhip_paillier_encrypt_device(n, G, bad, far[1], 4, far[2], None) == EINVAL
        assert lib.zkhip_paillier_encrypt_device(n, G, far[0], bad, 4, far[2], None) == EINVAL
        assert lib.zkhip_paillier_encrypt_device(n, G, far[0], far[1], 4, bad, None) == EINVAL
    for bad in (far[3] + 4, far[3] + 1):
        assert lib.zkhip_paillier_tally_device(n, far[0], 4, 5, bad, far[2], None) == EINVAL       # init may be null, not misaligned
    assert lib.zkhip_paillier_encrypt_device(n, None, far[0], far[1], 4, far[2], None) == EINVAL
    # a count of zero asks nothing of the array pointers and enqueues nothing: no device is needed for it
    assert lib.zkhip_paillier_mul_device(n, None, None, 0, None, None) == 0
    assert lib.zkhip_paillier_encrypt_device(n, G, None, None, 0, None, None) == 0


def test_zero_columns_and_overlaps_are_refused(lib):
    n = _n(PC.N_TOP)
    a, b, out = FAKE, FAKE + (1 << 24), FAKE + (2 << 24)
    assert lib.zkhip_paillier_tally_device(n, a, 4, 0, None, out, None) == EINVAL
    assert b"n_cols" in lib.zkhip_last_error()
    row = 5 * 48
    # d_running against the ballots and against init: first byte, last byte, and containment
    for running in (a, a + 4 * row - 8, a - 5 * row + 8, a + 48):
        assert lib.zkhip_paillier_tally_device(n, a, 4, 5, None, running, None) == EINVAL, hex(running)
    for init in (out, out + 5 * row - 8, out - row + 8):
        assert lib.zkhip_paillier_tally_device(n, a, 4, 5, init, out, None) == EINVAL, hex(init)
    # mul: d_out may BE an input, but not straddle one
    for o in (a + 48, a - 48, b + 3 * 48):
        assert lib.zkhip_paillier_mul_device(n, a, b, 4, o, None) == EINVAL, hex(o)
    # encrypt: d_out against m (32 bytes each) and r (24 bytes each)
    for o in (a, a + 4 * 32 - 8, a - 4 * 48 + 8, b, b + 4 * 24 - 8, b - 4 * 48 + 8):
        assert lib.zkhip_paillier_encrypt_device(n, G, a, b, 4, o, None) == EINVAL, hex(o)


def test_host_forms_agree_with_the_vectors_pinned_in_the_header():
    text = " ".join(open(os.path.join(ROOT, "include", "zkhip.h")).read().replace("\n *", " ").split())
    n = 293 * 433
    c1, c2 = P.enc_native(n, n + 1, 42, 23), P.enc_native(n, n + 1, 58, 101)
    assert (n, c1, c2, P.add_native(n, c1, c2)) == (0x1ef95, 0x13a7c1d25, 0x32a4da219, 0x1b5145505)
    n = (1 << 175) + (1 << 88) + 1
    d1, d2 = P.enc_native(n, n + 1, (1 << 253) + 5, (1 << 100) + 7), P.enc_native(n, n + 1, 1, n - 1)
    assert d1 == 0xd46573adf90cb6f703909e88c21470d8d54038324d18ed3723a3b62fae6bca752ac6bc47b0d61531e9c8199
    assert d2 == 0x400000000000000000000100000000000000000000018000000000000000000000ffffffffffffffffffffff
    assert P.add_native(n, d1, d2) == 0x695b9b430ba3fb1445f14b6f5912adac3d5d33a7d5d0877d0cb74a94285556ccd43275cac8214d40c0c624a
    for value in (c1, c2, P.add_native(293 * 433, c1, c2), d1, d2, P.add_native(n, d1, d2)):
        assert hex(value) in text, hex(value)
    # the textbook property the tally rests on: with g = n + 1 the product of two ciphertexts decrypts to the sum of the votes
    p, q = 293, 433
    n, lam = p * q, (p - 1) * (q - 1)
    dec = lambda c: (pow(c, lam, n * n) - 1) // n * pow(lam, -1, n) % n
    assert dec(c1) == 42 and dec(c2) == 58 and dec(P.add_native(n, c1, c2)) == 100


def test_encode_and_decode_are_inverse_and_little_endian():
    values = [[0, 1, 2**64], [2**383 + 5, PC.FULL, 2**320 - 1]]
    t = P.encode(values, device="cpu")
    assert tuple(t.shape) == (2, 3, 6) and P.decode(t) == values
    assert [int(x) for x in t[0, 2]] == [0, 1, 0, 0, 0, 0] and int(t[1, 1, 5]) == -1
    assert tuple(P.encode([], device="cpu").shape) == (0, 6) and P.decode(P.encode([], device="cpu")) == []
    with pytest.raises(ValueError):
        P.encode([1 << 384], device="cpu")
    with pytest.raises(ValueError):
        P.encode([[1, 2], [3]], device="cpu")


def test_an_even_n_is_computed_on_the_host_with_the_same_tensors():
    """the reference's generators draw n as a random 176-bit number: even half the time.  Host tensors in, host tensors out, no GPU touched."""
    n = PC.N_176 + 1
    assert n % 2 == 0
    N = n * n
    rng = PC.rng("even")
    B, Cc = 19, 5
    ballots = [[rng.choice([0, 1, N - 1, PC.FULL, rng.getrandbits(384)]) if b != 7 or c != 2 else 0 for c in range(Cc)] for b in range(B)]
    init = [rng.randrange(N) for _ in range(Cc)]
    for start in (None, init):
        tally = P.tally_device(n, P.encode(ballots, device="cpu"), None if start is None else P.encode(start, device="cpu"))
        rows = [[v % N for v in start] if start else [1] * Cc]
        for ballot in ballots:
            rows.append([x * y % N for x, y in zip(rows[-1], ballot)])
        assert tuple(tally.running.shape) == (B + 1, Cc, 6) and P.decode(tally.running) == rows
        assert tally.total() == rows[-1] and all(rows[i][2] == 0 for i in range(8, B + 1))
        assert tally.round(3) == ([v % N for v in ballots[3]], rows[3])
        with pytest.raises(IndexError):
            tally.round(B)
    a, b = [rng.getrandbits(384) for _ in range(7)], [rng.getrandbits(384) for _ in range(7)]
    ta, tb = P.encode(a, device="cpu"), P.encode(b, device="cpu")
    assert P.decode(P.mul_device(n, ta, tb)) == [x * y % N for x, y in zip(a, b)]
    assert P.mul_device(n, ta, tb, out=ta) is ta and P.decode(ta) == [x * y % N for x, y in zip(a, b)]
    g = rng.getrandbits(352)
    m, r = [0, 1, 2**256 - 1, rng.getrandbits(256)], [0, 1, n - 1, rng.getrandbits(192)]
    got = P.encrypt_many_device(n, g, P.encode_exponents(m, device="cpu"), P.encode_randomness(r, device="cpu"))
    assert tuple(got.shape) == (4, 6) and P.decode(got) == [pow(g, x, N) * pow(y, n, N) % N for x, y in zip(m, r)]
    # an odd n never takes this path: host tensors are refused, there is no CPU fallback for it
    with pytest.raises(ValueError):
        P.tally_device(PC.N_176, P.encode(ballots, device="cpu"))
    with pytest.raises(ValueError):
        P.tally_device(0, P.encode(ballots, device="cpu"))


def test_compress_nullifier_packs_tag_and_chunks_of_x():
    """`compress_native_nullifier`: the tag is 2 for an even y and 3 for an odd one; x's 32 little-endian bytes go in chunks of 11, 11 and 10"""
    rng = PC.rng("nullifier")
    for x, y in [(0, 0), (1, 1), (2**256 - 1, 2**256 - 1), (2**88, 2), (2**176, 3)] + [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(20)]:
        tag, c0, c1, c2 = poseidon.compress_nullifier((x, y))
        assert tag == (3 if y % 2 else 2)
        assert (c0, c1, c2) == (x % 2**88, (x >> 88) % 2**88, x >> 176) and c0 + (c1 << 88) + (c2 << 176) == x
        assert c0 < 2**88 and c1 < 2**88 and c2 < 2**80
    assert poseidon.compress_nullifier((2**88, 2)) == [2, 0, 1, 0] and poseidon.compress_nullifier((2**176, 3)) == [3, 0, 0, 1]
    with pytest.raises(ValueError):
        poseidon.compress_nullifier((2**256, 0))

"""CPU (`-m "not gpu"`): the signing calls of the PLUME section of the C ABI.  `zkhip_plume_sign` -- the host form, over the headers the kernel
runs -- reproduces the header's pinned vector, equals tests/plume_reference.py on seeded voters and at the scalar edges, gives status 2 and zeros
for a malformed sk or r, and `zkhip_plume_verify` accepts what it signs.  Every refusal of `zkhip_plume_sign_device` and
`zkhip_poseidon_hash_points_device` is ZKHIP_EINVAL decided on the host with nothing enqueued, in a process that sees no device."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest

import abi_header as AH
import plume_cases as PC
import plume_reference as R
from zksnap_circuits_halo2_amd import _lib, plume as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = 0x7000_0000_1000           # a non-null, 64-byte aligned address nothing lives at: a refused call never reads it
FAR = [FAKE + (k << 24) for k in range(9)]
MSG = PC.MSG
N = R.N
NAMES = ("zkhip_plume_sign_device", "zkhip_plume_sign", "zkhip_poseidon_hash_points_device")


def _sign_args(count=4, h=True):
    """msg, msg_len, sk, r, count, pk, nullifier, s, c, status, h, stream"""
    return [MSG, 2, FAR[0], FAR[1], count, FAR[2], FAR[3], FAR[4], FAR[5], FAR[6], FAR[7] if h else None, None]


def test_the_header_declares_the_calls():
    assert AH.params("zkhip_plume_sign_device") == ["const uint8_t *msg", "size_t msg_len", "const void *d_sk", "const void *d_r", "size_t count", "void *d_pk",
                                                    "void *d_nullifier", "void *d_s", "void *d_c", "void *d_status", "void *d_h_out", "void *stream"]
    assert AH.params("zkhip_plume_sign") == ["const uint8_t *msg", "size_t msg_len", "const uint64_t sk[4]", "const uint64_t r[4]", "uint64_t pk[8]",
                                             "uint64_t nullifier[8]", "uint64_t s[4]", "uint64_t c[4]", "uint32_t *status", "uint64_t h_out[8]"]
    assert AH.params("zkhip_poseidon_hash_points_device") == ["const void *d_points", "size_t n", "uint32_t layout", "void *d_out", "void *stream"]
    for name in NAMES:
        assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported()
        assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    section = text[text.index("---- PLUME nullifiers on secp256k1"):text.index("---- parity hooks")]
    assert "sign(msg, sk, r)" in section and "signing on the device" not in section[section.index("Not built"):]


def test_the_pinned_vector_of_the_header():
    sk = int.from_bytes(hashlib.sha256(b"sk").digest(), "big") % N
    r = int.from_bytes(hashlib.sha256(b"r").digest(), "big") % N
    pk, nul, s, c, status, h = PL.sign_host(bytes([1, 0]), sk, r)
    assert status == 0
    assert pk == (0x020f475341bdcaa86307f6bc73482e9f97de1eb143c4d377882338e41bd3816c, 0xd9b0bc73ac2ef11aa0d9c7e597a2247fae84397fbcf7c5545ca569c392a43d9d)
    assert h == (0xfc8ad938310804a146d15e27c45dd085890d059a4fe75efb792557945cd4e555, 0x5dff9477353e60cd4f45ced0dadf3646df67bc09aacc29b645ff2338763b8509)
    assert nul == (0x022e80224208f61d2bd0db01ee45f1ad280afed208073f8cadfea796b62ec66e, 0xeb2167a30ea8a02d40c3a86c93961b7f02664aac622d11d34b9f120eed108c73)
    assert s == 0x2dd6d3be74b08a383e981dac34dda120b5f0d32f9a1e245ab034d00b4d1149a3 and c == 0x31c5e6a7886d3802ee2e0bc16993e6dda5f9992597c67ee4bfb5acba7bf07535


def test_the_host_form_equals_the_reference_on_seeded_voters_and_at_the_scalar_edges():
    """the (sk, r) pairs of plume_cases.voters are re-drawn from its generator, so the expected values are the shared, cached ones"""
    voters = PC.voters(6)
    rng = PC.rng("voters-" + MSG.hex())
    pairs = [(rng.randrange(1, N), rng.randrange(1, N)) for _ in range(6)]
    for (sk, r), want in zip(pairs, voters):
        pk, nul, s, c, status, h = PL.sign_host(MSG, sk, r)
        assert (pk, nul, s, c) == want and status == 0 and h == R.hash_to_curve(MSG, pk)
    edges = [1, 2, N - 1, 1 << 255]
    for sk in edges:
        for r in edges:
            pk, nul, s, c, status, h = PL.sign_host(MSG, sk, r)
            assert (pk, nul, s, c) == R.gen(sk, MSG, r) and status == 0, (hex(sk), hex(r))
    for msg in (b"", bytes(range(34)), bytes(range(64))):
        sk, r = pairs[0]
        assert PL.sign_host(msg, sk, r)[:4] == R.gen(sk, msg, r)


def test_a_malformed_secret_gives_status_2_and_zeros():
    good = 0x1234567
    for bad in (0, N, PC.FULL):
        for sk, r in ((bad, good), (good, bad), (bad, bad)):
            assert PL.sign_host(MSG, sk, r) == ((0, 0), (0, 0), 0, 0, 2, (0, 0)), (hex(sk), hex(r))


def test_the_verifier_accepts_what_the_signer_signs():
    rng = PC.rng("sign-then-verify")
    for msg in (MSG, b"", bytes(range(64))):
        sk, r = rng.randrange(1, N), rng.randrange(1, N)
        pk, nul, s, c, status, h = PL.sign_host(msg, sk, r)
        assert status == 0 and PL.verify_host(msg, nul, pk, s, c) == (0, h)
        assert PL.verify_host(msg, nul, pk, s, (c + 1) % N)[0] == 1


def test_gen_native_equals_sign_host():
    rng = PC.rng("gen-native")
    for _ in range(3):
        sk, r = rng.randrange(1, N), rng.randrange(1, N)
        assert PL.gen_native(sk, MSG, r) == PL.sign_host(MSG, sk, r)[:4]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_the_host_call_refuses_null_pointers_and_long_messages(lib):
    sk, pk, nul, s, c, status = (C.c_uint64 * 4)(1), (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), C.c_uint32()
    good = [MSG, 2, sk, sk, pk, nul, s, c, C.addressof(status), None]
    assert lib.zkhip_plume_sign(*good) == 0, "h_out may be null"
    for at in (2, 3, 4, 5, 6, 7, 8):
        args = list(good)
        args[at] = None
        assert lib.zkhip_plume_sign(*args) == EINVAL, at
    assert lib.zkhip_plume_sign(bytes(65), 65, *good[2:]) == EINVAL and b"ZKHIP_PLUME_MAX_MSG" in lib.zkhip_last_error()
    assert lib.zkhip_plume_sign(None, 1, *good[2:]) == EINVAL
    assert lib.zkhip_plume_sign(None, 0, *good[2:]) == 0


def test_sign_device_refuses_messages_pointers_counts_and_overlaps(lib):
    sign = lib.zkhip_plume_sign_device
    assert sign(bytes(65), 65, *_sign_args()[2:]) == EINVAL and b"ZKHIP_PLUME_MAX_MSG" in lib.zkhip_last_error()
    assert sign(bytes(65), 65, None, None, 0, None, None, None, None, None, None, None) == EINVAL      # a count of zero does not excuse it
    assert sign(None, 2, *_sign_args()[2:]) == EINVAL
    for bad in (None, FAR[8] + 4, FAR[8] + 1):
        for at in (2, 3, 5, 6, 7, 8, 9):                       # sk, r, pk, nullifier, s, c, status
            args = _sign_args()
            args[at] = bad
            assert sign(*args) == EINVAL, (bad, at)
    for bad in (FAR[8] + 4, FAR[8] + 1):                       # d_h_out may be null, not misaligned
        args = _sign_args()
        args[10] = bad
        assert sign(*args) == EINVAL
    assert sign(*_sign_args(count=(1 << 30) + 1)) == EINVAL
    # every output against every input and every other output: first byte, last byte, containment
    n = 4
    size = {2: 32, 3: 32, 5: 64, 6: 64, 7: 32, 8: 32, 9: 4, 10: 64}
    for out in (5, 6, 7, 8, 9, 10):
        for other in size:
            if other == out:
                continue
            base = _sign_args(n)[other]
            for address in (base, base + n * size[other] - 8, base - n * size[out] + 8):
                args = _sign_args(n)
                args[out] = address
                assert sign(*args) == EINVAL, (out, other, hex(address))
    assert b"overlaps" in lib.zkhip_last_error()
    # a count of zero asks nothing of the arrays and enqueues nothing: no device is needed for it
    assert sign(MSG, 2, None, None, 0, None, None, None, None, None, None, None) == 0
    assert sign(None, 0, None, None, 0, None, None, None, None, None, None, None) == 0


def test_hash_points_device_refuses_layouts_pointers_counts_and_overlaps(lib):
    call = lib.zkhip_poseidon_hash_points_device
    assert call(FAR[0], 4, 2, FAR[1], None) == EINVAL and b"layout" in lib.zkhip_last_error()
    assert call(None, 0, 7, None, None) == EINVAL
    for layout in (0, 1):
        assert call(None, 4, layout, FAR[1], None) == EINVAL
        assert call(FAR[0], 4, layout, None, None) == EINVAL
        for off in (8, 4, 1):
            assert call(FAR[0] + off, 4, layout, FAR[1], None) == EINVAL
            assert call(FAR[0], 4, layout, FAR[1] + off, None) == EINVAL
        assert call(FAR[0], (1 << 30) + 1, layout, FAR[1], None) == EINVAL
        for out in (FAR[0], FAR[0] + 4 * 64 - 16, FAR[0] - 4 * 32 + 16):
            assert call(FAR[0], 4, layout, out, None) == EINVAL, hex(out)
        assert b"overlaps" in lib.zkhip_last_error()
        assert call(None, 0, layout, None, None) == 0


def test_the_refusals_need_no_device():
    """a fresh process in which HIP sees no device: the refusals are decided before it would be asked"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "from zksnap_circuits_halo2_amd import _lib\n"
            "lib = _lib.load()\n"
            "F = [0x700000001000 + (k << 24) for k in range(9)]\n"
            "assert lib.zkhip_plume_sign_device(bytes(65), 65, F[0], F[1], 4, F[2], F[3], F[4], F[5], F[6], None, None) == -1\n"
            "assert lib.zkhip_plume_sign_device(b'ab', 2, F[0], F[1], 4, F[2], F[3], F[4], F[5], F[6] + 4, None, None) == -1\n"
            "assert lib.zkhip_plume_sign_device(b'ab', 2, F[0], F[1], 4, F[2], F[2], F[4], F[5], F[6], None, None) == -1\n"
            "assert lib.zkhip_plume_sign_device(b'ab', 2, None, None, 0, None, None, None, None, None, None, None) == 0\n"
            "assert lib.zkhip_poseidon_hash_points_device(F[0], 4, 2, F[1], None) == -1\n"
            "assert lib.zkhip_poseidon_hash_points_device(F[0], 4, 0, F[0], None) == -1\n"
            "assert lib.zkhip_poseidon_hash_points_device(None, 0, 1, None, None) == 0\n"
            "print('refused without a device')\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0 and "refused without a device" in done.stdout, done.stdout + done.stderr

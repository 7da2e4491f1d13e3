"""CPU (`-m "not gpu"`): every refusal of the PLUME section of the C ABI is ZKHIP_EINVAL, decided on the host with nothing enqueued -- so it is
returned in a process that never initialises HIP: a null pointer where none is allowed, a message longer than ZKHIP_PLUME_MAX_MSG, a pointer
that is not 8-byte aligned, an output that overlaps another array.  A count of zero with null arrays is no refusal."""
import ctypes as C
import os

import pytest

import abi_header as AH
from zksnap_circuits_halo2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = 0x7000_0000_1000           # a non-null, 64-byte aligned address nothing lives at: a refused call never reads it
FAR = [FAKE + (k << 24) for k in range(8)]
MSG = bytes([1, 0])
NAMES = ("zkhip_secp256k1_lincomb_device", "zkhip_secp256k1_hash_to_curve_device", "zkhip_plume_verify_device", "zkhip_secp256k1_hash_to_curve", "zkhip_plume_verify")


def test_the_header_declares_the_section():
    assert AH.params("zkhip_secp256k1_lincomb_device") == ["const void *d_a", "const void *d_p", "const void *d_b", "const void *d_q", "size_t count", "void *d_out",
                                                           "void *d_status", "void *stream"]
    assert AH.params("zkhip_secp256k1_hash_to_curve_device") == ["const uint8_t *msg", "size_t msg_len", "const void *d_pk", "size_t count", "void *d_out", "void *d_status",
                                                                 "void *stream"]
    assert AH.params("zkhip_plume_verify_device") == ["const uint8_t *msg", "size_t msg_len", "const void *d_pk", "const void *d_nullifier", "const void *d_s",
                                                      "const void *d_c", "size_t count", "void *d_status", "void *d_report", "void *d_h_out", "void *stream"]
    for name in NAMES:
        assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported()
        assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"
    assert AH.defines()["ZKHIP_PLUME_MAX_MSG"] == _lib.ZKHIP_PLUME_MAX_MSG == 64
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    section = text[text.index("---- PLUME nullifiers on secp256k1"):text.index("---- parity hooks")]
    assert "struct" not in section.replace("zkhip_check_report", ""), "the section adds no struct"
    assert "QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_" in section


def test_zkhip_error_codes_are_what_this_file_assumes():
    assert AH.defines()["ZKHIP_EINVAL"] == EINVAL


def test_a_message_longer_than_the_limit_or_null_is_refused(lib):
    long = bytes(65)
    assert lib.zkhip_secp256k1_hash_to_curve_device(long, 65, FAR[0], 4, FAR[1], FAR[2], None) == EINVAL
    assert b"ZKHIP_PLUME_MAX_MSG" in lib.zkhip_last_error()
    assert lib.zkhip_plume_verify_device(long, 65, FAR[0], FAR[1], FAR[2], FAR[3], 4, FAR[4], FAR[5], None, None) == EINVAL
    assert lib.zkhip_plume_verify_device(long, 65, None, None, None, None, 0, None, FAR[5], None, None) == EINVAL      # a count of zero does not excuse it
    assert lib.zkhip_secp256k1_hash_to_curve_device(None, 2, FAR[0], 4, FAR[1], FAR[2], None) == EINVAL
    assert lib.zkhip_plume_verify_device(None, 2, FAR[0], FAR[1], FAR[2], FAR[3], 4, FAR[4], FAR[5], None, None) == EINVAL
    pk, out, status = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), C.c_uint32()
    assert lib.zkhip_secp256k1_hash_to_curve(long, 65, pk, out, C.addressof(status)) == EINVAL
    assert lib.zkhip_secp256k1_hash_to_curve(None, 1, pk, out, C.addressof(status)) == EINVAL
    s = (C.c_uint64 * 4)()
    assert lib.zkhip_plume_verify(long, 65, pk, pk, s, s, C.addressof(status), None) == EINVAL


def test_null_and_misaligned_pointers_are_refused(lib):
    for bad in (None, FAR[7] + 4, FAR[7] + 1):
        for at in (0, 1, 2, 3, 5, 6):                          # a, p, b, q, out, status
            args = [FAR[0], FAR[1], FAR[2], FAR[3], 4, FAR[4], FAR[5], None]
            args[at] = bad
            assert lib.zkhip_secp256k1_lincomb_device(*args) == EINVAL, (bad, at)
        for at in (2, 4, 5):                                   # pk, out, status
            args = [MSG, 2, FAR[0], 4, FAR[1], FAR[2], None]
            args[at] = bad
            assert lib.zkhip_secp256k1_hash_to_curve_device(*args) == EINVAL, (bad, at)
        for at in (2, 3, 4, 5, 7, 8):                          # pk, nullifier, s, c, status, report
            args = [MSG, 2, FAR[0], FAR[1], FAR[2], FAR[3], 4, FAR[4], FAR[5], None, None]
            args[at] = bad
            assert lib.zkhip_plume_verify_device(*args) == EINVAL, (bad, at)
    for bad in (FAR[7] + 4, FAR[7] + 1):                       # d_h_out may be null, not misaligned
        assert lib.zkhip_plume_verify_device(MSG, 2, FAR[0], FAR[1], FAR[2], FAR[3], 4, FAR[4], FAR[5], bad, None) == EINVAL
    # the report is written for no voters too
    assert lib.zkhip_plume_verify_device(MSG, 2, None, None, None, None, 0, None, None, None, None) == EINVAL
    assert lib.zkhip_plume_verify_device(MSG, 2, None, None, None, None, 0, None, FAR[5] + 4, None, None) == EINVAL
    # a count of zero asks nothing of the arrays and enqueues nothing: no device is needed for it
    assert lib.zkhip_secp256k1_lincomb_device(None, None, None, None, 0, None, None, None) == 0
    assert lib.zkhip_secp256k1_hash_to_curve_device(MSG, 2, None, 0, None, None, None) == 0
    assert lib.zkhip_secp256k1_hash_to_curve_device(None, 0, None, 0, None, None, None) == 0
    # the host calls
    pk, out, status, s = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), C.c_uint32(), (C.c_uint64 * 4)()
    assert lib.zkhip_secp256k1_hash_to_curve(MSG, 2, None, out, C.addressof(status)) == EINVAL
    assert lib.zkhip_secp256k1_hash_to_curve(MSG, 2, pk, None, C.addressof(status)) == EINVAL
    assert lib.zkhip_secp256k1_hash_to_curve(MSG, 2, pk, out, None) == EINVAL
    for at in (2, 3, 4, 5, 6):
        args = [MSG, 2, pk, pk, s, s, C.addressof(status), None]
        args[at] = None
        assert lib.zkhip_plume_verify(*args) == EINVAL, at


def test_an_output_that_overlaps_another_array_is_refused(lib):
    n = 4
    a, p, b, q, out, status = FAR[:6]
    # lincomb: d_out against every input (first byte, last byte, containment) and against d_status
    for o in (a, a + n * 32 - 8, a - n * 64 + 8, p, p + n * 64 - 8, b, q, q + 64, status, status - n * 64 + 8):
        assert lib.zkhip_secp256k1_lincomb_device(a, p, b, q, n, o, status, None) == EINVAL, hex(o)
    for st in (a, p + n * 64 - 8, b, q, out, out + n * 64 - 8, out - n * 4 + 8):
        assert lib.zkhip_secp256k1_lincomb_device(a, p, b, q, n, out, st, None) == EINVAL, hex(st)
    assert b"overlaps" in lib.zkhip_last_error()
    # hash_to_curve: the output IS the input is refused too (a lane's store is another call's load only by mistake)
    for o in (p, p + n * 64 - 8, p - n * 64 + 8, status):
        assert lib.zkhip_secp256k1_hash_to_curve_device(MSG, 2, p, n, o, status, None) == EINVAL, hex(o)
    # verify: status, report and h against the inputs and against each other
    pk, nul, s, c, st, rep, h = FAR[:7]
    for bad in (pk, nul + n * 64 - 8, s, c + n * 32 - 8, rep, rep - n * 4 + 8, h, h + n * 64 - 8):
        assert lib.zkhip_plume_verify_device(MSG, 2, pk, nul, s, c, n, bad, rep, h, None) == EINVAL, hex(bad)
    for bad in (pk, nul + n * 64 - 8, s, c, st, h + 64):
        assert lib.zkhip_plume_verify_device(MSG, 2, pk, nul, s, c, n, st, bad, h, None) == EINVAL, hex(bad)
    for bad in (pk, nul, s + 8, c, st - 8, rep - 8):
        assert lib.zkhip_plume_verify_device(MSG, 2, pk, nul, s, c, n, st, rep, bad, None) == EINVAL, hex(bad)
    assert lib.zkhip_plume_verify_device(MSG, 2, pk, nul, s, c, (1 << 30) + 1, st, rep, None, None) == EINVAL


def test_the_refusals_need_no_device():
    """a fresh process in which HIP sees no device: the refusals are decided before it would be asked"""
    import subprocess
    import sys

    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "from zksnap_circuits_halo2_amd import _lib\n"
            "lib = _lib.load()\n"
            "F = 0x700000001000\n"
            "assert lib.zkhip_plume_verify_device(bytes(65), 65, F, F + (1 << 24), F + (2 << 24), F + (3 << 24), 4, F + (4 << 24), F + (5 << 24), None, None) == -1\n"
            "assert lib.zkhip_secp256k1_lincomb_device(F, F + (1 << 24), F + (2 << 24), F + (3 << 24), 4, F, F + (5 << 24), None) == -1\n"
            "assert lib.zkhip_secp256k1_hash_to_curve_device(b'ab', 2, F + 4, 4, F + (1 << 24), F + (2 << 24), None) == -1\n"
            "assert lib.zkhip_secp256k1_lincomb_device(None, None, None, None, 0, None, None, None) == 0\n"
            "print('refused without a device')\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0 and "refused without a device" in done.stdout, done.stdout + done.stderr

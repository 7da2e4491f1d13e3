"""CPU: the transcript of include/zkhip.h ("transcript": halo2's Blake2bWrite / Blake2bRead with Challenge255) in a process without a GPU --
the hash and its framing against hashlib (tests/transcript_reference.py), the challenge reduction, the strict scalar reader, the round
trip through the proof bytes, and a C99 program through the header alone.  None of these calls may touch HIP."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bn254 as O
from transcript_reference import RefTranscript
from zksnap_circuits_halo2_amd import _lib, fields as F, multiopen as MO
from zksnap_circuits_halo2_amd.transcript import Blake2bRead, Blake2bWrite, decoded

R = O.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

PIN_FRESH = 0x0E89C2C9EF365F095EC7AA36500BB0BA58BF7D5E17194055AFB5A1C746F1786A
PIN_29 = 0x25568213223F071035F8DF44E2C9A0688DFD52B2E09D76EF6351F13B00CA3C70      # finalises exactly 128 bytes: a full last block
PIN_30 = 0x23C8DC750FB8A3CED8297C938ED895ED7DB39026663BE7247290DFA0A6DDBC70      # 129 bytes: the full block is now a non-final one
PIN_31 = 0x1215393609532AF43F5FF7B9085B1E5048CBB80F04BE2C3DB002CA4D3231536D


def affine(P):
    return F.g1_encode([P])[0]


def test_pinned_challenges():
    with Blake2bWrite() as t:
        assert t.squeeze_challenge() == PIN_FRESH
        t.common_scalar(1)
        t.common_point(affine(O.G1_GEN))
        got = [t.squeeze_challenge() for _ in range(31)]
        assert (got[28], got[29], got[30]) == (PIN_29, PIN_30, PIN_31)
        assert t.finalize() == b""                                                  # common_* and squeeze write nothing
    ref = RefTranscript()
    assert ref.squeeze() == PIN_FRESH                                               # the pins are hashlib's, too
    ref.common_scalar(1)
    ref.common_point(O.G1_GEN)
    got = [ref.squeeze() for _ in range(31)]
    assert ref.absorbed == 130 and (got[28], got[29], got[30]) == (PIN_29, PIN_30, PIN_31)


@pytest.mark.parametrize("k", range(9))
def test_scalars_then_squeeze_across_block_boundaries(k):
    """33 k + 1 bytes: crosses 128 at k = 4 and 256 at k = 8"""
    gen = O.SplitMix64(500 + k)
    scalars = [gen.fr() for _ in range(k)]
    ref = RefTranscript()
    with Blake2bWrite() as t:
        for s in scalars:
            ref.common_scalar(s)
        t.common_scalars(scalars)
        assert ref.absorbed == 33 * k
        assert t.squeeze_challenge() == ref.squeeze()
        assert t.squeeze_challenge() == ref.squeeze()


def interleaved(seed, ops, pad_to=None):
    """a seeded sequence of points, scalars and squeezes on the library and on hashlib; pad_to: squeeze when the absorbed bytes reach
    exactly that count minus the squeeze's own byte (squeezes are the only one-byte steps, so a count can always be hit with them)"""
    rng = random.Random(seed)
    gen = O.SplitMix64(seed)
    P = O.scalar_mul(gen.fr(), O.G1_GEN)
    ref = RefTranscript()
    hits = 0
    with Blake2bWrite() as t:
        for _ in range(ops):
            if pad_to and ref.absorbed % pad_to > pad_to - 66 and ref.absorbed % pad_to != 0:
                while (ref.absorbed + 1) % pad_to != 0:                             # walk up to the boundary with squeezes
                    assert t.squeeze_challenge() == ref.squeeze()
                assert t.squeeze_challenge() == ref.squeeze()                       # this one finalises a multiple of pad_to bytes
                assert ref.absorbed % pad_to == 0
                hits += 1
                continue
            what = rng.randrange(4)
            if what == 0:
                P = O.add(P, O.G1_GEN)
                ref.common_point(P)
                t.common_point(affine(P))
            elif what == 1:
                s = gen.fr()
                ref.write_scalar(s)
                t.write_scalar(s)
            elif what == 2:
                batch = [gen.fr() for _ in range(rng.randrange(1, 6))]
                for s in batch:
                    ref.common_scalar(s)
                t.common_scalars(batch)
            else:
                assert t.squeeze_challenge() == ref.squeeze()
        assert t.squeeze_challenge() == ref.squeeze()
        assert t.finalize() == ref.proof
    return hits


def test_interleaved_operations_match_hashlib():
    interleaved(0xA11CE, 300)


def test_interleaved_operations_with_squeezes_on_block_boundaries():
    assert interleaved(0xB0B, 300, pad_to=256) >= 5                                 # every multiple of 256 is a multiple of 128 as well


def reduce512(lib, data):
    out = np.zeros(4, dtype=np.uint64)
    assert lib.zkhip_test_reduce512(bytes(data), out.ctypes.data) == 0
    return F.fr_decode(out.reshape(1, 4))[0]


@pytest.mark.parametrize("value", [(1 << 512) - 1, R - 1, R, R + 1, 1 << 256, (1 << 256) * (R - 1), 0, (1 << 256) - 1, ((1 << 256) - 1) << 256],
                         ids=["all_ff", "r-1", "r", "r+1", "2^256", "2^256(r-1)", "zero", "low_half_ff", "high_half_ff"])
def test_challenge_reduction(lib, value):
    assert reduce512(lib, value.to_bytes(64, "little")) == value % R


def test_challenge_reduction_seeded(lib):
    rng = random.Random(77)
    for _ in range(200):
        v = rng.getrandbits(512)
        assert reduce512(lib, v.to_bytes(64, "little")) == v % R


def test_read_scalars_is_strict_and_failed_calls_change_nothing(lib):
    good = (R - 1).to_bytes(32, "little")
    for bad in (R, (1 << 256) - 1):
        with Blake2bRead(good + bad.to_bytes(32, "little") + good) as t, Blake2bRead(good) as twin:
            assert t.read_scalars(1) == [R - 1]                                     # r - 1 is accepted
            assert twin.read_scalars(1) == [R - 1]
            out = np.zeros((2, 4), dtype=np.uint64)
            assert lib.zkhip_transcript_read_scalars(t._t, 2, out.ctypes.data) == EINVAL      # the second of the two is good: nothing of the batch is taken
            assert b"scalar 0 of 2" in lib.zkhip_last_error()
            with pytest.raises(_lib.ZkhipError):
                t.read_scalar()
            assert t.squeeze_challenge() == twin.squeeze_challenge()               # neither the hash nor the cursor moved
    # past the end
    with Blake2bRead(good + b"\x01" * 31) as t, Blake2bRead(good) as twin:
        out = np.zeros((2, 4), dtype=np.uint64)
        assert lib.zkhip_transcript_read_scalars(t._t, 2, out.ctypes.data) == EINVAL
        assert t.read_scalar() == R - 1 and twin.read_scalar() == R - 1
        assert lib.zkhip_transcript_read_scalars(t._t, 1, out.ctypes.data) == EINVAL          # 31 bytes left
        assert t.squeeze_challenge() == twin.squeeze_challenge()
    with Blake2bRead(b"") as t:
        with pytest.raises(_lib.ZkhipError):
            t.read_scalar()
        assert t.squeeze_challenge() == PIN_FRESH


def test_round_trip_through_the_proof_bytes(lib):
    gen = O.SplitMix64(4242)
    scalars = [0, 1, R - 1, (1 << 256) % R] + [gen.fr() for _ in range(40)]
    with Blake2bWrite() as w:
        w.common_scalar(7)
        w.write_scalars(scalars[:3])
        c0 = w.squeeze_challenge()
        w.write_scalars(scalars[3:])
        c1 = w.squeeze_challenge()
        proof = w.finalize()
        n = C.c_size_t(12345)
        assert lib.zkhip_transcript_proof(w._t, None, 0, C.byref(n)) == 0 and n.value == 32 * len(scalars)
        small = C.create_string_buffer(16)
        assert lib.zkhip_transcript_proof(w._t, small, 16, C.byref(n)) == EINVAL and n.value == 32 * len(scalars)
        out = np.zeros(4, dtype=np.uint64)
        assert lib.zkhip_transcript_read_scalars(w._t, 1, out.ctypes.data) == EINVAL          # a writer does not read
    assert proof == b"".join(s.to_bytes(32, "little") for s in scalars)
    with Blake2bRead(proof) as r:
        r.common_scalar(7)
        assert r.read_scalars(3) == scalars[:3]
        assert r.squeeze_challenge() == c0
        assert r.read_scalars(len(scalars) - 3) == scalars[3:]
        assert r.squeeze_challenge() == c1
        assert r.proof() == proof
        w4 = F.fr_encode([1])
        assert lib.zkhip_transcript_write_scalars(r._t, w4.ctypes.data, 1) == EINVAL         # a reader does not write


def test_common_point_refuses_the_identity_and_stays_untouched(lib):
    pts = np.stack([affine(O.G1_GEN), np.zeros(8, dtype=np.uint64)])
    with Blake2bWrite() as t:
        assert lib.zkhip_transcript_common_points(t._t, pts.ctypes.data, 2) == EINVAL
        assert b"infinity" in lib.zkhip_last_error()
        assert t.squeeze_challenge() == PIN_FRESH
    assert lib.zkhip_transcript_new(2) is None and lib.zkhip_transcript_new_reader(b"", 0, -1) is None


def test_launch_shape_hook(lib):
    """the chunk of the points kernel's shared inversion doubles where tests/test_gpu_transcript.py expects it to"""
    shape = [lib.zkhip_test_transcript_chunk(n) for n in (1, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 1 << 20)]
    assert shape == [1, 1, 2, 2, 4, 4, 8, 8, 8, 8]


def test_c99_driver_reproduces_the_pin(tmp_path):
    exe = tmp_path / "transcript_driver"
    lib_dir = os.path.join(ROOT, "zksnap_circuits_halo2_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "transcript_driver.c"), "-o", str(exe), "-L", lib_dir, "-lzkhip", "-Wl,-rpath," + lib_dir])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert lines[-1] == "transcript driver OK"
    words = np.array([int(w, 16) for w in lines[0].split()], dtype=np.uint64)
    assert F.fr_decode(words.reshape(1, 4))[0] == PIN_FRESH


def test_cpp_mirror_transcript(tmp_path):
    """include/zkhip.hpp `Transcript`: the pin, and a scalar written and read back, from C++ without a GPU"""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include "zkhip.hpp"\nusing namespace zkhip::halo2;\n'
                   'int main() {\n'
                   '  Transcript w = Transcript::writer();\n'
                   '  const Fr c0 = w.squeeze_challenge();\n'
                   '  std::printf("%016llx %016llx %016llx %016llx\\n", (unsigned long long)c0.l[0], (unsigned long long)c0.l[1], (unsigned long long)c0.l[2], (unsigned long long)c0.l[3]);\n'
                   '  w.common_scalar(c0);\n'
                   '  w.write_scalars(std::vector<Fr>{c0, detail::one()});\n'
                   '  const Fr c1 = w.squeeze_challenge();\n'
                   '  const std::vector<uint8_t> proof = w.finalize();\n'
                   '  if (proof.size() != 64) return 2;\n'
                   '  Transcript r = Transcript::reader(proof);\n'
                   '  if (!(r.squeeze_challenge() == c0)) return 3;\n'
                   '  r.common_scalar(c0);\n'
                   '  const std::vector<Fr> back = r.read_scalars(2);\n'
                   '  if (!(back[0] == c0) || !(back[1] == detail::one()) || !(r.squeeze_challenge() == c1)) return 4;\n'
                   '  try { r.read_scalars(1); return 5; } catch (const std::runtime_error&) {}\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "t"
    lib_dir = os.path.join(ROOT, "zksnap_circuits_halo2_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lzkhip",
                           "-Wl,-rpath," + lib_dir])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    words = np.array([int(w, 16) for w in res.stdout.split()], dtype=np.uint64)
    assert F.fr_decode(words.reshape(1, 4))[0] == PIN_FRESH


# ---- the multi-opens' parts of a proof ---------------------------------------------------------------------------------------------------------
# Points of a transcript are decoded and normalised on the device, so the reading functions meet real proof bytes in
# tests/test_gpu_multiopen_reads.py; here a reader that records its calls shows the order, and what becomes of its errors.
class RecordingReader:
    """hands out 1, 2, 3 .. as challenges and as points, in the order of the calls; `fail`: (the call that raises, the error's code)"""

    def __init__(self, fail=None):
        self.calls, self.next, self.fail = [], 0, fail

    def _step(self, call, n=1):
        self.calls.append(call)
        if self.fail and len(self.calls) == self.fail[0]:
            raise _lib.ZkhipError(self.fail[1], "a stub's error")
        self.next += n
        return list(range(self.next - n + 1, self.next + 1))

    def squeeze_challenge(self):
        return self._step("squeeze")[0]

    def read_points(self, n, device=True):
        return np.array(self._step(("read", n, device), n), dtype=np.uint64)[:, None] * np.ones(8, dtype=np.uint64)


@pytest.mark.parametrize("device", [False, True])
def test_each_verifier_class_reads_its_part_in_its_provers_order(device):
    gwc, shplonk = RecordingReader(), RecordingReader()
    points, challenges = MO.VerifierGWC(None).read_proof(gwc, 3, device=device)
    assert gwc.calls == ["squeeze", ("read", 3, device), "squeeze"]
    assert [int(p[0]) for p in points] == [2, 3, 4] and challenges == (1, 5)                    # W_0 .., (v, u)
    points, challenges = MO.VerifierSHPLONK(None).read_proof(shplonk, 3, device=device)
    assert shplonk.calls == ["squeeze", "squeeze", ("read", 1, device), "squeeze", ("read", 1, device)]
    assert [int(p[0]) for p in points] == [5, 3] and challenges == (1, 2, 4)                    # [H', H], (y, v, u)


@pytest.mark.parametrize("verifier, last_read", [(MO.VerifierGWC, 2), (MO.VerifierSHPLONK, 5)])
def test_a_part_that_does_not_decode_is_none_and_other_errors_pass_through(verifier, last_read):
    cut = RecordingReader(fail=(last_read, EINVAL))
    assert decoded(verifier(None).read_proof, cut, 3) is None and len(cut.calls) == last_read  # nothing is asked of the reader after the failing read
    assert verifier(None).verify_proof_transcript([], RecordingReader(fail=(last_read, EINVAL))) is False
    for code in (-2, -3):
        with pytest.raises(_lib.ZkhipError) as other:
            decoded(verifier(None).read_proof, RecordingReader(fail=(last_read, code)), 3)
        assert other.value.code == code
        with pytest.raises(_lib.ZkhipError):
            verifier(None).verify_proof_transcript([], RecordingReader(fail=(last_read, code)))

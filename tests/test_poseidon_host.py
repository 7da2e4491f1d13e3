"""CPU: Poseidon over Fr (include/zkhip.h, "Poseidon") in a process without a GPU -- the pins of the header through the C ABI, the constants the
library's Grain makes against those of the restatement (tests/poseidon_reference.py), the sponge and the Poseidon transcript against it, and
the Blake2b transcript's pin, which routing by hash must not move.  None of these calls may touch HIP."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import poseidon_reference as PR
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F, poseidon as PS
from zksnap_circuits_halo2_amd.transcript import Blake2bRead, Blake2bWrite, PoseidonRead, PoseidonWrite

R, Q = O.R_MOD, F.Q_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

PERM_012 = (0x115cc0f5e7d690413df64c6b9662e9cf2a3617f2743245519e19607a4417189a,
            0x0fca49b798923ab0239de1c9e7a4a9a2210312b6a2f616d18b5a87f9b628ae29,
            0x0e7ae82e40091e63cbd4f16a6d16310b3729d4b6e138fcf54110e2867045a30c)
CIRCOMLIB_POSEIDON_1_2 = 7853200120776062878684798364095072458815029376092732009249414926327459813530
RC_0_0 = 0x0ee9a592ba9a9518d05986d656f40c2114c4993c11bb29938d21d47304cd8e6e
RC_64_2 = 0x1da55cc900f0d21f4a3e694391918a1b3c23b2ac773c6b3ef88e2e4228325161
M_0_0 = 0x109b7f411ba0e4c9b2b70caf5c36a7b194be7c11ad24378bfedb68592ba8118b
M_2_2 = 0x19a3fc0a56702bf417ba7fee3802593fa644470307043f7773279cd71d25d5e0
FRESH = 0x14b2e5484b232721d64f405caa487febbce835dd07c5de940f2a775dc9aa0da6
FRESH_SECOND = 0x1f0db93536afb96e038f897b4fb5548b6aa3144c46893a6459c4b847951a23b4
HASHES = {(1,): 0x0852dd5e76ddcfab001c178a8e3ff6e40ed9c34bf8fd53868704c7ca58042de1,
          (1, 2): 0x305df2f9f9f1c0b591427aa9fd8ff8b8b8ad8a16953065fca066cb6a69deff53,
          (1, 2, 3): 0x1e771e80490bde52a453e40889e14665d5396a81ff3076ac798ce39ef71b6cf1,
          (0, 0): 0x2b2ceb8eb042a119d745d0d54ba961a45e20a1b94cf2195b11a7076780eeb04f,
          (R - 1, R - 1): 0x2d88e5e300b4872c95eb4750ac19ee3f65bf86a5c88a24ac0f0e452e0ae5602b}
UPDATE_12_SQUEEZE_UPDATE_3 = 0x115f9d49c89f19c874d20e4de0ab67ac6f18e1beea44371b84c540138465ace4
ROOT_1234 = 0x2c01ebd821c7ffc51531dc18169a856bfa0e54c4f5ff99b94f328a38d57d2194
BLAKE2B_FRESH = 0x0E89C2C9EF365F095EC7AA36500BB0BA58BF7D5E17194055AFB5A1C746F1786A


def affine_raw(x, y):
    """8 Montgomery limbs of the pair (x, y) as Fq elements, on the curve or not: the transcript's host calls do not ask"""
    return F.g1_encode([(x, y)])[0]


def test_permutation_pins(lib):
    assert tuple(PS.permute([(0, 1, 2)])[0]) == PERM_012
    assert PERM_012[0] == CIRCOMLIB_POSEIDON_1_2
    assert tuple(PR.permute([0, 1, 2])) == PERM_012                                 # the restatement reproduces the published vector as well


def test_constants_are_the_restatements(lib):
    rc, mds = PS.constants()
    assert rc == PR.ROUND_CONSTANTS and mds == PR.MDS
    assert len(rc) == 65 and all(len(r) == 3 for r in rc) and sum(len(r) for r in rc) + 9 == 204
    assert (rc[0][0], rc[64][2], mds[0][0], mds[2][2]) == (RC_0_0, RC_64_2, M_0_0, M_2_2)
    assert all(c < R for r in rc for c in r)


def test_sponge_pins(lib):
    assert PS.hash([]) == FRESH
    for msg, want in HASHES.items():
        assert PS.hash(list(msg)) == want, msg
    with PoseidonWrite() as t:
        assert t.squeeze_challenge() == FRESH
        assert t.squeeze_challenge() == FRESH_SECOND                                # the state carries on
    with PoseidonWrite() as t:
        t.common_scalars([1, 2])
        t.squeeze_challenge()
        t.common_scalar(3)
        assert t.squeeze_challenge() == UPDATE_12_SQUEEZE_UPDATE_3
    assert PR.merkle_levels([1, 2, 3, 4])[-1] == [ROOT_1234]
    assert PS.hash([PS.hash([1, 2]), PS.hash([3, 4])]) == ROOT_1234


@pytest.mark.parametrize("length", range(8))
def test_sponge_against_the_restatement(lib, length):
    rng = random.Random(900 + length)
    pool = [0, 1, R - 1]
    cases = [[v] * length for v in pool] + [[rng.choice(pool + [rng.randrange(R)]) for _ in range(length)] for _ in range(4)]
    for msg in cases:
        assert PS.hash(msg) == PR.hash(*msg), msg


@pytest.mark.parametrize("n", [0, 1, 5])
def test_permute_batches(lib, n):
    rng = random.Random(n)
    states = [[rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(3)] for _ in range(n)]
    assert PS.permute(states) == [PR.permute(s) for s in states]
    assert lib.zkhip_poseidon_permute(None, 0) == 0 and lib.zkhip_poseidon_permute(None, 1) == EINVAL


def test_transcript_against_the_reference_transcript(lib):
    """common_*, write_scalars, read_scalars and squeeze; one coordinate is >= r, so that the reduction mod r shows"""
    rng = random.Random(31337)
    big_x = R + 5                                                                   # below q: a canonical Fq coordinate that is not a canonical Fr
    assert R <= big_x < Q
    points = [O.G1_GEN, (big_x, 11), (Q - 1, R - 1), O.scalar_mul(77, O.G1_GEN)]
    scalars = [0, 1, R - 1] + [rng.randrange(R) for _ in range(6)]
    ref = PR.Transcript()
    with PoseidonWrite() as w:
        assert w.squeeze_challenge() == ref.squeeze()
        for P in points:
            w.common_point(affine_raw(*P))
            ref.common_point(*P)
            assert w.squeeze_challenge() == ref.squeeze()
        unreduced = PR.Transcript()
        unreduced.sponge.update(big_x, 11)
        reduced = PR.Transcript()
        reduced.sponge.update(5, 11)
        assert unreduced.squeeze() == reduced.squeeze()                             # what "mod r" means for the restatement
        w.common_scalars(scalars[:2])
        for s in scalars[:2]:
            ref.common_scalar(s)
        w.write_scalars(scalars[2:])                                                # an odd count: the next squeeze pads a half chunk
        for s in scalars[2:]:
            ref.common_scalar(s)
        c0 = w.squeeze_challenge()
        assert c0 == ref.squeeze()
        w.write_scalar(c0)
        ref.common_scalar(c0)
        c1 = w.squeeze_challenge()
        assert c1 == ref.squeeze()
        proof = w.finalize()
    assert proof == b"".join(s.to_bytes(32, "little") for s in scalars[2:] + [c0])  # the bytes a Blake2b writer appends
    with Blake2bWrite() as b:
        b.write_scalars(scalars[2:] + [c0])
        assert b.finalize() == proof
    with PoseidonRead(proof) as r:
        r.squeeze_challenge()
        for P in points:
            r.common_point(affine_raw(*P))
            r.squeeze_challenge()
        r.common_scalars(scalars[:2])
        assert r.read_scalars(len(scalars) - 2) == scalars[2:]
        assert r.squeeze_challenge() == c0
        assert r.read_scalar() == c0
        assert r.squeeze_challenge() == c1
        out = np.zeros(4, dtype=np.uint64)
        assert lib.zkhip_transcript_write_scalars(r._t, out.ctypes.data, 1) == EINVAL          # a reader does not write


def test_transcript_point_pins_and_the_refused_identity(lib):
    with PoseidonWrite() as t:
        t.common_point(affine_raw(1, 2))
        assert t.squeeze_challenge() == HASHES[(1, 2)]
    pts = np.stack([affine_raw(1, 2), np.zeros(8, dtype=np.uint64)])
    with PoseidonWrite() as t, PoseidonWrite() as twin:
        assert lib.zkhip_transcript_common_points(t._t, pts.ctypes.data, 2) == EINVAL          # the first of the two is good: nothing of the batch is taken
        assert b"infinity" in lib.zkhip_last_error()
        assert t.squeeze_challenge() == twin.squeeze_challenge() == FRESH
    assert lib.zkhip_transcript_new_poseidon(2) is None and lib.zkhip_transcript_new_poseidon_reader(b"", 0, -1) is None


def test_read_scalars_is_strict_and_failed_calls_change_nothing(lib):
    good = (R - 1).to_bytes(32, "little")
    with PoseidonRead(good + R.to_bytes(32, "little") + good) as t, PoseidonRead(good) as twin:
        assert t.read_scalars(1) == [R - 1] and twin.read_scalars(1) == [R - 1]
        out = np.zeros((2, 4), dtype=np.uint64)
        assert lib.zkhip_transcript_read_scalars(t._t, 2, out.ctypes.data) == EINVAL
        assert t.squeeze_challenge() == twin.squeeze_challenge() == PR.hash(R - 1)


def test_blake2b_transcript_is_where_it_was(lib):
    with Blake2bWrite() as t:
        assert t.squeeze_challenge() == BLAKE2B_FRESH
    with Blake2bRead(b"") as t:
        assert t.squeeze_challenge() == BLAKE2B_FRESH


def test_device_calls_validate_before_they_touch_a_gpu(lib):
    """bad widths and leaf counts are refused on the host: no HIP call is reached (this process has no GPU)"""
    buf = (C.c_uint64 * 64)()
    p = C.addressof(buf) & ~15
    for width in (0, PS.MAX_WIDTH + 1):
        assert lib.zkhip_poseidon_hash_many_device(p, 1, width, p, None) == EINVAL
    for n in (0, 3, 6, (1 << 30) + 1, 1 << 31):
        assert lib.zkhip_poseidon_merkle_device(p, n, p, None) == EINVAL
        assert b"power of two" in lib.zkhip_last_error()
    assert lib.zkhip_poseidon_merkle_device(p + 8, 2, p, None) == EINVAL
    assert lib.zkhip_poseidon_merkle_device(p, 1, None, None) == 0                 # one leaf: the root is the leaf, nothing to write
    assert (PS.MAX_WIDTH, PS.SUBTREE) == (16, 256)


def test_cpp_mirror_poseidon(tmp_path):
    """include/zkhip.hpp `Poseidon` and the Poseidon `Transcript`: the pins from C++ without a GPU"""
    src = tmp_path / "p.cpp"
    src.write_text('#include <cstdio>\n#include "zkhip.hpp"\nusing namespace zkhip::halo2;\n'
                   'static void show(const Fr& c) { std::printf("%016llx %016llx %016llx %016llx\\n", (unsigned long long)c.l[0], (unsigned long long)c.l[1], (unsigned long long)c.l[2], (unsigned long long)c.l[3]); }\n'
                   'int main() {\n'
                   '  show(Poseidon::hash({detail::from_u64(1), detail::from_u64(2)}));\n'
                   '  Transcript w = Transcript::poseidon_writer();\n'
                   '  show(w.squeeze_challenge());\n'
                   '  Fr st[3] = {detail::from_u64(0), detail::from_u64(1), detail::from_u64(2)};\n'
                   '  Poseidon::permute(st);\n'
                   '  show(st[0]);\n'
                   '  w.write_scalars(std::vector<Fr>{st[0]});\n'
                   '  const Fr c = w.squeeze_challenge();\n'
                   '  Transcript r = Transcript::poseidon_reader(w.finalize());\n'
                   '  r.squeeze_challenge();\n'
                   '  if (!(r.read_scalars(1)[0] == st[0]) || !(r.squeeze_challenge() == c)) return 2;\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "p"
    lib_dir = os.path.join(ROOT, "zksnap_circuits_halo2_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lzkhip",
                           "-Wl,-rpath," + lib_dir])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    got = [F.fr_decode(np.array([int(w, 16) for w in line.split()], dtype=np.uint64).reshape(1, 4))[0] for line in res.stdout.splitlines()]
    assert got == [HASHES[(1, 2)], FRESH, PERM_012[0]]

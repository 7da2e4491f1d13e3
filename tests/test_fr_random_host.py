"""CPU: the random Fr stream of include/zkhip.h ("random field elements"), restated here and compared word for word with a host build of
csrc/fr_random.hpp -- the per-element function the device kernels call -- under ASan + UBSan.

The restatement is a ChaCha20 written below in numpy (pinned by the block of RFC 8439 section 2.3.2) and a reduction mod r in Python's big
integers; `restate` is also what tests/test_gpu_fr_random.py compares the device's columns with."""
import os
import random
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SEED = bytes(range(32))
M64 = (1 << 64) - 1
# (first, stream_id, stored words as a 256-bit number), seed bytes 00 01 .. 1f
PINS = [
    (0x0900000000000001, 0x4A000000, 0x25312D9BE543D4C7A1D921E13F01589A414C389165C4CAD2B5E970BF8F628F64),
    (0, 0, 0x2DF7496ECA799E16CE3D4B34E4002E395ECBAF692C663DC252F2060930C43D94),
    (0xFFFFFFFF, 0x0123456789ABCDEF, 0x2F0B8A99903CB76BFDF69C3543739D5554D6024036E5C19E80FC1FC65ACA83F6),
]
RFC_VALUE = 0x099D737C79BEA952E4C9671A82BAA6DE853AF4F7694E36C4E5577D4AE6D300C5


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def chacha20_blocks(seed: bytes, stream_id: int, counters) -> np.ndarray:
    """(n, 16) uint32: the output words of the 20-round ChaCha20 blocks with key `seed`, 64-bit block counters `counters` (words 12, 13) and the
    64-bit `stream_id` in words 14, 15"""
    counters = np.asarray(counters, dtype=np.uint64).reshape(-1)
    n = counters.shape[0]
    init = np.empty((16, n), dtype=np.uint32)
    init[0:4] = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)[:, None]
    init[4:12] = np.frombuffer(seed, dtype="<u4").astype(np.uint32)[:, None]
    init[12] = (counters & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    init[13] = (counters >> np.uint64(32)).astype(np.uint32)
    init[14] = np.uint32(stream_id & 0xFFFFFFFF)
    init[15] = np.uint32(stream_id >> 32)
    x = init.copy()

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def quarter(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        quarter(0, 4, 8, 12); quarter(1, 5, 9, 13); quarter(2, 6, 10, 14); quarter(3, 7, 11, 15)
        quarter(0, 5, 10, 15); quarter(1, 6, 11, 12); quarter(2, 7, 8, 13); quarter(3, 4, 9, 14)
    return np.ascontiguousarray((x + init).T)


def restate_values(seed: bytes, stream_id: int, indices):
    """the elements at `indices` of stream (seed, stream_id) as plain integers in [0, r)"""
    blocks = chacha20_blocks(seed, stream_id, indices)
    return [int.from_bytes(row.astype("<u4").tobytes(), "little") % R_MOD for row in blocks]


def restate(seed: bytes, stream_id: int, indices) -> np.ndarray:
    """(n, 4) uint64: the elements at `indices` as the library stores them (Montgomery-256, canonical, little-endian words)"""
    out = np.empty((len(indices), 4), dtype=np.uint64)
    for i, v in enumerate(restate_values(seed, stream_id, indices)):
        s = (v << 256) % R_MOD
        out[i] = [(s >> (64 * j)) & M64 for j in range(4)]
    return out


def stored_number(words) -> int:
    return sum(int(w) << (64 * j) for j, w in enumerate(words))


# ---- the restatement itself is pinned ---------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_rfc_8439_block_and_the_pins():
    first, stream_id, stored = PINS[0]
    blk = chacha20_blocks(SEED, stream_id, [first])[0]
    assert [int(w) for w in blk[:4]] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3] and int(blk[15]) == 0x4E3C50A2
    rfc = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert blk.astype("<u4").tobytes() == rfc
    assert restate_values(SEED, stream_id, [first]) == [RFC_VALUE]
    for first, stream_id, stored in PINS:
        assert stored_number(restate(SEED, stream_id, [first])[0]) == stored, hex(first)


# ---- the library's per-element function, on the host, under the sanitizers ---------------------------------------------------------------
def _requests():
    """(seed, stream_id, first, n): a few hundred seeded triples around the pins and the edges of the two counters"""
    reqs = [(SEED, sid, first, 1) for first, sid, _ in PINS]
    for sid in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, M64):
        reqs.append((SEED, sid, (1 << 32) - 3, 6))                 # the block counter crosses 2^32 inside the run
        reqs.append((SEED, sid, M64, 1))                           # the last index of the stream
        reqs.append((SEED, sid, M64 - 3, 4))
        reqs.append((SEED, sid, (1 << 63) - 2, 4))
    rng = random.Random(0xC4AC4A20)
    for t in range(300):
        seed = bytes(rng.randrange(256) for _ in range(32)) if t % 3 else bytes([rng.randrange(256)] * 32)
        sid = rng.choice([rng.randrange(1 << 64), rng.randrange(1 << 32), (1 << 32) - rng.randrange(3), M64 - rng.randrange(3)])
        first = rng.choice([rng.randrange(1 << 64), rng.randrange(1 << 20), (1 << 32) - rng.randrange(1, 4), M64 - rng.randrange(2, 5)])
        reqs.append((seed, sid, first, rng.randrange(1, 4)))
    return reqs


def test_fr_random_hpp_on_the_host_with_sanitizers_equals_the_restatement(tmp_path):
    exe = tmp_path / "fr_random_host_check"
    build = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "fr_random_host_check.cpp"), "-o", str(exe)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert build.returncode == 0, build.stdout
    reqs = _requests()
    assert len(reqs) >= 300
    text = "".join(f"{seed.hex()} {sid:x} {first:x} {n}\n" for seed, sid, first, n in reqs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.split()
    # the two new constants of bn254_constants.hpp
    assert lines[0] == "C" and int(lines[1], 16) == pow(2, 517, R_MOD) and int(lines[2], 16) == pow(2, 773, R_MOD)
    got = [int(x, 16) for x in lines[3:]]
    want = []
    for seed, sid, first, n in reqs:
        want += [stored_number(w) for w in restate(seed, sid, [first + j for j in range(n)])]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"element {i}: {g:064x} != {w:064x}"
    assert got[:3] == [p[2] for p in PINS]
    assert all(g < R_MOD for g in got)                                                     # canonical

"""CPU (`-m "not gpu"`): the scalars mod n of csrc/secp256k1.hpp -- sk_scalar_reduce512 / mul / add / muladd / from_digest, the arithmetic of
s = r + sk c under the signing kernel -- compiled for the host under ASan + UBSan (tests/cpp/secp256k1_scalar_host_check.cpp) and compared,
value by value, with Python's `%`: 512-bit inputs at 0, n - 1, n, n + 1, 2^256 - 1, 2^256, (n - 1)^2, (2^256 - 1)^2, 2^512 - 1,
(2^256 - 1) 2^256 and at the inputs that make each fold's carry largest (the header's REDUCTION DISCIPLINE, bounds (1) to (4)), the operand
edges of muladd, the digest edges, a few thousand seeded cases, and one voter through the host form of the signer."""
import os
import subprocess

import pytest

import plume_cases as PC
import plume_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
N = R.N
FULL = PC.FULL
DELTA = (1 << 256) - N


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("secp256k1_scalar") / "secp256k1_scalar_host_check"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    build = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "secp256k1_scalar_host_check.cpp"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
    assert build.returncode == 0, build.stdout

    def call(lines):
        done = subprocess.run([str(out)], input="".join(line + "\n" for line in lines), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
        assert done.returncode == 0 and f"secp256k1 scalar host check done: {len(lines)} lines" in done.stdout, done.stdout[-4000:]
        return [[int(x, 16) for x in row.split()] for row in done.stdout.splitlines()[:len(lines)]]

    return call


def _folds(t):
    """the carries the header's folds see for the 512-bit input t: (hi1, hi2, the wrap of fold (3))"""
    t1 = (t & FULL) + (t >> 256) * DELTA
    t2 = (t1 & FULL) + (t1 >> 256) * DELTA
    t3 = (t2 & FULL) + (t2 >> 256) * DELTA
    return t1 >> 256, t2 >> 256, t3 >> 256


def _unfold(t_next):
    """a value lo + hi 2^256 with lo < delta whose fold lo + hi delta is t_next"""
    hi, lo = divmod(t_next, DELTA)
    assert hi <= FULL
    return lo + (hi << 256)


def largest_carry_inputs():
    """inputs at which each fold's carry is as large as its bound in the header allows"""
    top = (1 << 512) - 1
    assert _folds(top)[0] == DELTA and _folds(top)[1] == 2, "bounds (1) and (2) are met by 2^512 - 1: hi1 = delta, hi2 = 2"
    # fold (3) wraps only when the low words before it are within 2 delta of 2^256: build T2 = 2^257 - 1 (hi2 = 1, low words all ones), and
    # T2 = 3 * 2^256 - 1 (hi2 = 2), from below
    # hi2 = 2 leaves low words below 0.62 * 2^256 (bound (2)), which fold (3) cannot wrap; with hi2 = 1 it wraps when the low words are
    # within delta of 2^256.  T2 = 2^257 - 1 (all ones: the largest wrap), 2^257 - delta (the sum is exactly 2^256) and one less (no wrap,
    # the sum 2^256 - 1 >= n: the last subtraction alone), each reached from a 512-bit input through folds (1) and (2) backwards.
    out = [top]
    for t2 in ((1 << 257) - 1, (1 << 257) - DELTA, (1 << 257) - DELTA - 1):
        hi1 = min(t2 // DELTA, DELTA - 1)
        lo1 = t2 - hi1 * DELTA
        assert 0 <= lo1 <= FULL
        t = _unfold(lo1 + (hi1 << 256))
        assert ((t & FULL) + (t >> 256) * DELTA, _folds(t)[1]) == (lo1 + (hi1 << 256), 1)
        out.append(t)
    assert [_folds(t)[2] for t in out] == [0, 1, 1, 0]
    return out


def test_reduce512_at_its_edges_and_largest_carries(run):
    edges = [0, 1, N - 1, N, N + 1, FULL, 1 << 256, (1 << 256) + 1, (N - 1) ** 2, N * N, FULL * FULL, (1 << 512) - 1, FULL << 256, N << 256, (N - 1) << 256, 1 << 511,
             DELTA, DELTA << 256, (DELTA << 256) + FULL, 2 * N, 2 * N - 1, 3 * N - 1]
    cases = edges + largest_carry_inputs()
    got = run([f"red {t:x}" for t in cases])
    for t, (value,) in zip(cases, got):
        assert value == t % N, hex(t)


def test_muladd_mul_add_take_any_256_bit_operand(run):
    values = [0, 1, N - 1, N, FULL]
    cases = [(a, b, c) for a in values for b in values for c in values]
    got = run([f"ops {a:x} {b:x} {c:x}" for a, b, c in cases])
    for (a, b, c), row in zip(cases, got):
        assert row == [(a * b + c) % N, a * b % N, (a + b) % N, a % N], (hex(a), hex(b), hex(c))


def test_from_digest_reads_big_endian_and_reduces(run):
    rng = PC.rng("scalar-digest")
    values = [N - 1, N, FULL, 0, 1, N + 1, 1 << 255, 0x0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20] + [rng.getrandbits(256) for _ in range(16)]
    got = run([f"dig {d:064x}" for d in values])
    for d, (value,) in zip(values, got):
        assert value == d % N, hex(d)


def test_seeded_random_cases(run):
    rng = PC.rng("scalar-random")
    wide = [rng.getrandbits(512) for _ in range(2000)] + [rng.getrandbits(rng.randrange(1, 513)) for _ in range(500)]
    got = run([f"red {t:x}" for t in wide])
    assert [row[0] for row in got] == [t % N for t in wide]
    triples = [(rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256)) for _ in range(2000)]
    triples += [(N - rng.randrange(1, 4), FULL - rng.randrange(4), rng.getrandbits(256)) for _ in range(200)]
    got = run([f"ops {a:x} {b:x} {c:x}" for a, b, c in triples])
    for (a, b, c), row in zip(triples, got):
        assert row == [(a * b + c) % N, a * b % N, (a + b) % N, a % N], (hex(a), hex(b), hex(c))


def test_one_voter_through_the_host_form_of_the_signer(run):
    rng = PC.rng("scalar-sign")
    sk, r = rng.randrange(1, N), rng.randrange(1, N)
    lines = [f"sign {PC.MSG.hex()} {sk:x} {r:x}", f"sign - {sk:x} {r:x}", f"sign {PC.MSG.hex()} 0 {r:x}", f"sign {PC.MSG.hex()} {sk:x} {N:x}"]
    got = run(lines)
    for msg, row in zip((PC.MSG, b""), got):
        pk, nul, s, c = R.gen(sk, msg, r)
        assert row == [0, *pk, *nul, s, c, *R.hash_to_curve(msg, pk)]
    assert got[2] == [2] + [0] * 8 and got[3] == [2] + [0] * 8

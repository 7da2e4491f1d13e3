"""CPU (`-m "not gpu"`): csrc/modn.hpp -- the run-time-modulus Montgomery arithmetic under the Paillier kernels -- compiled for the host under
ASan + UBSan (tests/cpp/modn_host_check.cpp) and compared, value by value, with Python integers: the context builder (n^2, -N^-1 mod 2^32,
R mod N, R^2 mod N), `modn_to_mont`, `modn_from_mont`, `modn_mul` with one unreduced factor and with two reduced ones, and `modn_pow`.
Moduli: n = 3, a 176-bit n, n = 2^192 - 237 (n^2 just under 2^384: the carry word) and n = 2^32 k + 1 (the low limb of n^2 is 1); operands
0, 1, N - 1, N, 2^384 - 1 in every pair, and random ones."""
import os
import subprocess

import pytest

import paillier_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
R = 1 << 384


def _run(cmd, **kw):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600, **kw)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("modn") / "modn_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "modn_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return str(out)


def _cases(n):
    rng = PC.rng(f"modn-{n}")
    N = n * n
    edges = PC.edge_operands(n)
    exps = [0, 1, 2, (1 << 256) - 1, n, rng.getrandbits(256)]
    cases = [(a, b, exps[(i + j) % len(exps)]) for i, a in enumerate(edges) for j, b in enumerate(edges)]
    for _ in range(12):
        cases.append((rng.getrandbits(384), rng.getrandbits(384), rng.getrandbits(256)))
        cases.append((rng.randrange(N), rng.randrange(N), rng.getrandbits(rng.randrange(1, 257))))
    return cases


def _expected(n, a, b, e):
    N = n * n
    return [N, (-pow(N, -1, 1 << 32)) % (1 << 32), R % N, R * R % N, a * R % N, a * pow(R, -1, N) % N, a * b % N, a * b * R % N, pow(a, e, N)]


@pytest.mark.parametrize("name", sorted(PC.MODULI))
def test_modn_agrees_with_python_integers(exe, name):
    n = PC.MODULI[name]
    cases = _cases(n)
    run = _run([exe], input="".join(f"{n:x} {a:x} {b:x} {e:x}\n" for a, b, e in cases))
    assert run.returncode == 0 and f"modn host check done: {len(cases)} cases" in run.stdout, run.stdout
    lines = run.stdout.splitlines()[:len(cases)]
    for (a, b, e), line in zip(cases, lines):
        assert [int(x, 16) for x in line.split()] == _expected(n, a, b, e), (name, hex(a), hex(b), hex(e))


def test_the_context_builder_refuses_what_montgomery_cannot_take(exe):
    """an even modulus has no inverse mod 2^32; N < 3 leaves no room for 1 < N"""
    run = _run([exe], input="2 1 1 1\n0 1 1 1\n1 0 0 0\n100000000000000000000000000000000000000000000 5 7 3\n3 5 7 3\n")
    assert run.returncode == 0, run.stdout
    lines = run.stdout.splitlines()
    assert lines[:4] == ["refused"] * 4 and [int(x, 16) for x in lines[4].split()] == _expected(3, 5, 7, 3), run.stdout

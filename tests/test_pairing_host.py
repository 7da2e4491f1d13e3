"""CPU: the pairing arithmetic of csrc/pairing.hpp, built with the host compiler under ASan + UBSan (its single-lane policy), against the
independent big-integer pairing of tests/pairing_reference.py -- which is pinned here first: the curve parameters from x, the order and the
bilinearity of e(G, H) for the EIP-196 / EIP-197 generators that oracle/bn254.py pins."""
import os
import re
import subprocess

import pytest

import pairing_reference as P
import pairing_vectors as V
from oracle import bn254 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


# ---- the reference is pinned -------------------------------------------------------------------------------------------------------------
def test_curve_parameters_come_from_x():
    x = 4965661367192848881
    assert P.X_BN == x
    assert P.Q == 36 * x**4 + 36 * x**3 + 24 * x**2 + 6 * x + 1 == O.Q_MOD
    assert P.R == 36 * x**4 + 36 * x**3 + 18 * x**2 + 6 * x + 1 == O.R_MOD
    assert P.ATE == 6 * x + 2 and P.ATE.bit_length() == 65
    assert P.G1 == O.G1_GEN and P.G2 == O.G2_GEN and P.g2_on_twist(P.G2)
    assert P.TWIST_B == O.G2_B


@pytest.fixture(scope="module")
def e_gh():
    return P.pairing(P.G1, P.G2)


def test_reference_pairing_has_order_r(e_gh):
    assert e_gh != P.ONE
    assert P.f12_pow(e_gh, P.R) == P.ONE


def test_reference_pairing_is_bilinear(e_gh):
    scalars = V.EDGE_SCALARS
    for a, b in zip(scalars, scalars[2:] + scalars[:2]):
        assert P.pairing(P.g1_mul(a, P.G1), P.g2_mul(b, P.G2)) == P.f12_pow(e_gh, a * b % P.R), (a, b)


def test_basis_map_round_trips():
    for t in V.elements():
        assert P.to_tower(P.from_tower(t)) == t
    # v = w^2 and xi = v^3 = 9 + u in the flat ring
    v = P.from_tower([[(0, 0), (1, 0), (0, 0)], [(0, 0)] * 3])
    assert P.f12_mul(P.f12_mul(v, v), v) == P.from_tower([[(9, 1), (0, 0), (0, 0)], [(0, 0)] * 3])


def test_hard_part_chain_is_the_hard_part():
    """the exponents of the chain in pairing.hpp's final_exponentiation, as integers: y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 = (q^4 - q^2 + 1) / r"""
    x, q, r = P.X_BN, P.Q, P.R
    y0, y1, y2, y3 = q + q**2 + q**3, -1, x**2 * q**2, -(x * q)
    y4, y5, y6 = -(x + x**2 * q), -(x**2), -(x**3 + x**3 * q)
    e = y0 + 2 * y1 + 6 * y2 + 12 * y3 + 18 * y4 + 30 * y5 + 36 * y6
    assert e * r == q**4 - q**2 + 1


# ---- the generated constants -----------------------------------------------------------------------------------------------------------------
def test_generated_frobenius_constants():
    text = open(os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc", "pairing_constants.hpp")).read()
    arrays = {m.group(1): [int(w, 16) for w in re.findall(r"0x([0-9a-f]+)u", m.group(2))]
              for m in re.finditer(r"static constexpr uint32_t (\w+)\[9\] = \{([^}]*)\}", text)}
    assert len(arrays) == 30
    inv = pow(1 << 261, -1, P.Q)
    for k in (1, 2, 3):
        for i in range(1, 6):
            want = P.f2_pow(P.XI, i * (P.Q**k - 1) // 6)
            got = tuple(sum(l << (29 * j) for j, l in enumerate(arrays[f"GAMMA_{k}_{i}_C{c}"])) * inv % P.Q for c in (0, 1))
            assert all(l < 1 << 29 for c in (0, 1) for l in arrays[f"GAMMA_{k}_{i}_C{c}"])
            assert got == want, (k, i)
    assert P.f2_pow(P.XI, (P.Q**2 - 1) // 2) == (P.Q - 1, 0)                    # GAMMA_2_3 = -1: -pi^2(Q) keeps y
    assert int(re.search(r"ATE_LOW = 0x([0-9a-f]+)ull", text).group(1), 16) == P.ATE - (1 << 64)
    assert int(re.search(r"uint64_t X = 0x([0-9a-f]+)ull", text).group(1), 16) == P.X_BN
    # the committed file is what the generator writes
    import runpy

    gen = runpy.run_path(os.path.join(ROOT, "tools", "gen_pairing_constants.py"))
    for k in (1, 2, 3):
        for i in range(1, 6):
            g = gen["gamma"](k, i)
            assert gen["arr"](f"GAMMA_{k}_{i}_C0", g[0]) in text and gen["arr"](f"GAMMA_{k}_{i}_C1", g[1]) in text


# ---- pairing.hpp on the host, under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pairing") / "pairing_host_check"
    build = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "pairing_host_check.cpp"), "-o", str(exe)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert build.returncode == 0, build.stdout

    def run(requests):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([str(exe)], input="".join(r + "\n" for r in requests), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             timeout=900, env=env)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.split()
        assert len(lines) == len(requests)
        return lines

    return run


def test_tower_operations_equal_the_reference(driver):
    cases = V.tower_cases()
    got = driver([f"O {op} {a.hex()} {b.hex()}" for _, op, a, b, _ in cases])
    for (name, _, _, _, want), g in zip(cases, got):
        assert P.from_tower(V.dec12(bytes.fromhex(g))) == want, name          # dec12 also checks that every word pattern is canonical


def test_inverse_times_the_element_is_one(driver):
    els = V.elements()[1:]
    inv = driver([f"O {V.OP_INV} {V.enc12(t).hex()} {V.enc12(t).hex()}" for t in els])
    prod = driver([f"O {V.OP_MUL} {V.enc12(t).hex()} {i}" for t, i in zip(els, inv)])
    for p in prod:
        assert P.from_tower(V.dec12(bytes.fromhex(p))) == P.ONE


def test_miller_loop_reduces_to_the_reference_pairing(driver):
    cases = V.miller_cases()
    got = driver([f"O {V.OP_MILLER} {a.hex()} {a.hex()}" for _, a, _ in cases])
    for (name, _, want), g in zip(cases, got):
        assert P.final_exponentiation(P.from_tower(V.dec12(bytes.fromhex(g)))) == want, name


def test_verdicts_of_the_complete_check(driver):
    cases = V.verdict_cases()
    assert sum(1 for c in cases if not c[4]) >= 5 and sum(1 for c in cases if c[4]) >= 8
    got = driver([f"V {n} {g1.hex() or '-'} {g2.hex() or '-'}" for _, g1, g2, n, _ in cases])
    for (name, _, _, _, want), g in zip(cases, got):
        assert g == ("1" if want else "0"), name
    # hook operation 11 is the same check on two pairs
    two = [c for c in cases if c[3] == 2]
    got = driver([f"O {V.OP_CHECK2} {(g1 + g2).hex()} {(g1 + g2).hex()}" for _, g1, g2, _, _ in two])
    for (name, _, _, _, want), g in zip(two, got):
        assert bytes.fromhex(g) == (b"\x01" if want else b"\x00").ljust(384, b"\0"), name

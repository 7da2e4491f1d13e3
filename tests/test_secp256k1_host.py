"""CPU (`-m "not gpu"`): csrc/secp256k1.hpp, csrc/sha256.hpp and csrc/secp256k1_h2c.hpp -- the arithmetic under the PLUME kernels -- compiled for the
host under ASan + UBSan (tests/cpp/secp256k1_host_check.cpp) and compared, value by value, with Python integers, hashlib and
tests/plume_reference.py: the field at 0, 1, p - 1 and at the unreduced operands p, p + 1, 2^256 - 1 where the header admits them (products and
the fixed exponentiations; sums and differences take canonical operands), inverse and square root with a non-residue, the complete addition and
doubling at P + P, P + (-P), the identity on either side, the joint ladder at its corners, 2 G and n G, SHA-256 at the padding's switches and
through the challenge's register path, the map at u = 0, 1, p - 1 (which hashing cannot reach), and both vectors of RFC 9380 J.8.1."""
import hashlib
import os
import subprocess

import pytest

import plume_cases as PC
import plume_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
P, N, G = R.P, R.N, R.G


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("secp256k1") / "secp256k1_host_check"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    build = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "secp256k1_host_check.cpp"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=600)
    assert build.returncode == 0, build.stdout

    def call(lines):
        done = subprocess.run([str(out)], input="".join(line + "\n" for line in lines), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
        assert done.returncode == 0 and f"secp256k1 host check done: {len(lines)} lines" in done.stdout, done.stdout[-4000:]
        return [[int(x, 16) for x in row.split()] for row in done.stdout.splitlines()[:len(lines)]]

    return call


def _hex(*values):
    return " ".join(f"{v:x}" for v in values)


def _pt(pt):
    return _hex(*pt)


def test_field_products_take_any_256_bit_operand(run):
    rng = PC.rng("field-mul")
    values = [0, 1, 2, P - 1, P, P + 1, PC.FULL, 1 << 255, (1 << 32) + 977, (1 << 224) - 1] + [rng.getrandbits(256) for _ in range(6)]
    cases = [(a, b) for a in values for b in values]
    got = run([f"mul {_hex(a, b)}" for a, b in cases])
    for (a, b), row in zip(cases, got):
        assert row == [a * b % P, a * a % P, 21 * a % P, a % P], (hex(a), hex(b))


def test_field_sums_and_differences_of_canonical_operands(run):
    rng = PC.rng("field-add")
    values = [0, 1, 2, P - 1, P - 2, (P + 1) // 2, (P - 1) // 2, (1 << 32) + 977, 977] + [rng.randrange(P) for _ in range(6)]
    cases = [(a, b) for a in values for b in values]
    got = run([f"add {_hex(a, b)}" for a, b in cases])
    for (a, b), row in zip(cases, got):
        assert row == [(a + b) % P, (a - b) % P, -a % P], (hex(a), hex(b))


def test_inverse_and_square_root_are_the_fixed_exponentiations(run):
    rng = PC.rng("field-inv")
    values = [0, 1, 2, 3, 4, 5, 7, P - 1, P, P + 1, PC.FULL] + [rng.randrange(P) for _ in range(12)]
    assert any(pow(a, (P - 1) // 2, P) == P - 1 for a in values[:8]), "a non-residue is among the small cases"
    got = run([f"inv {a:x}" for a in values])
    for a, (inv, root) in zip(values, got):
        assert inv == pow(a, P - 2, P) and root == pow(a, (P + 1) // 4, P), hex(a)
        assert inv * a % P == (1 if a % P else 0)
        assert root * root % P == (a % P if pow(a, (P - 1) // 2, P) in (0, 1) else -a % P)


def test_the_group_law_is_complete(run):
    A, B = PC.points(2, "law")
    ident = (0, 0)
    cases = [(A, A), (A, R.neg(A)), (A, ident), (ident, A), (ident, ident), (A, B), (B, A), (G, G), (G, R.neg(G)), (R.mul(N - 1, G), G), (R.mul(N - 2, G), R.mul(2, G))]
    got = run([f"padd {_pt(a)} {_pt(b)}" for a, b in cases])
    for (a, b), row in zip(cases, got):
        assert tuple(row[:2]) == R.add(a, b) and tuple(row[2:4]) == R.add(a, a) and row[4] == (1 if a != ident else 0), (a, b)
    assert got[7][0] == 0xC6047F9441ED7D6D3045406E95C07CD85C778E4B8CEF3CA7ABAC09B95C709EE5
    # what on_curve refuses
    bad = run([f"padd {_pt(pt)} {_pt(G)}" for pt in PC.off_curve_points()])
    assert all(row[4] == 0 for row in bad)


def test_the_joint_ladder_at_its_corners(run):
    rng = PC.rng("ladder")
    pts = PC.points(4, "ladder-points")
    cases = PC.lincomb_edges() + [(rng.getrandbits(256), pts[i % 4], rng.getrandbits(256), pts[(i + 1) % 4]) for i in range(6)]
    cases += [(3, (0, 0), 5, pts[0]), (3, pts[0], 5, (0, 0)), (3, (0, 0), 5, (0, 0))]          # the identity as an operand: internal use only
    got = run([f"lin {a:x} {_pt(p)} {b:x} {_pt(q)}" for a, p, b, q in cases])
    for (a, p, b, q), row in zip(cases, got):
        assert tuple(row) == R.lincomb(a, p, b, q), (hex(a), hex(b))
    by_case = {(a, p, b, q): tuple(row) for (a, p, b, q), row in zip(cases, got)}
    assert by_case[(2, G, 0, G)][0] == 0xC6047F9441ED7D6D3045406E95C07CD85C778E4B8CEF3CA7ABAC09B95C709EE5
    assert by_case[(N, G, 0, G)] == (0, 0), "n G is the identity"
    assert sum(1 for row in got if tuple(row) == (0, 0)) >= 6, "the cancelling cases give (0, 0)"


def test_sha256_at_the_padding_switches(run):
    rng = PC.rng("sha")
    data = [bytes(rng.getrandbits(8) for _ in range(n)) for n in (0, 55, 56, 64, 119, 120, 198, 1, 63, 65, 127, 128)]
    got = run([f"sha {d.hex() or '-'}" for d in data])
    for d, (digest,) in zip(data, got):
        assert digest == int.from_bytes(hashlib.sha256(d).digest(), "big"), len(d)


def test_the_challenge_hashes_198_bytes_from_registers(run):
    pts = list(PC.points(10, "challenge"))
    groups = [pts[0:5], pts[5:10], [(0, 0)] * 5, [pts[0], (0, 0), pts[1], (0, 0), pts[2]], [R.neg(p) for p in pts[0:5]]]
    got = run(["chal " + " ".join(_pt(p) for p in g) for g in groups])
    for g, (digest,) in zip(groups, got):
        assert digest == R.challenge(*g)
        assert len(b"".join(R.compress_point(p) for p in [G] + g)) == 198


def test_the_map_at_the_inputs_hashing_cannot_reach(run):
    rng = PC.rng("sswu")
    us = [0, 1, P - 1, 2, P - 2] + [rng.randrange(P) for _ in range(10)]
    got = run([f"sswu {u:x}" for u in us])
    for u, row in zip(us, got):
        on_iso = R.map_to_curve_sswu(u)
        assert tuple(row[:2]) == on_iso and tuple(row[2:]) == R.iso_map(on_iso), hex(u)
        assert R.on_curve(tuple(row[2:]))
    assert got[0][0] == R.ISO_B * pow(R.Z * R.ISO_A, -1, P) % P, "u = 0 is the exceptional case: x1 = B' / (Z A')"


def test_the_published_vectors_of_rfc_9380(run):
    got = run(["h2craw -", "h2craw 616263"])
    assert got[0] == [0xc1cae290e291aee617ebaef1be6d73861479c48b841eaba9b7b5852ddfeb1346, 0x64fa678e07ae116126f08b022a94af6de15985c996c3a91b64c406a960e51067]
    assert got[1] == [0x3377e01eab42db296b512293120c6cee72b6ecf9f9205760bd9ff11fb3cb2c4b, 0x7f95890f33efebd1044d382a01b1bee0900fb6116f94688d487c6c7b9c8371f6]
    rng = PC.rng("h2craw")
    msgs = [bytes(rng.getrandbits(8) for _ in range(n)) for n in (1, 33, 34, 64, 97)]      # 86 + 33, 86 + 34: either side of the padding switch
    assert [tuple(row) for row in run([f"h2craw {m.hex()}" for m in msgs])] == [R.hash_to_curve_bytes(m) for m in msgs]


def test_one_voter_through_the_headers(run):
    """H and the verdict for message lengths either side of every block count, valid, refused and malformed voters"""
    lines, want = [], []
    for n in (0, 2, 33, 34, 64):
        msg = bytes(range(1, n + 1)) if n != 2 else PC.MSG
        pk, nul, s, c = PC.voters(1, msg)[0]
        h = R.hash_to_curve(msg, pk)
        lines.append(f"h2c {msg.hex() or '-'} {_pt(pk)}")
        want.append(list(h))
        for (kk, nn, ss, cc) in [(pk, nul, s, c), (pk, nul, s, (c + 1) % N), (pk, nul, N, c), (pk, (0, 0), s, c), (pk, nul, 0, c), (pk, nul, s, 0)]:
            lines.append(f"verify {msg.hex() or '-'} {_pt(kk)} {_pt(nn)} {ss:x} {cc:x}")
            want.append([R.verdict(msg, nn, kk, ss, cc)] + list(h))
    got = run(lines)
    assert got == want
    assert [row[0] for row in got[1:7]] == [0, 1, 2, 2, 1, 1]

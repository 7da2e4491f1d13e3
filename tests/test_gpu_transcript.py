"""GPU (-m gpu): the `_device` and host-buffer calls of the transcript (include/zkhip.h, "transcript"; csrc/transcript.hip) against big
integers and hashlib (tests/transcript_reference.py): affine x, y and the encoding are recomputed from the Jacobian inputs, the hash is
hashlib's.  Sizes are the ones at which k_transcript_points changes its launch shape; inputs are the edge cases of the conversion.  Then the
multi-open provers and verifiers joined by nothing but proof bytes, and the flow of tools/prove_flow.py with `transcript=True`."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

import zksnap_circuits_halo2_amd as Z
from oracle import bn254 as O
from transcript_reference import RefTranscript, encode_point
from zksnap_circuits_halo2_amd import _lib, fields as F, multiopen as M
from zksnap_circuits_halo2_amd.transcript import Blake2bRead, Blake2bWrite

pytestmark = pytest.mark.gpu
R, Q = O.R_MOD, O.Q_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

# csrc/transcript.hip: up to TR_SINGLE_MAX points every thread inverts its own z; beyond, the chunk of the shared inversion doubles up to TR_CHUNK_MAX
TR_BLOCK, TR_SINGLE_MAX, TR_CHUNK_MAX = 64, 1024, 8
CHUNK_SWITCHES = [TR_SINGLE_MAX * ch for ch in (1, 2, 4)]                             # the last size of chunk 1, 2, 4
LARGEST = TR_SINGLE_MAX * TR_CHUNK_MAX + TR_BLOCK * TR_CHUNK_MAX + 3                  # more than 16 workgroups, a part-filled last chunk
NON_RESIDUE = next(z for z in range(2, 50) if pow(z, (Q - 1) // 2, Q) == Q - 1)


def limbs(v):
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def jacobian(points, zs):
    """(x z^2, y z^3, z) in Montgomery limbs; a point None is an identity as a Jacobian sum may leave it: z = 0 under non-zero X and Y"""
    out = np.zeros((len(points), 12), dtype=np.uint64)
    for i, (P, z) in enumerate(zip(points, zs)):
        if P is None:
            out[i, 0:4], out[i, 4:8] = limbs((z * z + 7) % Q * F.MONT % Q), limbs((z + 11) % Q * F.MONT % Q)      # X, Y arbitrary and non-zero, Z = 0
            continue
        out[i, 0:4] = limbs(P[0] * z * z % Q * F.MONT % Q)
        out[i, 4:8] = limbs(P[1] * z * z * z % Q * F.MONT % Q)
        out[i, 8:12] = limbs(z * F.MONT % Q)
    return out


def to_device(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda")


@pytest.fixture(scope="module")
def walk():
    """LARGEST points: edge cases first, then a walk; computed once, read only"""
    G = O.G1_GEN
    pts = [G, O.neg(G), O.scalar_mul(2, G), O.neg(O.scalar_mul(2, G)), O.scalar_mul(R - 2, G)]      # (1, 2): top limbs zero; (1, q - 2): y next to the modulus
    acc, step = O.scalar_mul(0xC0FFEE, G), O.scalar_mul(0x5EED5, G)
    while len(pts) < LARGEST:
        pts.append(acc)
        acc = O.add(acc, step)
    assert {P[1] & 1 for P in pts[:64]} == {0, 1}                                                   # both signs of y
    return pts


def z_values(n, seed):
    """z = 1, a non-residue times a square, q - 1, small, and random, in turn"""
    rng = random.Random(seed)
    kinds = [lambda: 1, lambda: NON_RESIDUE * pow(rng.randrange(1, Q), 2, Q) % Q, lambda: Q - 1, lambda: 2, lambda: rng.randrange(1, Q)]
    return [kinds[i % len(kinds)]() for i in range(n)]


def reference(points, layout, before=(5,)):
    ref = RefTranscript(layout)
    for s in before:
        ref.common_scalar(s)
    for P in points:
        ref.write_point(P)
    return ref


def test_launch_shape_constants(lib):
    for ch, n in zip((1, 2, 4), CHUNK_SWITCHES):
        assert lib.zkhip_test_transcript_chunk(n) == ch and lib.zkhip_test_transcript_chunk(n + 1) == 2 * ch
    assert lib.zkhip_test_transcript_chunk(LARGEST) == TR_CHUNK_MAX


@pytest.mark.parametrize("n,layout", [(1, 0), (1, 1), (5, 0), (5, 1), (TR_BLOCK + 1, 1)]
                         + [(s + d, (i + d) % 2) for i, s in enumerate(CHUNK_SWITCHES) for d in (0, 1)] + [(LARGEST, 0)])
def test_write_points_device_vs_big_integers(lib, walk, n, layout):
    pts = walk[:n]
    d_pts = to_device(jacobian(pts, z_values(n, n)))
    ref = reference(pts, layout)
    with Blake2bWrite(layout) as t:
        t.common_scalar(5)
        t.write_points(d_pts)
        assert t.finalize() == ref.proof
        assert t.squeeze_challenge() == ref.squeeze()


def test_write_points_all_z_equal_one_and_all_non_residue(lib, walk):
    pts = walk[:200]
    for zs in ([1] * 200, [NON_RESIDUE * pow(i + 3, 2, Q) % Q for i in range(200)]):
        ref = reference(pts, 0)
        with Blake2bWrite(0) as t:
            t.common_scalar(5)
            t.write_points(to_device(jacobian(pts, zs)))
            assert t.finalize() == ref.proof and t.squeeze_challenge() == ref.squeeze()


@pytest.mark.parametrize("where", ["first", "last", "alone", "last_of_a_chunk"])
def test_identity_inputs_are_refused_and_leave_the_transcript_untouched(lib, walk, where):
    n = {"alone": 1, "last_of_a_chunk": 2 * TR_SINGLE_MAX}.get(where, 70)
    pts = list(walk[:n])
    pts[0 if where in ("first", "alone") else n - 1] = None
    bad = to_device(jacobian(pts, z_values(n, 9)))
    good = to_device(jacobian(walk[:n], z_values(n, 9)))
    with Blake2bWrite(0) as t, Blake2bWrite(0) as twin:
        t.common_scalar(11)
        twin.common_scalar(11)
        assert lib.zkhip_transcript_write_points_device(t._t, bad.data_ptr(), n, None) == EINVAL
        assert b"infinity" in lib.zkhip_last_error()
        assert (b"point %d of" % (0 if where in ("first", "alone") else n - 1)) in lib.zkhip_last_error()
        assert t.finalize() == b""
        host = jacobian(pts, z_values(n, 9))
        assert lib.zkhip_transcript_write_points(t._t, host.ctypes.data, n) == EINVAL                # the host-buffer form refuses too
        # bit for bit as before: the same good batch afterwards gives the twin's bytes and challenge (the identity count of the failed calls is not carried over)
        t.write_points(good)
        twin.write_points(good)
        assert t.finalize() == twin.finalize() == reference(walk[:n], 0, before=(11,)).proof
        assert t.squeeze_challenge() == twin.squeeze_challenge()


def test_write_scalars_device(lib):
    gen = O.SplitMix64(31337)
    scalars = [0, 1, R - 1, F.MONT % R] + [gen.fr() for _ in range(300)]
    d = to_device(F.fr_encode(scalars))
    ref = RefTranscript()
    for s in scalars:
        ref.write_scalar(s)
    with Blake2bWrite() as t, Blake2bWrite() as host:
        t.write_scalars(d)
        host.write_scalars(scalars)
        assert t.finalize() == host.finalize() == ref.proof
        c = ref.squeeze()
        assert t.squeeze_challenge() == c and host.squeeze_challenge() == c


@pytest.mark.parametrize("layout", [0, 1])
def test_read_points_device_and_host_forms(lib, walk, layout):
    n = 300
    pts = walk[:n]
    ref = reference(pts, layout)
    proof, challenge = ref.proof, ref.squeeze()
    expect = F.g1_encode(pts)
    src = np.frombuffer(proof, dtype=np.uint8)
    dec, bad = np.zeros((n, 8), dtype=np.uint64), C.c_uint64(0)
    _lib.check(lib.zkhip_g1_decompress(src.ctypes.data, n, dec.ctypes.data, layout, C.byref(bad)))
    assert bad.value == n and np.array_equal(dec, expect)
    with Blake2bRead(proof, layout) as r, Blake2bRead(proof, layout) as h:
        r.common_scalar(5)
        h.common_scalar(5)
        got = r.read_points(n)
        assert got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint64), expect)
        assert np.array_equal(h.read_points(n, device=False), expect)
        assert r.squeeze_challenge() == challenge and h.squeeze_challenge() == challenge
    # the host-buffer writer gives the device writer's bytes
    with Blake2bWrite(layout) as w:
        w.common_scalar(5)
        w.write_points(jacobian(pts, z_values(n, 4)))
        assert w.finalize() == proof and w.squeeze_challenge() == challenge


def test_read_points_refuses_bad_encodings_with_their_index(lib, walk):
    pts = walk[:12]
    good = b"".join(encode_point(P, 0) for P in pts)
    x_off = next(x for x in range(2, 100) if pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) != 1)
    flagged = bytearray(encode_point(pts[7], 0))
    flagged[31] |= 0x80
    cases = {"x >= q": Q.to_bytes(32, "little"), "off the curve": x_off.to_bytes(32, "little"),
             "identity": bytes(31) + bytes([0x80]), "identity flag on a point": bytes(flagged)}
    for name, enc in cases.items():
        proof = good[:32 * 7] + enc + good[32 * 8:]
        with Blake2bRead(proof) as r, Blake2bRead(good) as twin:
            out = torch.zeros((12, 8), dtype=torch.int64, device="cuda")
            assert lib.zkhip_transcript_read_points_device(r._t, 12, out.data_ptr(), None) == EINVAL, name
            assert b"encoding 7 of 12" in lib.zkhip_last_error(), name
            host = np.zeros((12, 8), dtype=np.uint64)
            assert lib.zkhip_transcript_read_points(r._t, 12, host.ctypes.data) == EINVAL, name
            assert lib.zkhip_transcript_read_points_device(r._t, 13, out.data_ptr(), None) == EINVAL           # past the end
            # the cursor and the hash did not move: the seven good points in front are still there
            a, b = r.read_points(7), twin.read_points(7)
            assert torch.equal(a, b) and r.squeeze_challenge() == twin.squeeze_challenge(), name
            with pytest.raises(_lib.ZkhipError):
                r.read_points(1)


# ---- multi-open: prover and verifier joined by the proof bytes alone -----------------------------------------------------------------------------
def upload_polys(lib, polys):
    return [to_device(p) for p in polys]


@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_multiopen_through_a_transcript(lib, cref, k, scheme):
    from test_gpu_verify import device_commit, plans

    n = 1 << k
    gen = O.SplitMix64(1900 + k)
    polys = [cref.gen_scalars(8300 + 10 * k + i, n, 0) for i in range(6)]
    d_polys = upload_polys(lib, polys)
    with Z.ParamsKZG.setup(k, 0x1F2E3D4C5B6A7988 + k) as params:
        commit, d_out = device_commit(lib, params)
        prover = M.ProverSHPLONK(k, commit) if scheme == "shplonk" else M.ProverGWC(k, commit)
        verifier = M.VerifierSHPLONK(params) if scheme == "shplonk" else M.VerifierGWC(params)
        try:
            commitments = np.stack([commit(p.data_ptr()) for p in d_polys])
            for name, plan in plans(gen.fr(), F.omega_for(k)).items():
                # the prover: commitments, evaluations, then the multi-open, all into one transcript
                queries = [M.ProverQuery(pt, d_polys[pi].data_ptr()) for pi, pt in plan]
                M.evaluate_queries(queries, k)
                with Blake2bWrite() as w:
                    w.write_points(to_device(commitments))
                    w.write_scalars([q.eval for q in queries])
                    prover.create_proof_transcript(queries, w)
                    proof = w.finalize()
                n_points = 2 if scheme == "shplonk" else len({pt % R for _, pt in plan})
                assert len(proof) == 32 * (6 + len(plan) + n_points), name

                def verdict(data):
                    """everything the verifier uses comes out of `data`"""
                    with Blake2bRead(data) as r:
                        try:
                            cs = r.read_points(6, device=False)
                            evals = r.read_scalars(len(plan))
                        except _lib.ZkhipError:
                            return False
                        vq = [M.VerifierQuery(pt, M._affine_to_xyz(cs[pi]), e) for (pi, pt), e in zip(plan, evals)]
                        return verifier.verify_proof_transcript(vq, r)

                assert verdict(proof) is True, name
                flip = lambda i: proof[:i] + bytes([proof[i] ^ 1]) + proof[i + 1:]
                assert verdict(flip(len(proof) - 32)) is False, name                                  # H' (GWC: the last witness)
                assert verdict(flip(32 * (6 + len(plan) // 2))) is False, name                        # one evaluation
                assert verdict(flip(32 * 2)) is False, name                                           # a commitment
                assert verdict(proof[:-1]) is False, name                                             # a truncated proof
            prover.close()
        finally:
            lib.zkhip_free(d_out)


# ---- the flow: mock -> prove -> verify, joined by proof bytes ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flow():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_flow

    return prove_flow


@pytest.fixture(scope="module")
def proved(flow):
    """run(7, 3, lookups=2, transcript=True, verify=True) once: (result, the arguments the verifier was handed)"""
    seen = []
    real = flow.verify_transcript_proof

    def spy(*args):
        seen.append(args)
        return real(*args)

    flow.verify_transcript_proof = spy
    try:
        res = flow.run(7, 3, lookups=2, verbose=False, transcript=True, verify=True)
    finally:
        flow.verify_transcript_proof = real
    return res, seen


def written(res):
    """points and scalars a proof holds, counted from the plan and the shape"""
    sh = res["proof_shape"]
    points = sh["advice"] + 2 * sh["lookups"] + sh["permutation_sets"] + sh["lookups"] + (1 if sh["random_poly"] else 0) + 3 + 2
    return points, len(res["proof_plan"])


def test_flow_with_a_transcript_verifies_from_bytes_alone(flow, proved):
    res, seen = proved
    assert res["checks"]["proof_verifies"] is True and all(res["checks"].values())
    points, scalars = written(res)
    assert res["proof_bytes"] == len(res["proof"]) == 32 * (points + scalars)
    assert "transcript" in res["timings_ms"] and "verify" in res["timings_ms"]
    # what the verifier was handed: parameters, the verifying key, k, bytes, and plain descriptions of the circuit -- no tensor, no prover object
    (params, vk, k, proof, shape, plan), = seen
    assert type(proof) is bytes and proof == res["proof"] and k == 7
    assert all(type(v) in (int, bool) for v in shape.values())
    assert all(type(kind) is str and type(i) is int and type(r) is int for kind, i, r in plan)
    assert not any(torch.is_tensor(a) for a in (params, vk, k, proof, shape, plan))
    small = flow.run(7, 1, verbose=False, transcript=True, verify=True)
    assert small["checks"]["proof_verifies"] is True and all(small["checks"].values())
    assert small["proof_bytes"] == 32 * sum(written(small))


def test_flow_proof_bytes_depend_on_the_seed_alone(flow, proved):
    res, _ = proved
    again = flow.run(7, 3, lookups=2, verbose=False, transcript=True)
    assert again["proof"] == res["proof"] and "proof_verifies" not in again["checks"]
    other = flow.run(7, 3, lookups=2, verbose=False, transcript=True, seed=2)
    assert other["proof"] != res["proof"] and other["proof_bytes"] == res["proof_bytes"]


@pytest.mark.parametrize("what", ["first advice commitment", "a lookup product commitment", "one evaluation", "H", "H'"])
def test_flow_rejects_a_proof_with_one_flipped_bit(flow, proved, what):
    res, _ = proved
    sh = res["proof_shape"]
    points, scalars = written(res)
    first_eval = points - 2
    at = {"first advice commitment": 0, "a lookup product commitment": sh["advice"] + 2 * sh["lookups"] + sh["permutation_sets"],
          "one evaluation": first_eval + scalars // 2, "H": first_eval + scalars, "H'": first_eval + scalars + 1}[what]
    try:
        bad = flow.run(7, 3, lookups=2, verbose=False, transcript=True, verify=True, corrupt_proof=("byte", 32 * at))
    except _lib.ZkhipError as e:                                                    # the decode error
        assert e.code == EINVAL
        return
    assert bad["checks"]["proof_verifies"] is False, what
    assert all(v for kk, v in bad["checks"].items() if kk != "proof_verifies"), what     # the prover's own checks do not see it
    assert bad["proof"] == res["proof"]                                             # the prover wrote the same bytes: the flip is the verifier's input


def test_flow_without_a_transcript_is_as_it_was(flow):
    plain = flow.run(7, 1, verbose=False)
    assert set(plain) == {"timings_ms", "prove_ms", "checks", "columns", "proof_columns", "msms", "queries", "program_insns", "program_registers",
                          "h_commitments", "keygen_ms", "pk_file_bytes", "vanishing_random_commitment"}
    assert set(plain["checks"]) == {"permutation_product_closes", "lookup_product_closes", "quotient_is_a_polynomial",
                                    "commit_lagrange_equals_commit_coeff", "multiopen_linearisation_vanishes"}
    assert all(plain["checks"].values()) and "transcript" not in plain["timings_ms"]
    with pytest.raises(ValueError):
        flow.run(7, 1, verbose=False, corrupt_proof=("byte", 0))                    # needs transcript and verify
    with pytest.raises(ValueError):
        flow.run(7, 1, verbose=False, transcript=True, verify=True, corrupt_proof="eval")

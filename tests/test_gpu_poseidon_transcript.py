"""GPU (-m gpu): the `_device` calls of a POSEIDON transcript (include/zkhip.h, "transcript" and "Poseidon").  They launch the kernels of the
Blake2b transcript and move the same records; what the host does with a record differs.  So: the proof bytes equal a Blake2b writer's for the
same input, the challenges are those of the restated transcript (tests/poseidon_reference.py), a reader walks what a writer wrote, and a
flipped byte rejects.  Then the flow of tools/prove_flow.py under `gen_snark`'s pair -- the Poseidon transcript with the GWC multi-open --
and the Blake2b + SHPLONK flow's bytes, which routing by hash must leave as they were."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import poseidon_reference as PR
from oracle import bn254 as O
from test_gpu_transcript import jacobian, to_device, z_values
from zksnap_circuits_halo2_amd import _lib, fields as F
from zksnap_circuits_halo2_amd.transcript import Blake2bWrite, PoseidonRead, PoseidonWrite

pytestmark = pytest.mark.gpu
R, Q = O.R_MOD, O.Q_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SIZES = [1, 64, 1025]                 # one point; a whole workgroup of k_transcript_points; the first size whose points share inversions in pairs
# sha256 of the proof of run(7, 3, lookups=2, transcript=True) (seed 1) on the commit before the Poseidon transcript existed
BLAKE2B_SHPLONK_PROOF_SHA256 = "534e4cc6303399005a0e87c9d5870dc9f95473bea207a452a12fd34680d77aff"


@pytest.fixture(scope="module")
def walk():
    """1025 points: the generator and its negative, the largest multiple, then a walk; computed once, read only.  (No curve point at hand has a
    coordinate in [r, q): that interval is 2^-127 of the field.  The reduction mod r is shown on the host, tests/test_poseidon_host.py.)"""
    G = O.G1_GEN
    pts = [G, O.neg(G), O.scalar_mul(R - 2, G)]
    acc, step = O.scalar_mul(0xFACADE, G), O.scalar_mul(0x51DE, G)
    while len(pts) < max(SIZES):
        pts.append(acc)
        acc = O.add(acc, step)
    return pts


def reference(points, scalars=(), before=(5,)):
    ref = PR.Transcript()
    for s in before:
        ref.common_scalar(s)
    for P in points:
        ref.common_point(*P)
    for s in scalars:
        ref.common_scalar(s)
    return ref


@pytest.mark.parametrize("n", SIZES)
def test_write_points_device(lib, walk, n):
    pts = walk[:n]
    d_pts = to_device(jacobian(pts, z_values(n, n)))
    ref = reference(pts)
    with PoseidonWrite() as t, Blake2bWrite() as b:
        t.common_scalar(5)
        b.common_scalar(5)
        t.write_points(d_pts)
        b.write_points(d_pts)
        assert t.finalize() == b.finalize() and len(t.finalize()) == 32 * n         # the bytes do not depend on the hash
        assert t.squeeze_challenge() == ref.squeeze()
        assert t.squeeze_challenge() == ref.squeeze()                               # the state carries on


@pytest.mark.parametrize("n", SIZES)
def test_write_scalars_device(lib, n):
    gen = O.SplitMix64(600 + n)
    scalars = ([0, 1, R - 1, F.MONT % R] + [gen.fr() for _ in range(n)])[:n]
    d = to_device(F.fr_encode(scalars))
    ref = reference((), scalars)
    with PoseidonWrite() as t, PoseidonWrite() as host, Blake2bWrite() as b:
        for w in (t, host, b):
            w.common_scalar(5)
        t.write_scalars(d)
        host.write_scalars(scalars)
        b.write_scalars(d)
        assert t.finalize() == host.finalize() == b.finalize() == b"".join(s.to_bytes(32, "little") for s in scalars)
        c = ref.squeeze()
        assert t.squeeze_challenge() == c and host.squeeze_challenge() == c


def test_identity_inputs_are_refused_and_leave_the_transcript_untouched(lib, walk):
    n = 70
    pts = list(walk[:n])
    pts[n - 1] = None
    bad = to_device(jacobian(pts, z_values(n, 9)))
    good = to_device(jacobian(walk[:n], z_values(n, 9)))
    with PoseidonWrite() as t:
        t.common_scalar(5)
        assert lib.zkhip_transcript_write_points_device(t._t, bad.data_ptr(), n, None) == EINVAL
        assert b"infinity" in lib.zkhip_last_error() and t.finalize() == b""
        t.write_points(good)
        assert t.squeeze_challenge() == reference(walk[:n]).squeeze()


def test_writer_to_reader_round_trip_and_a_flipped_byte(lib, walk):
    n = 65
    pts = walk[:n]
    gen = O.SplitMix64(99)
    scalars = [gen.fr() for _ in range(7)]
    with PoseidonWrite() as w:
        w.common_scalar(5)
        w.write_points(to_device(jacobian(pts, z_values(n, 3))))
        c0 = w.squeeze_challenge()
        w.write_scalars(to_device(F.fr_encode(scalars)))
        c1 = w.squeeze_challenge()
        w.write_points(jacobian(pts[:2], [1, 2]))                                   # the host-buffer form
        c2 = w.squeeze_challenge()
        proof = w.finalize()
    ref = reference(pts)
    assert c0 == ref.squeeze()
    assert len(proof) == 32 * (n + 7 + 2)
    expect = F.g1_encode(pts)
    with PoseidonRead(proof) as r, PoseidonRead(proof) as h:
        r.common_scalar(5)
        h.common_scalar(5)
        got = r.read_points(n)
        assert got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint64), expect)
        assert np.array_equal(h.read_points(n, device=False), expect)
        assert r.squeeze_challenge() == c0 and h.squeeze_challenge() == c0
        assert r.read_scalars(7) == scalars and r.squeeze_challenge() == c1
        assert np.array_equal(r.read_points(2, device=False), expect[:2]) and r.squeeze_challenge() == c2
    # one flipped bit: in a point's x (another point or no point at all), in a scalar (another challenge)
    flip = lambda i: proof[:i] + bytes([proof[i] ^ 1]) + proof[i + 1:]
    with PoseidonRead(flip(32 * 3)) as r:
        r.common_scalar(5)
        try:
            r.read_points(n)
            assert r.squeeze_challenge() != c0
        except _lib.ZkhipError as e:
            assert e.code == EINVAL
    with PoseidonRead(flip(32 * n + 5)) as r:
        r.common_scalar(5)
        r.read_points(n)
        assert r.squeeze_challenge() == c0
        assert r.read_scalars(7) != scalars and r.squeeze_challenge() != c1
    with PoseidonRead(proof[:32 * n - 1]) as r:
        out = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        assert lib.zkhip_transcript_read_points_device(r._t, n, out.data_ptr(), None) == EINVAL      # a truncated proof


# ---- the flow under gen_snark's pair ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flow():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_flow

    return prove_flow


@pytest.fixture(scope="module")
def snark(flow):
    return flow.run(k=8, transcript="poseidon", multiopen="gwc", verify=True, verbose=False)


def test_flow_poseidon_gwc_verifies(flow, snark):
    assert snark["checks"]["proof_verifies"] is True and all(snark["checks"].values())
    sh = snark["proof_shape"]
    points = sh["advice"] + 2 * sh["lookups"] + sh["permutation_sets"] + sh["lookups"] + 3
    witnesses = snark["proof_bytes"] // 32 - points - len(snark["proof_plan"])
    assert snark["proof_bytes"] == len(snark["proof"]) and snark["proof_bytes"] % 32 == 0
    assert witnesses == len({r for _, _, r in snark["proof_plan"]})                 # GWC: one witness per distinct point, x omega^rotation
    assert "multiopen_gwc" in snark["timings_ms"] and "multiopen_shplonk" not in snark["timings_ms"]
    # the same circuit and seed under Blake2b: the same layout, other challenges, so other evaluations and witnesses
    blake = flow.run(k=8, transcript=True, multiopen="gwc", verify=True, verbose=False)
    assert blake["checks"]["proof_verifies"] is True and blake["proof_bytes"] == snark["proof_bytes"]
    assert blake["proof"][:32 * sh["advice"]] == snark["proof"][:32 * sh["advice"]] and blake["proof"] != snark["proof"]


@pytest.mark.parametrize("what", ["first advice commitment", "one evaluation", "last witness"])
def test_flow_poseidon_gwc_rejects_a_flipped_byte(flow, snark, what):
    sh = snark["proof_shape"]
    points = sh["advice"] + 2 * sh["lookups"] + sh["permutation_sets"] + sh["lookups"] + 3
    at = {"first advice commitment": 0, "one evaluation": 32 * (points + len(snark["proof_plan"]) // 2), "last witness": snark["proof_bytes"] - 32}[what]
    try:
        bad = flow.run(k=8, transcript="poseidon", multiopen="gwc", verify=True, verbose=False, corrupt_proof=("byte", at))
    except _lib.ZkhipError as e:                                                    # the decode error
        assert e.code == EINVAL
        return
    assert bad["checks"]["proof_verifies"] is False, what
    assert all(v for kk, v in bad["checks"].items() if kk != "proof_verifies"), what
    assert bad["proof"] == snark["proof"]                                           # the flip is the verifier's input


def test_flow_blake2b_shplonk_bytes_are_as_they_were(flow):
    res = flow.run(7, 3, lookups=2, verbose=False, transcript=True)
    assert hashlib.sha256(res["proof"]).hexdigest() == BLAKE2B_SHPLONK_PROOF_SHA256
    named = flow.run(7, 3, lookups=2, verbose=False, transcript="blake2b", multiopen="shplonk")
    assert named["proof"] == res["proof"]


def test_flow_refuses_unknown_names(flow):
    with pytest.raises(ValueError):
        flow.run(7, 1, verbose=False, transcript="keccak")
    with pytest.raises(ValueError):
        flow.run(7, 1, verbose=False, transcript=True, multiopen="ipa")
    with pytest.raises(ValueError):
        flow.run(7, 1, verbose=False, multiopen="gwc")                              # the seeded flow opens with SHPLONK

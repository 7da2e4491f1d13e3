"""GPU (-m gpu): the verifiers that end in `zkhip_pairing_check` -- `ParamsKZG.verify_opening`, `VerifierGWC` / `VerifierSHPLONK` on what the
provers of the same file emit, `ParamsKZG.verify` on a parameter set and on four ways of spoiling one, and the flow mock -> prove -> verify of
tools/prove_flow.py.  Acceptance alone shows little: every case is followed by inputs that differ in one place and must be rejected."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import zksnap_circuits_halo2_amd as Z
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, arithmetic as A, fields as F, multiopen as M, srs

pytestmark = pytest.mark.gpu
R = O.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes(range(100, 132))


class DevicePolys:
    """polynomials uploaded once, freed at the end"""

    def __init__(self, lib, polys):
        self.lib, self.ptrs = lib, []
        for p in polys:
            ptr = C.c_void_p()
            _lib.check(lib.zkhip_alloc(p.shape[0] * 32, C.byref(ptr)))
            _lib.check(lib.zkhip_upload(ptr, p.ctypes.data, p.shape[0] * 32))
            self.ptrs.append(ptr)

    def __enter__(self):
        return [p.value for p in self.ptrs]

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.zkhip_free(p)


def device_commit(lib, params):
    d_out = C.c_void_p()
    _lib.check(lib.zkhip_alloc(96, C.byref(d_out)))

    def commit(d_coeffs):
        params.commit_device(d_coeffs, params.n, d_out.value)
        out = np.zeros(12, dtype=np.uint64)
        _lib.check(lib.zkhip_sync())
        _lib.check(lib.zkhip_download(out.ctypes.data, d_out, 96))
        return out

    return commit, d_out


def another_point(point_xyz):
    """a different curve point: the given one plus the generator"""
    out = np.zeros(12, dtype=np.uint64)
    pts = np.stack([point_xyz, M._affine_to_xyz(F.g1_encode([O.G1_GEN])[0])])
    _lib.check(_lib.load().zkhip_g1_sum(pts.ctypes.data, 2, out.ctypes.data))
    return out


# ---- KZG, one point ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 6])
def test_verify_opening_accepts_the_quotient_commitment_and_rejects_changes(lib, cref, k):
    n = 1 << k
    with Z.ParamsKZG.setup(k, 0x3A4B5C6D7E8F9012 + k) as params:
        poly = cref.gen_scalars(7100 + k, n, 0)
        z = O.SplitMix64(71 + k).fr()
        value = F.fr_decode(A.eval_polynomial(poly, F.fr_encode([z])[0]).reshape(1, 4))[0]
        shifted = poly.copy()
        shifted[0] = F.fr_encode([(F.fr_decode(poly[:1])[0] - value) % R])[0]
        quotient = A.kate_division(shifted, F.fr_encode([z])[0])                  # zkhip_fr_kate_division
        commitment, witness = params.commit(poly), params.commit(quotient)
        assert params.verify_opening(commitment, z, value, witness)
        assert not params.verify_opening(commitment, z, (value + 1) % R, witness)
        assert not params.verify_opening(commitment, (z + 1) % R, value, witness)
        assert not params.verify_opening(commitment, z, value, another_point(witness))
        assert not params.verify_opening(another_point(commitment), z, value, witness)


# ---- multi-open -------------------------------------------------------------------------------------------------------------------------------
def plans(x, w):
    px, pn, pp = x, x * w % R, x * pow(w, -1, R) % R
    return {
        "one set": [(0, px), (1, px), (2, px)],
        "several sets": [(0, px), (1, px), (1, pn), (2, px), (2, pn), (2, pp), (3, px), (4, pp), (4, px), (4, pn)],
        "three points": [(0, px), (0, pn), (0, pp)],
        "mixed order": [(0, px), (1, px), (2, pn), (0, pn), (3, px), (4, pp), (5, px), (1, pp)],
        "repeated query": [(0, px), (1, px), (1, pn), (2, pn), (1, px)],
    }


@pytest.mark.parametrize("k", [5, 8])
def test_multiopen_verifiers_accept_the_provers_and_reject_changes(lib, cref, k):
    n = 1 << k
    gen = O.SplitMix64(900 + k)
    polys = [cref.gen_scalars(7300 + 10 * k + i, n, 0) for i in range(6)]
    with Z.ParamsKZG.setup(k, 0x0F1E2D3C4B5A6978 + k) as params, DevicePolys(lib, polys) as d_polys:
        commit, d_out = device_commit(lib, params)
        try:
            commitments = [commit(p) for p in d_polys]
            gwc, shp = M.ProverGWC(k, commit), M.ProverSHPLONK(k, commit)
            vg, vs = M.VerifierGWC(params), M.VerifierSHPLONK(params)
            for name, plan in plans(gen.fr(), F.omega_for(k)).items():
                y, v, u = gen.fr(), gen.fr(), gen.fr()
                queries = [M.ProverQuery(pt, d_polys[pi]) for pi, pt in plan]
                W = gwc.create_proof(queries, v)
                H, Hp = shp.create_proof(queries, y, v, u)
                vq = lambda: [M.VerifierQuery(q.point, commitments[pi], q.eval) for (pi, _), q in zip(plan, queries)]
                assert vg.verify_proof(vq(), W, v, u), name
                assert vs.verify_proof(vq(), H, Hp, y, v, u), name
                # one changed evaluation
                bad = vq()
                bad[len(bad) // 2].eval = (bad[len(bad) // 2].eval + 1) % R
                assert not vg.verify_proof(bad, W, v, u), name
                assert not vs.verify_proof(bad, H, Hp, y, v, u), name
                # two commitments swapped (the first two queries that name different polynomials)
                bad = vq()
                j = next(t for t in range(1, len(plan)) if plan[t][0] != plan[0][0]) if len({pi for pi, _ in plan}) > 1 else None
                if j is not None:
                    bad[0].commitment, bad[j].commitment = bad[j].commitment, bad[0].commitment
                else:
                    bad[0].commitment = commitments[5]                         # a single polynomial: another one's commitment in its place
                assert not vg.verify_proof(bad, W, v, u), name
                assert not vs.verify_proof(bad, H, Hp, y, v, u), name
                # a changed challenge: u enters the SHPLONK proof itself; GWC's u is the verifier's own, there the prover's v is changed.
                # (With ONE opening point x the SHPLONK proof does not depend on u at all: L(X) = h(X) (X - x) - (u - x) h(X) = h(X) (X - u), so
                # H' = H and the verifier's left point is (f(s) - r) G + x H for every u -- nothing to reject in the plan "one set".)
                if len({pt for _, pt in plan}) > 1:
                    assert not vs.verify_proof(vq(), H, Hp, y, v, (u + 1) % R), name
                else:
                    assert np.array_equal(F.g1_decode_jacobian(H), F.g1_decode_jacobian(Hp))
                if max(len(qs) for _, qs in M.construct_intermediate_sets(queries)) > 1:
                    assert not vg.verify_proof(vq(), W, (v + 1) % R, u), name
                # A repeated query.  The set construction keeps the FIRST evaluation of a (polynomial, point) pair, so the repetition is where
                # a changed claim could hide: SHPLONK's sets do not see one more agreeing repetition (GWC's do: its prover and verifier take
                # every query), and a disagreeing one is refused by both -- on the plan whose LAST query is a repetition, exactly that one.
                rep = vq() + [vq()[len(plan) // 2]]
                assert vs.verify_proof(rep, H, Hp, y, v, u), name
                rep[-1].eval = (rep[-1].eval + 1) % R
                assert not vg.verify_proof(rep, W, v, u) and not vs.verify_proof(rep, H, Hp, y, v, u), name
                if plan[-1] in plan[:-1]:
                    bad = vq()
                    bad[-1].eval = (bad[-1].eval + 1) % R
                    assert not vg.verify_proof(bad, W, v, u) and not vs.verify_proof(bad, H, Hp, y, v, u), name
                # one query of a polynomial that is opened several times names another polynomial's commitment: by bytes and by poly_id
                multi = next((t for t, (pi, _) in enumerate(plan) if sum(1 for pj, _ in plan if pj == pi) > 1), None)
                if multi is not None:
                    for ids in (False, True):
                        bad = [M.VerifierQuery(q.point, commitments[pi], q.eval, poly_id=pi if ids else None) for (pi, _), q in zip(plan, queries)]
                        assert vg.verify_proof(bad, W, v, u) and vs.verify_proof(bad, H, Hp, y, v, u), (name, ids)
                        bad[multi].commitment = commitments[(plan[multi][0] + 1) % 6]
                        assert not vg.verify_proof(bad, W, v, u) and not vs.verify_proof(bad, H, Hp, y, v, u), (name, ids)
                # a changed proof point
                assert not vg.verify_proof(vq(), [another_point(W[0])] + W[1:], v, u), name
                assert not vs.verify_proof(vq(), H, another_point(Hp), y, v, u), name
                assert not vs.verify_proof(vq(), another_point(H), Hp, y, v, u), name
            gwc.close()
            shp.close()
        finally:
            lib.zkhip_free(d_out)


# ---- the parameter set ------------------------------------------------------------------------------------------------------------------------
def twist_point_outside_the_subgroup():
    """A point of the twist E'(Fq2) whose order is not r, found by trial: x = (t, 1) for t = 0, 1, 2, ... until x^3 + b' is a square in Fq2; the
    first point found is taken unless r times it is the identity (the twist has r (2q - r) points, so a point found this way has order r with
    probability about 1 / (2q - r)), in which case the search goes on."""
    t = 0
    while True:
        x = (t, 1)
        y = srs._f2sqrt(O.f2_add(O.f2_mul(O.f2_mul(x, x), x), O.G2_B))
        t += 1
        if y is None:
            continue
        P = (x, y)
        assert O.g2_on_curve(P)
        if O.g2_scalar_mul(R - 1, P) != O.g2_neg(P):
            return P


def test_params_verify_accepts_a_setup_and_rejects_spoiled_tables(lib):
    k, s = 6, 0x1122334455667788
    n = 1 << k
    with Z.ParamsKZG.setup(k, s) as params:
        g, gl, g2, s_g2 = params.g.copy(), params.g_lagrange.copy(), params.g2.copy(), params.s_g2.copy()
        assert params.verify(SEED)
        assert params.verify(bytes(32))                                            # whatever the seed
    def verdict(g_=g, gl_=gl, g2_=g2, s_g2_=s_g2):
        with Z.ParamsKZG(k, g_.copy(), gl_.copy(), g2_.copy(), s_g2_.copy()) as p:
            return p.verify(SEED)
    assert verdict()
    # g[5] replaced by 7 G: a valid curve point, the wrong power
    bad = g.copy()
    bad[5] = F.g1_encode([O.scalar_mul(7, O.G1_GEN)])[0]
    assert not verdict(g_=bad)
    # s_g2 replaced by (s + 1) H
    assert not verdict(s_g2_=srs.g2_encode(srs.g2_mul(s + 1)))
    # two g_lagrange entries swapped
    bad = gl.copy()
    bad[[3, 9]] = bad[[9, 3]]
    assert not verdict(gl_=bad)
    # a g2 on the twist but outside the subgroup of order r
    P = twist_point_outside_the_subgroup()
    assert srs.g2_is_on_curve(P)
    assert not verdict(g2_=srs.g2_encode(P))
    # an identity where a generator belongs, a point off the curve
    bad = g.copy()
    bad[0] = 0
    assert not verdict(g_=bad)
    bad = g.copy()
    bad[7, 0] ^= np.uint64(1)
    assert not verdict(g_=bad)


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------------------------
def test_cpp_verifier_mirror(lib, tmp_path):
    """include/zkhip.hpp: pairing_check, verify_opening, VerifierGWC, VerifierSHPLONK on proofs of the mirror's own provers (tests/cpp/verify_driver.cpp)"""
    import subprocess

    drv = os.path.join(ROOT, "tests", "cpp", "verify_driver")
    assert os.path.exists(drv), "tests/cpp/verify_driver is built by __graft_entry__.build()"
    k, s = 6, 0x51A2B3C4D5E6F708
    (tmp_path / "g2.bin").write_bytes(srs.g2_encode(srs.G2_GENERATOR).tobytes() + srs.g2_encode(srs.g2_mul(s)).tobytes())
    out = subprocess.run([drv, str(k), hex(s), str(tmp_path / "g2.bin"), str(tmp_path / "report.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    flags = int.from_bytes((tmp_path / "report.bin").read_bytes(), "little")
    assert flags == 0x7FF, bin(flags)


# ---- the flow ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flow():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_flow

    return prove_flow


def test_flow_verifies_its_proof_and_only_that_check_sees_a_corrupted_proof(flow):
    plain = flow.run(7, 1, verbose=False)
    assert "proof_verifies" not in plain["checks"] and "verify" not in plain["timings_ms"] and all(plain["checks"].values())
    res = flow.run(7, 1, verbose=False, verify=True)
    assert res["checks"]["proof_verifies"] is True and all(res["checks"].values())
    assert set(res) == set(plain) and set(res["checks"]) == set(plain["checks"]) | {"proof_verifies"}
    assert "verify" in res["timings_ms"]
    others = sum(v for kk, v in res["timings_ms"].items() if kk not in ("setup_srs", "witness_columns", "mock_prover", "stack_columns", "verify") and not kk.startswith("keygen_"))
    assert abs(res["prove_ms"] - others) < 1e-6                                    # the verify lap is not part of prove_ms
    # two gate columns: their selector columns are equal, and so are the commitments of two different polynomials of the plan (poly_id)
    two = flow.run(7, 2, verbose=False, verify=True)
    assert two["checks"]["proof_verifies"] is True and all(two["checks"].values())
    for what in ("eval", "commitment", "witness"):
        bad = flow.run(7, 1, verbose=False, verify=True, corrupt_proof=what)
        assert bad["checks"]["proof_verifies"] is False, what
        assert all(v for kk, v in bad["checks"].items() if kk != "proof_verifies"), what
    with pytest.raises(ValueError):
        flow.run(7, 1, verbose=False, verify=True, corrupt_proof="nothing")

"""GPU (-m gpu): the SHPLONK provers divide by a rotation set's vanishing polynomial with ONE `zkhip_fr_divide_by_roots_device` per set -- and
produce the bytes they produced when they folded `kate_division`s.

For a query list whose rotation sets have 1, 2, 3 and 4 points (k = 10), H and H' from the Python prover, from the C++ mirror
(tests/cpp/multiopen_driver) and from `zkhip_multiopen_shplonk_{begin, finish}_device` equal the values of a restatement, local to this
file, of the construction the provers used BEFORE: linear combination with Python integers, the low-degree interpolant subtracted
coefficient by coefficient, the oracle's `kate_division` once per point, the oracle's MSM.  That pins "no change of bytes" to the oracle,
not to the code under test.

The profiler (`zkhip_profile_enable`) records marks inside the transforms, the MSMs and the sharded quotient only: neither
`kate_division` nor the one-element row programs ever recorded one, so it cannot count them and no such test is made here."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import zksnap_circuits_halo2_amd as Z
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F, multiopen as M

pytestmark = pytest.mark.gpu
R = O.R_MOD


def _interpolate(points, evals):
    m = len(points)
    coeffs = [0] * m
    for i in range(m):
        num, den = [1], 1
        for j in range(m):
            if j != i:
                num = [(a - points[j] * b) % R for a, b in zip([0] + num, num + [0])]
                den = den * (points[i] - points[j]) % R
        scale = evals[i] * pow(den, -1, R) % R
        for t in range(m):
            coeffs[t] = (coeffs[t] + scale * num[t]) % R
    return coeffs


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def _vanishing_at(points, x):
    acc = 1
    for p in points:
        acc = acc * (x - p) % R
    return acc


def _old_construction(cref, ints, sets, n, g, y, v, u):
    """sets: [(points ascending, [polynomial indices])] in order of first appearance -> (H, H') affine, as the fold-of-kate_division provers built them"""
    super_points = sorted({p for pts, _ in sets for p in pts})
    evals = {(pi, z): _horner(ints[pi], z) for pts, idx in sets for pi in idx for z in pts}
    quotients = []
    for pts, idx in sets:
        acc = [0] * n
        low = [0] * len(pts)
        for j, pi in enumerate(idx):
            yp = pow(y, j, R)
            for t, c in enumerate(ints[pi]):
                acc[t] = (acc[t] + yp * c) % R
            for t, c in enumerate(_interpolate(pts, [evals[(pi, z)] for z in pts])):
                low[t] = (low[t] + yp * c) % R
        for t, c in enumerate(low):
            acc[t] = (acc[t] - c) % R
        cur = F.fr_encode(acc)
        for z in pts:                                               # `div_by_vanishing`: one kate_division per point
            cur = cref.kate_division(np.ascontiguousarray(cur), F.fr_encode([z])[0])
        quotients.append(F.fr_decode(cur) + [0] * len(pts))
    h = [0] * n
    for i, q in enumerate(quotients):
        vp = pow(v, i, R)
        for t, c in enumerate(q):
            h[t] = (h[t] + vp * c) % R
    H = cref.jac_to_affine(cref.best_multiexp(F.fr_encode(h), np.ascontiguousarray(g), 2))
    z_diffs = [_vanishing_at([p for p in super_points if p not in pts], u) for pts, _ in sets]
    zt, norm = _vanishing_at(super_points, u), pow(z_diffs[0], -1, R)
    L, const = [0] * n, 0
    for i, (pts, idx) in enumerate(sets):
        for j, pi in enumerate(idx):
            c = pow(v, i, R) * z_diffs[i] % R * pow(y, j, R) % R * norm % R
            for t, a in enumerate(ints[pi]):
                L[t] = (L[t] + c * a) % R
            const = (const + c * _horner(_interpolate(pts, [evals[(pi, z)] for z in pts]), u)) % R
    c = (-zt * norm) % R
    for t, a in enumerate(h):
        L[t] = (L[t] + c * a) % R
    L[0] = (L[0] - const) % R
    assert _horner(L, u) == 0
    final = cref.kate_division(F.fr_encode(L), F.fr_encode([u])[0])
    Hp = cref.jac_to_affine(cref.best_multiexp(np.ascontiguousarray(final), np.ascontiguousarray(g[: n - 1]), 2))
    return H, Hp


def test_shplonk_commitments_equal_the_fold_construction(lib, cref, tmp_path):
    k, s, blinding = 10, 0x6B8B4567327B23C6, 5
    n = 1 << k
    polys = [cref.gen_scalars(8100 + i, n, i % 2) for i in range(7)]
    ints = [F.fr_decode(p) for p in polys]
    gen = O.SplitMix64(81)
    x = gen.fr()
    w = F.omega_for(k)
    px, pn, pp, pb = x, x * w % R, x * pow(w, -1, R) % R, x * pow(w, -(blinding + 1), R) % R
    # polynomial -> its points: sets of 1, 2, 3 and 4 points; the sets of 1 and 3 points hold two polynomials each
    plan = [(0, px), (1, px), (1, pn), (2, pp), (2, px), (2, pn), (3, px), (3, pn), (3, pp), (3, pb), (4, px), (5, pn), (5, pp), (5, px)]
    sets = [(sorted([px]), [0, 4]), (sorted([px, pn]), [1]), (sorted([px, pn, pp]), [2, 5]), (sorted([px, pn, pp, pb]), [3])]
    y, v, u = gen.fr(), gen.fr(), gen.fr()
    with Z.ParamsKZG.setup(k, s) as params:
        g = params.g.copy()
    exp_H, exp_Hp = _old_construction(cref, ints, sets, n, g, y, v, u)

    d_polys = []
    for p in polys:
        ptr = C.c_void_p()
        _lib.check(lib.zkhip_alloc(n * 32, C.byref(ptr)))
        _lib.check(lib.zkhip_upload(ptr, p.ctypes.data, n * 32))
        d_polys.append(ptr)
    _lib.check(lib.zkhip_register_bases(g.ctypes.data, n))
    d_out = C.c_void_p()
    _lib.check(lib.zkhip_alloc(96, C.byref(d_out)))

    def commit(d_coeffs):
        _lib.check(lib.zkhip_msm_g1_registered_device(g.ctypes.data, C.c_void_p(d_coeffs), n, d_out, None))
        out = np.zeros(12, dtype=np.uint64)
        _lib.check(lib.zkhip_download(out.ctypes.data, d_out, 96))
        return out

    aff = lambda a: cref.jac_to_affine(np.ascontiguousarray(a))
    try:
        # 1. the Python prover
        queries = [M.ProverQuery(pt, d_polys[pi].value) for pi, pt in plan]
        got_sets, _ = M.construct_rotation_sets(queries)
        ptr_to_idx = {d.value: i for i, d in enumerate(d_polys)}
        assert [(rs.points, [ptr_to_idx[p] for p in rs.polys]) for rs in got_sets] == sets
        assert sorted(len(rs.points) for rs in got_sets) == [1, 2, 3, 4]
        sh = M.ProverSHPLONK(k, commit)
        H, Hp = sh.create_proof(queries, y, v, u)
        sh.close()
        assert np.array_equal(aff(H), exp_H), "Python prover: H"
        assert np.array_equal(aff(Hp), exp_Hp), "Python prover: H'"
        # 2. the C entry points (the C++ mirror behind `extern "C"`)
        qs = (_lib.ProverQueryC * len(plan))()
        for i, (pi, pt) in enumerate(plan):
            qs[i].point[:] = [int(t) for t in F.fr_encode([pt])[0]]
            qs[i].d_poly = d_polys[pi].value
        yw, vw, uw = (F.fr_encode([t])[0] for t in (y, v, u))
        h_out, hp_out = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        st = C.c_void_p()
        _lib.check(lib.zkhip_multiopen_shplonk_begin_device(g.ctypes.data, k, qs, len(plan), yw.ctypes.data, vw.ctypes.data, h_out.ctypes.data, C.byref(st)))
        _lib.check(lib.zkhip_multiopen_shplonk_finish_device(st, uw.ctypes.data, hp_out.ctypes.data))
        assert np.array_equal(aff(h_out), exp_H), "C entry points: H"
        assert np.array_equal(aff(hp_out), exp_Hp), "C entry points: H'"
    finally:
        _lib.check(lib.zkhip_unregister_bases(g.ctypes.data))
        for ptr in d_polys + [d_out]:
            lib.zkhip_free(ptr)
    # 3. the C++ mirror compiled into a host program (its own process)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    drv = os.path.join(root, "tests", "cpp", "multiopen_driver")
    assert os.path.exists(drv), "build it with __graft_entry__.build()"
    fin, report = tmp_path / "in.bin", tmp_path / "report.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<IIIQ", k, len(polys), len(plan), s))
        for p in polys:
            f.write(p.tobytes())
        for pi, pt in plan:
            f.write(struct.pack("<I", pi))
            f.write(F.fr_encode([pt]).tobytes())
        f.write(F.fr_encode([y, v, u]).tobytes())
    subprocess.check_call([drv, str(fin), str(report)], timeout=300)
    rep = report.read_bytes()
    count, = struct.unpack("<I", rep[:4])
    pts = np.frombuffer(rep[4:4 + 64 * (count + 2)], dtype=np.uint64).reshape(count + 2, 8)
    assert np.array_equal(pts[count], exp_H), "C++ mirror: H"
    assert np.array_equal(pts[count + 1], exp_Hp), "C++ mirror: H'"


def test_python_prover_issues_one_division_per_rotation_set(lib, cref, monkeypatch):
    """`ProverSHPLONK.create_proof` over s rotation sets: s + 1 calls of `zkhip_fr_divide_by_roots_device` (the sets, then L(X) / (X - u)), no
    `zkhip_fr_kate_division_device`, and one one-element row program (the constant term of L) where there were 1 + sum |S| + s + 1"""
    k = 10
    n = 1 << k
    polys = [cref.gen_scalars(8200 + i, n, 0) for i in range(4)]
    gen = O.SplitMix64(82)
    x = gen.fr()
    w = F.omega_for(k)
    px, pn, pp = x, x * w % R, x * pow(w, -1, R) % R
    plan = [(0, px), (1, px), (1, pn), (2, px), (2, pn), (2, pp), (3, px)]
    with Z.ParamsKZG.setup(k, 0x1234ABCD) as params:
        g = params.g.copy()
    d_polys = []
    for p in polys:
        ptr = C.c_void_p()
        _lib.check(lib.zkhip_alloc(n * 32, C.byref(ptr)))
        _lib.check(lib.zkhip_upload(ptr, p.ctypes.data, n * 32))
        d_polys.append(ptr)
    _lib.check(lib.zkhip_register_bases(g.ctypes.data, n))
    d_out = C.c_void_p()
    _lib.check(lib.zkhip_alloc(96, C.byref(d_out)))

    def commit(d_coeffs):
        _lib.check(lib.zkhip_msm_g1_registered_device(g.ctypes.data, C.c_void_p(d_coeffs), n, d_out, None))
        out = np.zeros(12, dtype=np.uint64)
        _lib.check(lib.zkhip_download(out.ctypes.data, d_out, 96))
        return out

    calls = {"roots": [], "kate": 0, "one_row": 0}
    real_roots, real_kate, real_sub, real_zero = lib.zkhip_fr_divide_by_roots_device, lib.zkhip_fr_kate_division_device, M._sub_const_at, M._zero_at

    def roots_spy(d_a, size, roots, m, d_q, d_evals, stream):
        calls["roots"].append(m)
        return real_roots(d_a, size, roots, m, d_q, d_evals, stream)

    def kate_spy(*a):
        calls["kate"] += 1
        return real_kate(*a)

    def one_row_spy(real):
        def f(*a, **kw):
            calls["one_row"] += 1
            return real(*a, **kw)
        return f

    monkeypatch.setattr(lib, "zkhip_fr_divide_by_roots_device", roots_spy)
    monkeypatch.setattr(lib, "zkhip_fr_kate_division_device", kate_spy)
    monkeypatch.setattr(M, "_sub_const_at", one_row_spy(real_sub))
    monkeypatch.setattr(M, "_zero_at", one_row_spy(real_zero))
    try:
        sh = M.ProverSHPLONK(k, commit)
        sh.create_proof([M.ProverQuery(pt, d_polys[pi].value) for pi, pt in plan], gen.fr(), gen.fr(), gen.fr())
        sh.close()
    finally:
        monkeypatch.undo()
        _lib.check(lib.zkhip_unregister_bases(g.ctypes.data))
        for ptr in d_polys + [d_out]:
            lib.zkhip_free(ptr)
    assert calls["roots"] == [1, 2, 3, 1], calls        # the sets {x}, {x, wx}, {x, wx, w^-1 x} in order of first appearance, then (X - u)
    assert calls["kate"] == 0 and calls["one_row"] == 1, calls

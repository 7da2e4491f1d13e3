"""The KZG multi-open arguments of the reference: `ProverGWC::create_proof` (the `gen_snark` path) and, below,
`ProverSHPLONK::create_proof` (the bench path).

Mirror of [DEP] halo2-axiom `poly/kzg/multiopen/gwc.rs` + `gwc/prover.rs` as the reference reaches it:
`gen_snark::<.., ProverGWC<_>, ..>` (/root/reference/aggregator/src/wrapper.rs:59-60, 127-137; accumulation scheme `KzgAs<Bn256, Gwc19>`,
wrapper.rs:55).  For every distinct opening point z, in the order the points first appear among the queries:

    poly_batch = sum_i v^i p_i            eval_batch = sum_i v^i e_i             (the queries at z, in query order)
    W_z        = commit( kate_division(poly_batch - eval_batch, z) )

Everything runs on device-resident polynomials: the combination is one fused row program (`linear_combination_program`), the
quotient is `zkhip_fr_kate_division_device`, the commitment the prepared MSM.  The transcript is the host's business: the challenge v is
an argument and the witness commitments are returned (the reference writes each to the transcript as it is produced).
The bench path of the reference uses SHPLONK instead (halo2-base `gen_proof`): `ProverSHPLONK` in the second half of this file.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib, evaluation as E
from .buffers import DeviceBuffer
from .fields import R_MOD, fr_decode, fr_encode
from .transcript import _is_device, decoded


@dataclass
class ProverQuery:
    """`ProverQuery { point, poly, eval }`: `poly` is the device address of 2^k coefficients (32 bytes each); `eval` may be None, in
    which case `evaluate_queries` fills it in (the prover computes these evaluations anyway and writes them to the transcript)"""
    point: int
    poly: int
    eval: int = None


def construct_intermediate_sets(queries: Sequence[ProverQuery]) -> List[Tuple[int, List[ProverQuery]]]:
    """`construct_intermediate_sets` of gwc.rs: queries grouped by point, points in order of first appearance, queries in query order"""
    sets: List[Tuple[int, List[ProverQuery]]] = []
    for q in queries:
        for point, qs in sets:
            if point == q.point % R_MOD:
                qs.append(q)
                break
        else:
            sets.append((q.point % R_MOD, [q]))
    return sets


def evaluate_queries(queries: Sequence[ProverQuery], k: int, stream: int = 0) -> None:
    """fills `eval` of every query that lacks it: one batched evaluation per distinct point (`eval_polynomial` on the device)"""
    lib = _lib.load()
    n = 1 << k
    for point, qs in construct_intermediate_sets([q for q in queries if q.eval is None]):
        with DeviceBuffer(len(qs) * 32) as out:
            ptrs = (C.c_void_p * len(qs))(*[q.poly for q in qs])
            x = fr_encode([point])[0]
            _lib.check(lib.zkhip_fr_eval_polynomial_batch_device(ptrs, len(qs), n, x.ctypes.data, out.ptr, stream))
            _lib.check(lib.zkhip_stream_sync(stream))        # zkhip_download copies on the legacy default stream: not ordered behind a non-blocking `stream`
            host = out.download((len(qs), 4))
        for q, e in zip(qs, fr_decode(host)):
            q.eval = e


def _sub_const_at(d_poly: int, index: int, value: int, stream: int = 0) -> None:
    """d_poly[index] -= value, enqueued on the stream (a one-row program: no host round trip)"""
    prog = E.RowProgram()
    prog.emit(E.OP_SUB, 0, prog.column(0), prog.constant(value))
    prog.run_device([d_poly + index * 32], 0, d_poly + index * 32, stream=stream)


def _zero_at(d_poly: int, index: int, stream: int = 0) -> None:
    prog = E.RowProgram()
    prog.emit(E.OP_MOV, 0, prog.constant(0))
    prog.run_device([], 0, d_poly + index * 32, stream=stream)


class _BufferPool:
    """n-coefficient device buffers kept between proofs (a prover object lives as long as its proving key)"""

    def __init__(self, n: int):
        self.n, self.free, self.all = n, [], []

    def take(self) -> int:
        if self.free:
            return self.free.pop()
        self.all.append(DeviceBuffer(self.n * 32))
        return self.all[-1].address

    def give_back(self, taken: List[int]) -> None:
        self.free.extend(taken)

    def close(self) -> None:
        for b in self.all:
            b.free()
        self.all, self.free = [], []


class ProverGWC:
    """`ProverGWC::new(params)` / `create_proof(transcript, queries)`; `commit` is a callable taking the device address of 2^k
    coefficients and returning the commitment (12 uint64 limbs, Jacobian) -- e.g. a prepared-table MSM over `params.g`.  `create_proof`
    enqueues on `stream` (any HIP stream, blocking or not) and drains it before every host read and before every call of `commit`."""

    def __init__(self, k: int, commit):
        self.k, self.n, self.commit = k, 1 << k, commit
        self.pool = _BufferPool(self.n)

    def close(self) -> None:
        self.pool.close()

    def create_proof(self, queries: Sequence[ProverQuery], v: int, stream: int = 0) -> List[np.ndarray]:
        lib = _lib.load()
        n = self.n
        evaluate_queries(queries, self.k, stream)
        batch, quot = self.pool.take(), self.pool.take()
        witnesses = []
        try:
            for z, qs in construct_intermediate_sets(queries):
                powers = [pow(v, i, R_MOD) for i in range(len(qs))]
                eval_batch = sum(p * q.eval for p, q in zip(powers, qs)) % R_MOD
                # poly_batch - eval_batch: the combination over all n rows, then the constant term alone (a one-row program on the same buffer)
                E.linear_combination_program(powers).run_device([q.poly for q in qs], self.k, batch, stream=stream)
                _sub_const_at(batch, 0, eval_batch, stream)
                zw = fr_encode([z])[0]
                _lib.check(lib.zkhip_fr_kate_division_device(C.c_void_p(batch), n, zw.ctypes.data, C.c_void_p(quot), stream))
                _zero_at(quot, n - 1, stream)           # the quotient has n - 1 coefficients; the commitment takes n scalars
                _lib.check(lib.zkhip_stream_sync(stream))     # `commit` runs on a stream of its own choosing: hand it finished coefficients
                witnesses.append(np.array(self.commit(quot), dtype=np.uint64).reshape(12))
        finally:
            _lib.check(lib.zkhip_sync())
            self.pool.give_back([batch, quot])
        return witnesses

    def create_proof_transcript(self, queries: Sequence[ProverQuery], tr, stream: int = 0) -> List[np.ndarray]:
        """`create_proof(transcript, queries)` with the transcript (transcript.Blake2bWrite): v is squeezed, every witness commitment written"""
        v = tr.squeeze_challenge()
        witnesses = self.create_proof(queries, v, stream)
        if witnesses:
            tr.write_points(np.stack(witnesses))
        return witnesses


# ---------------------------------------------------------------------------------------------------------------------------------
# SHPLONK: `ProverSHPLONK::create_proof` [DEP poly/kzg/multiopen/shplonk.rs + shplonk/prover.rs] -- the multi-open of the reference's
# bench path (halo2-base `gen_proof`: /root/reference/aggregator/benches/wrapper_circuit.rs:140, state_transition_circuit.rs:84,
# /root/reference/voter/benches/voter_circuit.rs:80).  Restated from the published algorithm (unpinned, as everything at this boundary):
#
#   rotation sets      polynomials grouped by the SET of points they are opened at (sets in order of first appearance of their first
#                      polynomial, polynomials in order of first appearance, the points of a set ascending as canonical integers: a BTreeSet)
#   R_ij               the interpolation of P_ij's evaluations over its set's points ("low degree equivalent")
#   h(X)  = sum_i v^i ( sum_j y^j (P_ij - R_ij) ) / Z_i(X),   Z_i = prod over the set's points (X - z)                    -> commit: H
#   L(X)  = sum_i v^i Z_{T \ S_i}(u) sum_j y^j (P_ij(X) - R_ij(u))  -  Z_T(u) h(X),     T = all points;   L(u) = 0
#   h'(X) = L(X) / (X - u) / Z_{T \ S_0}(u)                                                                              -> commit: H'
#
# Device work: the y- and v-combinations are fused row programs over the device-resident polynomials, the divisions one
# `zkhip_fr_divide_by_roots_device` per rotation set, the two commitments prepared MSMs; the interpolations are host arithmetic on a handful of points.
# ---------------------------------------------------------------------------------------------------------------------------------
def _interpolate(points: Sequence[int], evals: Sequence[int]) -> List[int]:
    """`lagrange_interpolate`: coefficients (low to high) of the polynomial of degree < len(points) through (points[i], evals[i])"""
    m = len(points)
    coeffs = [0] * m
    for i in range(m):
        num = [1]
        den = 1
        for j in range(m):
            if j == i:
                continue
            num = [(a - points[j] * b) % R_MOD for a, b in zip([0] + num, num + [0])]      # num * (X - points[j])
            den = den * (points[i] - points[j]) % R_MOD
        scale = evals[i] * pow(den, -1, R_MOD) % R_MOD
        for t in range(m):
            coeffs[t] = (coeffs[t] + scale * num[t]) % R_MOD
    return coeffs


def _eval_small(coeffs: Sequence[int], x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R_MOD
    return acc


def _vanishing_at(points: Sequence[int], x: int) -> int:
    acc = 1
    for p in points:
        acc = acc * (x - p) % R_MOD
    return acc


@dataclass
class RotationSet:
    points: List[int]                      # ascending canonical integers
    polys: List[int]                       # device addresses, in order of first appearance
    evals: List[List[int]]                 # evals[j][t] = P_j(points[t])


def construct_rotation_sets(queries: Sequence[ProverQuery]) -> Tuple[List[RotationSet], List[int]]:
    """`construct_intermediate_sets` of shplonk.rs -> (rotation sets, super point set ascending)"""
    by_poly: dict = {}                                  # poly -> its points, in order of first appearance (dicts keep insertion order)
    evals: dict = {}
    for q in queries:
        by_poly.setdefault(q.poly, set()).add(q.point % R_MOD)
        evals.setdefault((q.poly, q.point % R_MOD), q.eval)          # the first query of a (poly, point) pair gives the evaluation
    sets_by_key: dict = {}                              # point set -> its polynomials, in order of first appearance
    for poly, pts in by_poly.items():
        sets_by_key.setdefault(frozenset(pts), []).append(poly)
    sets = list(sets_by_key.items())

    def get_eval(poly, point):
        return evals[(poly, point)]

    out = []
    for key, polys in sets:
        pts = sorted(key)
        out.append(RotationSet(pts, polys, [[get_eval(p, z) for z in pts] for p in polys]))
    return out, sorted({q.point % R_MOD for q in queries})


class ProverSHPLONK:
    def __init__(self, k: int, commit):
        self.k, self.n, self.commit = k, 1 << k, commit
        self.pool = _BufferPool(self.n)

    def close(self) -> None:
        self.pool.close()

    def _patch_low(self, d_poly: int, low: Sequence[int], stream: int = 0) -> None:
        """d_poly[t] -= low[t] for the first len(low) coefficients (the low degree equivalent has as many coefficients as the set has points)"""
        for t, val in enumerate(low):
            if val % R_MOD:
                _sub_const_at(d_poly, t, val, stream)

    def _divide(self, d_poly: int, d_tmp: int, roots: Sequence[int], stream: int) -> int:
        """`div_by_vanishing`: one `zkhip_fr_divide_by_roots_device` for the whole point set, the quotient kept at n coefficients (the top
        len(roots) zero); returns the buffer that holds it.  More points than ZKHIP_MAX_ROOTS (no rotation set of halo2): the fold."""
        lib = _lib.load()
        if len(roots) > _lib.ZKHIP_MAX_ROOTS:
            src, dst = d_poly, d_tmp
            for z in roots:
                zw = fr_encode([z])[0]
                _lib.check(lib.zkhip_fr_kate_division_device(C.c_void_p(src), self.n, zw.ctypes.data, C.c_void_p(dst), stream))
                _zero_at(dst, self.n - 1, stream)
                src, dst = dst, src
            return src
        zw = fr_encode(list(roots))
        _lib.check(lib.zkhip_fr_divide_by_roots_device(C.c_void_p(d_poly), self.n, zw.ctypes.data, len(roots), C.c_void_p(d_tmp), None, stream))
        return d_tmp

    def create_proof_transcript(self, queries: Sequence[ProverQuery], tr, stream: int = 0):
        """`create_proof(transcript, queries)` with the transcript (transcript.Blake2bWrite), in the reference's order: squeeze y, squeeze v,
        commit and write H, squeeze u, write H'.  -> (H, H')"""
        y = tr.squeeze_challenge()
        v = tr.squeeze_challenge()

        def u_after(H):
            tr.write_points(H.reshape(1, 12))
            return tr.squeeze_challenge()

        H, Hp = self._create_proof(queries, y, v, u_after, stream)
        tr.write_points(Hp.reshape(1, 12))
        return H, Hp

    def create_proof(self, queries: Sequence[ProverQuery], y: int, v: int, u: int, stream: int = 0):
        """-> (H, H') as 12-limb Jacobian commitments.  In the reference y and v are squeezed before h is committed and u after h has been
        written to the transcript; here all three are arguments."""
        return self._create_proof(queries, y, v, lambda H: u, stream)

    def _create_proof(self, queries: Sequence[ProverQuery], y: int, v: int, u_of_H, stream: int = 0):
        """the prover with u asked for once H exists (`u_of_H(H) -> u`): the one place where the transcript reaches into the argument"""
        lib = _lib.load()
        n = self.n
        evaluate_queries(queries, self.k, stream)
        sets, super_points = construct_rotation_sets(queries)
        bufs = []

        def alloc():
            bufs.append(self.pool.take())
            return bufs[-1]

        try:
            # ---- h(X): per set the y-combination of P - R, divided by the set's vanishing polynomial; then the v-combination -------------
            quotients = []
            for rs in sets:
                ypow = [pow(y, j, R_MOD) for j in range(len(rs.polys))]
                acc, tmp = alloc(), alloc()
                E.linear_combination_program(ypow).run_device(rs.polys, self.k, acc, stream=stream)
                # the quotient by Z_i is the same polynomial whether or not sum_j y^j R_ij (degree < the number of points) is subtracted first
                quotients.append(self._divide(acc, tmp, rs.points, stream))
            vpow = [pow(v, i, R_MOD) for i in range(len(sets))]
            h_x = alloc()
            E.linear_combination_program(vpow).run_device(quotients, self.k, h_x, stream=stream)
            _lib.check(lib.zkhip_stream_sync(stream))         # `commit` runs on a stream of its own choosing: hand it finished coefficients
            H = np.array(self.commit(h_x), dtype=np.uint64).reshape(12)
            u = u_of_H(H)
            # ---- L(X) and the final quotient ----------------------------------------------------------------------------------------------
            z_diffs = [_vanishing_at([p for p in super_points if p not in rs.points], u) for rs in sets]
            zt_eval = _vanishing_at(super_points, u)
            norm = pow(z_diffs[0], -1, R_MOD)                                                  # "normalize by the coefficient of the first polynomial"
            cols, coeffs, const = [], [], 0
            for i, rs in enumerate(sets):
                for j, poly in enumerate(rs.polys):
                    c = vpow[i] * z_diffs[i] % R_MOD * pow(y, j, R_MOD) % R_MOD * norm % R_MOD
                    cols.append(poly)
                    coeffs.append(c)
                    r_eval = _eval_small(_interpolate(rs.points, rs.evals[j]), u)               # R_ij(u)
                    const = (const + c * r_eval) % R_MOD
            cols.append(h_x)
            coeffs.append((-zt_eval * norm) % R_MOD)
            l_x, tmp = alloc(), alloc()
            E.linear_combination_program(coeffs).run_device(cols, self.k, l_x, stream=stream)
            self._patch_low(l_x, [const], stream)
            # the reference's debug assertion: L(u) = 0 (the result lands in the top coefficient slot of the scratch buffer, which the
            # division below overwrites)
            uw = fr_encode([u])[0]
            chk = tmp + (n - 1) * 32
            _lib.check(lib.zkhip_fr_eval_polynomial_device(C.c_void_p(l_x), n, uw.ctypes.data, C.c_void_p(chk), stream))
            res = np.zeros(4, dtype=np.uint64)
            _lib.check(lib.zkhip_stream_sync(stream))
            _lib.check(lib.zkhip_download(res.ctypes.data, C.c_void_p(chk), 32))
            if res.any():
                raise ArithmeticError("SHPLONK: L(u) != 0 -- inconsistent queries (an evaluation does not match its polynomial)")
            final = self._divide(l_x, tmp, [u], stream)
            _lib.check(lib.zkhip_stream_sync(stream))
            Hp = np.array(self.commit(final), dtype=np.uint64).reshape(12)
            return H, Hp
        finally:
            _lib.check(lib.zkhip_sync())
            self.pool.give_back(bufs)


# ---------------------------------------------------------------------------------------------------------------------------------
# The verifiers: `VerifierGWC::verify_proof` / `VerifierSHPLONK::verify_proof` [DEP poly/kzg/multiopen/{gwc,shplonk}/verifier.rs], the third
# step of the reference's `gen_proof` (`assert!(verify_proof(..))`, /root/reference/aggregator/src/wrapper.rs:140-155).  They accept exactly
# what the provers above emit and use the same set construction, keyed by commitment instead of device address (see VerifierQuery.poly_id for
# polynomials whose commitments are equal).  The scalars are Python integers, the G1 side is one small MSM through zkhip_msm_g1 per
# accumulated point, and the end is one zkhip_pairing_check of two pairs: e(L, g2) e(-R, [s]_2) = 1.  The transcript is the host's business.
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class VerifierQuery:
    """`VerifierQuery { point, commitment, eval }`: `commitment` is a 12-limb Jacobian point (what `commit` returns).  The set construction
    groups queries by polynomial; a verifier knows a polynomial by its commitment's bytes.  Two DIFFERENT polynomials of a proof may have EQUAL
    commitments (two selector columns with the same rows): halo2 tells them apart by the address of the commitment (`CommitmentReference`
    compares pointers), here `poly_id` -- any hashable value, one per polynomial -- does, and must then be given for every query
    (`check_queries` refuses a mixture)."""
    point: int
    commitment: np.ndarray
    eval: int
    poly_id: object = None

    @property
    def poly(self):                   # the key the set construction groups by
        if self.poly_id is not None:
            return self.poly_id
        return np.ascontiguousarray(self.commitment, dtype=np.uint64).reshape(12).tobytes()


class InconsistentQueries(ValueError):
    """the queries contradict each other: a verifier rejects"""


def check_queries(queries: Sequence[VerifierQuery]) -> None:
    """What the set construction would otherwise hide.  It was written for the prover, whose repeated queries agree by construction: it keeps the
    FIRST evaluation of a (polynomial, point) pair and one commitment per key.  A verifier's queries are claims: two different evaluations of one
    polynomial at one point, or two different commitments under one `poly_id`, raise InconsistentQueries (the verifiers answer False), so that a
    changed claim cannot hide behind a repeated query.  `poly_id` on some queries and not on others is a ValueError: the keys would not be comparable."""
    with_id = sum(q.poly_id is not None for q in queries)
    if with_id not in (0, len(queries)):
        raise ValueError("VerifierQuery.poly_id: give it for every query or for none")
    commitment_of, eval_at = {}, {}
    for q in queries:
        key = q.poly
        c = np.ascontiguousarray(q.commitment, dtype=np.uint64).reshape(12).tobytes()
        if commitment_of.setdefault(key, c) != c:
            raise InconsistentQueries("two commitments for one polynomial")
        if eval_at.setdefault((key, q.point % R_MOD), q.eval % R_MOD) != q.eval % R_MOD:
            raise InconsistentQueries("two evaluations of one polynomial at one point")


def commitment_points(queries, keys) -> List[np.ndarray]:
    """the commitments (12 limbs each) of the polynomial keys that an accumulation returned"""
    by_key = {q.poly: np.ascontiguousarray(q.commitment, dtype=np.uint64).reshape(12) for q in queries}
    return [by_key[k] for k in keys]


def _affine_to_xyz(point: np.ndarray) -> np.ndarray:
    """G1Affine (8 limbs, not the identity) -> Jacobian (12 limbs) with z = 1"""
    out = np.zeros(12, dtype=np.uint64)
    out[:8] = np.asarray(point, dtype=np.uint64).reshape(8)
    out[8:] = _FQ_ONE
    return out


def _points_xyz(points) -> List[np.ndarray]:
    """points read from a transcript, each 8 affine limbs on the host or an (8,) device tensor, as Jacobian points with z = 1 on the host (a
    transcript holds no identity)"""
    return [_affine_to_xyz(p.cpu().numpy().view(np.uint64) if _is_device(p) else p) for p in points]


def _generator_xyz(params) -> np.ndarray:
    """g[0] as a Jacobian point"""
    return _affine_to_xyz(params.g[0])


_FQ_ONE = np.array([0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f], dtype=np.uint64)      # 2^256 mod q: 1 in Fq's Montgomery form


def gwc_accumulate(queries: Sequence[VerifierQuery], n_witnesses: int, v: int, u: int):
    """-> (scalars of the left point over the witnesses, scalars of the right point over [witnesses | commitments | G], the commitments in order):
    left = sum_i u^i W_i, right = sum_i u^i (z_i W_i + sum_j v^j C_ij - (sum_j v^j e_ij) G)"""
    check_queries(queries)
    sets = construct_intermediate_sets(queries)
    if len(sets) != n_witnesses:
        raise ValueError("GWC: one witness per distinct point")
    left, right_w, commitments, right_c, g_scalar = [], [], [], [], 0
    for i, (z, qs) in enumerate(sets):
        ui = pow(u, i, R_MOD)
        left.append(ui)
        right_w.append(ui * z % R_MOD)
        for j, q in enumerate(qs):
            vj = pow(v, j, R_MOD)
            commitments.append(q.poly)
            right_c.append(ui * vj % R_MOD)
            g_scalar = (g_scalar - ui * vj % R_MOD * q.eval) % R_MOD
    return left, right_w + right_c + [g_scalar], commitments


def shplonk_accumulate(queries: Sequence[VerifierQuery], y: int, v: int, u: int):
    """-> (scalars over [commitments | G | H | H'], the commitments in order) of the left point Lc + u H' with
    Lc = sum_ij c_ij (C_ij - R_ij(u) G) - Z_T(u) / Z_{T \\ S_0}(u) H, c_ij = v^i Z_{T \\ S_i}(u) y^j / Z_{T \\ S_0}(u) (the comment block above
    ProverSHPLONK); the right point is H'"""
    check_queries(queries)
    sets, super_points = construct_rotation_sets(queries)
    z_diffs = [_vanishing_at([p for p in super_points if p not in rs.points], u) for rs in sets]
    norm = pow(z_diffs[0], -1, R_MOD)
    commitments, coeffs, g_scalar = [], [], 0
    for i, rs in enumerate(sets):
        for j, key in enumerate(rs.polys):
            c = pow(v, i, R_MOD) * z_diffs[i] % R_MOD * pow(y, j, R_MOD) % R_MOD * norm % R_MOD
            commitments.append(key)
            coeffs.append(c)
            g_scalar = (g_scalar - c * _eval_small(_interpolate(rs.points, rs.evals[j]), u)) % R_MOD
    h_scalar = (-_vanishing_at(super_points, u) * norm) % R_MOD
    return coeffs + [g_scalar, h_scalar, u % R_MOD], commitments


_Q_MOD = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47


def negate_affine(point: np.ndarray) -> np.ndarray:
    """-(x, y) = (x, q - y) on the 8 affine limbs (Montgomery words: the negation is the same subtraction); the identity (0, 0) stays"""
    out = np.array(point, dtype=np.uint64).reshape(8)
    y = sum(int(w) << (64 * i) for i, w in enumerate(out[4:]))
    if y:
        out[4:] = [((_Q_MOD - y) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return out


def _final_check(params, left_affine: np.ndarray, right_affine_negated: np.ndarray) -> bool:
    from .arithmetic import pairing_check

    if params.g2 is None or params.s_g2 is None:
        raise ValueError("the verifier needs g2 and s_g2")
    return pairing_check(np.stack([left_affine, right_affine_negated]), np.stack([params.g2, params.s_g2]))


class VerifierGWC:
    """`VerifierGWC::new(params)` / `verify_proof`: e(sum_i u^i W_i, [s]_2) = e(sum_i u^i (z_i W_i + sum_j v^j C_ij - (sum_j v^j e_ij) G), g2).
    `witnesses`: what `ProverGWC.create_proof` returned; v the prover's challenge, u the verifier's own."""

    def __init__(self, params):
        self.params = params

    def accumulator_points(self, queries: Sequence[VerifierQuery], witnesses: Sequence[np.ndarray], v: int, u: int):
        """the two points the pairing would check, (lhs, rhs) with e(lhs, g2) = e(rhs, [s]g2) for an honest proof, each 8 affine limbs:
        lhs = sum_i u^i (z_i W_i + sum_j v^j C_ij - (sum_j v^j e_ij) G), rhs = sum_i u^i W_i.  None: inconsistent queries"""
        from .arithmetic import g1_combination

        try:
            left, right, commitments = gwc_accumulate(queries, len(witnesses), v, u)
        except InconsistentQueries:
            return None
        W = [np.ascontiguousarray(w, dtype=np.uint64).reshape(12) for w in witnesses]
        lhs = g1_combination(right, np.stack(W + commitment_points(queries, commitments) + [_generator_xyz(self.params)]))
        return lhs, g1_combination(left, np.stack(W))

    def verify_proof(self, queries: Sequence[VerifierQuery], witnesses: Sequence[np.ndarray], v: int, u: int) -> bool:
        points = self.accumulator_points(queries, witnesses, v, u)
        return points is not None and _final_check(self.params, points[0], negate_affine(points[1]))

    def accumulator_points_read(self, queries: Sequence[VerifierQuery], W, challenges):
        """`accumulator_points` over what `read_proof` returned"""
        return self.accumulator_points(queries, _points_xyz(W), *challenges)

    def read_proof(self, tr, n_points: int, device: bool = False):
        """GWC's part of a proof from a transcript reader, in the order ProverGWC.create_proof_transcript wrote it: v is squeezed, one witness per
        distinct point read (`n_points` of them), then u squeezed -> (the witnesses W_0 .., each 8 affine limbs on the host or, device=True,
        in HBM: the first columns of an A row; (v, u): what follows x in a `points` record).  ZkhipError(-1): the witnesses do not decode;
        v has been squeezed by then, u has not."""
        v = tr.squeeze_challenge()
        W = tr.read_points(n_points, device=device)
        return list(W), (v, tr.squeeze_challenge())

    def verify_proof_read(self, queries: Sequence[VerifierQuery], W, challenges) -> bool:
        """`verify_proof` over what `read_proof` returned, the points on the host or on the device"""
        return self.verify_proof(queries, _points_xyz(W), *challenges)

    def verify_proof_transcript(self, queries: Sequence[VerifierQuery], tr) -> bool:
        """`verify_proof(transcript, queries, ..)` with the transcript (transcript.Blake2bRead): `read_proof` with host points, then
        `verify_proof`.  Proof bytes that do not decode reject."""
        part = decoded(self.read_proof, tr, len(construct_intermediate_sets(queries)))
        return part is not None and self.verify_proof_read(queries, *part)

    # the batch verifier's plan and rows: the module's functions, looked up when called (tests substitute them)
    @staticmethod
    def fold_plan(plan_triples):
        return gwc_plan(plan_triples)

    @staticmethod
    def fold_scalars(plan, evals, points, k: int):
        """-> (rows_a, rows_c, None): GWC has a row for every proof, so no status"""
        return (*gwc_scalars_device(plan, evals, points, k), None)


class VerifierSHPLONK:
    """`VerifierSHPLONK::new(params)` / `verify_proof`: e(Lc + u H', g2) e(-H', [s]_2) = 1.  H, Hp: what `ProverSHPLONK.create_proof` returned."""

    def __init__(self, params):
        self.params = params

    def accumulator_points(self, queries: Sequence[VerifierQuery], H: np.ndarray, Hp: np.ndarray, y: int, v: int, u: int):
        """the two points the pairing would check, (lhs, rhs) = (Lc + u H', H') with e(lhs, g2) = e(rhs, [s]g2) for an honest proof, each 8
        affine limbs.  None: inconsistent queries"""
        from .arithmetic import g1_combination

        try:
            scalars, commitments = shplonk_accumulate(queries, y, v, u)
        except InconsistentQueries:
            return None
        H = np.ascontiguousarray(H, dtype=np.uint64).reshape(12)
        Hp = np.ascontiguousarray(Hp, dtype=np.uint64).reshape(12)
        lhs = g1_combination(scalars, np.stack(commitment_points(queries, commitments) + [_generator_xyz(self.params), H, Hp]))
        if np.array_equal(Hp[8:], _FQ_ONE):                # read from a transcript: affine already (z = 1)
            return lhs, Hp[:8].copy()
        return lhs, g1_combination([1], Hp.reshape(1, 12))  # a prover's Jacobian point

    def verify_proof(self, queries: Sequence[VerifierQuery], H: np.ndarray, Hp: np.ndarray, y: int, v: int, u: int) -> bool:
        points = self.accumulator_points(queries, H, Hp, y, v, u)
        return points is not None and _final_check(self.params, points[0], negate_affine(points[1]))

    def accumulator_points_read(self, queries: Sequence[VerifierQuery], points, challenges):
        """`accumulator_points` over what `read_proof` returned ([H', H])"""
        Hp, H = _points_xyz(points)
        return self.accumulator_points(queries, H, Hp, *challenges)

    def read_proof(self, tr, n_points: int = None, device: bool = False):
        """SHPLONK's part of a proof from a transcript reader, in the order ProverSHPLONK.create_proof_transcript wrote it: squeeze y, squeeze
        v, read H, squeeze u, read H' (whatever `n_points`, the number of distinct points, is) -> ([H', H], each 8 affine limbs on the host
        or, device=True, in HBM: the first columns of an A row; (y, v, u): what follows x in a `points` record).  ZkhipError(-1): H or H' does
        not decode; the squeezes in front of the failing read have happened."""
        y, v = tr.squeeze_challenge(), tr.squeeze_challenge()
        H = tr.read_points(1, device=device)
        u = tr.squeeze_challenge()
        Hp = tr.read_points(1, device=device)
        return [Hp[0], H[0]], (y, v, u)

    def verify_proof_read(self, queries: Sequence[VerifierQuery], points, challenges) -> bool:
        """`verify_proof` over what `read_proof` returned ([H', H]: `verify_proof` takes H first), the points on the host or on the device"""
        Hp, H = _points_xyz(points)
        return self.verify_proof(queries, H, Hp, *challenges)

    def verify_proof_transcript(self, queries: Sequence[VerifierQuery], tr) -> bool:
        """`verify_proof(transcript, queries, ..)` with the transcript (transcript.Blake2bRead): `read_proof` with host points, then
        `verify_proof`.  Proof bytes that do not decode reject."""
        part = decoded(self.read_proof, tr)
        return part is not None and self.verify_proof_read(queries, *part)

    # the batch verifier's plan and rows: the module's functions, looked up when called (tests substitute them)
    @staticmethod
    def fold_plan(plan_triples):
        return shplonk_plan(plan_triples)

    @staticmethod
    def fold_scalars(plan, evals, points, k: int):
        """-> (rows_a, rows_c, status): status 1 is a proof without a row (shplonk_scalars_device)"""
        return shplonk_scalars_device(plan, evals, points, k)


MULTIOPEN = {"shplonk": (ProverSHPLONK, VerifierSHPLONK), "gwc": (ProverGWC, VerifierGWC)}


def multiopen_classes(multiopen):
    """(prover, verifier) of a multi-open's name; ValueError on any other name"""
    if multiopen not in MULTIOPEN:
        raise ValueError(f"multiopen {multiopen!r}: 'shplonk' or 'gwc'")
    return MULTIOPEN[multiopen]


# ---------------------------------------------------------------------------------------------------------------------------------
# The batch verifier: the opening checks of a batch folded into one pairing check (halo2's `BatchVerifier`; the reference's aggregator folds
# its KZG accumulators with random powers the same way, `KzgAs<Bn256, Gwc19>`, /root/reference/aggregator/src/wrapper.rs).  The openings of
# proof i accept exactly when e(A_i, g2) e(-C_i, [s]g2) = 1; with random r_i the batch accepts, except with probability about 1 / r, exactly
# when e(sum r_i A_i, g2) e(-sum r_i C_i, [s]g2) = 1.  A_i and C_i are given as ROWS of scalars over points: the proof's own points (different
# in every proof: their scalars are scaled by r_i) and shared points (the key's commitments and G: their scalars are summed over the proofs).
# BN254 G1 has cofactor 1 and the transcript readers check every point, so nothing here checks a subgroup.
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class FoldPlan:
    """What the fold plans of both multi-opens hold of the opened (kind, index, rotation) triples (prover.opening_plan); query q is triple q of
    the plan.  `rotations`: the distinct rotations as the plan spells them, in order of first appearance -- the verifiers' set constructions
    grouped by rotation, which is what grouping by point gives for every x but 0; `query_rotation`: the index of a query's rotation;
    `query_slot`: the slot of its polynomial, the proof's own polynomials (`own_keys`, in order of first appearance) first and the key's
    (`shared_keys`) behind them.  `repeated`: a (kind, index, rotation) triple occurs twice, which the set constructions would fold into one
    query: such a plan is verified one by one, as is one with two rotations equal mod 2^k (`foldable`)."""
    n_evals: int
    rotations: List[int]
    query_rotation: List[int]
    query_slot: List[int]
    own_keys: List[tuple]
    shared_keys: List[tuple]
    repeated: bool

    @staticmethod
    def fields_of(plan_triples, shared_kinds):
        """-> (the fields above of `plan_triples`, in order; keys, keys[q] = the (kind, index) of query q): polynomials of a kind in
        `shared_kinds` are the key's"""
        triples = [tuple(t) for t in plan_triples]
        rotations = list(dict.fromkeys(rot for _, _, rot in triples))
        keys = [(kind, idx) for kind, idx, _ in triples]
        own = list(dict.fromkeys(key for key in keys if key[0] not in shared_kinds))
        shared = list(dict.fromkeys(key for key in keys if key[0] in shared_kinds))
        slots = {key: s for s, key in enumerate(own + shared)}
        return (len(triples), rotations, [rotations.index(rot) for _, _, rot in triples], [slots[key] for key in keys], own, shared, len(set(triples)) != len(triples)), keys

    @property
    def n_slots(self) -> int:
        return len(self.own_keys) + len(self.shared_keys)

    def foldable(self, k: int) -> bool:
        """may the batch verifier group this plan by rotation at 2^k rows?  Not with a repeated triple, and not with two rotations equal mod 2^k
        (they are one point, their sets one set of points): such plans are verified one by one, which groups by point"""
        return not self.repeated and len({r % (1 << k) for r in self.rotations}) == len(self.rotations)

    def _marshal(self, k: int, struct, counts, lists):
        """-> (struct(*counts, a pointer per list), the uint32 arrays they point into), the rotations reduced mod 2^k in front of `lists`.
        ValueError: two rotations of the plan are equal mod 2^k"""
        rot = [r % (1 << k) for r in self.rotations]
        if len(set(rot)) != len(rot):
            raise ValueError("fold plan: two rotations of the plan are equal mod 2^k")
        arrays = [np.array(a, dtype=np.uint32) for a in [rot] + lists]
        return struct(*counts, *[a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in arrays]), arrays


def _scalars_device(call: str, plan: FoldPlan, evals, points, n_challenges: int, k: int, stream, outs):
    """zkhip_<call> for both multi-opens: the tensor checks, plan.marshal(k), one output per entry of `outs` = (the shape behind B, the torch
    dtype's name) allocated beside `evals`, omega, the call.  -> the outputs.  Asynchronous on `stream`."""
    import torch

    from .fields import omega_for

    B = evals.shape[0]
    if not (evals.is_cuda and evals.is_contiguous() and points.is_cuda and points.is_contiguous()) or tuple(evals.shape) != (B, plan.n_evals, 4) or \
            tuple(points.shape) != (B, 1 + n_challenges, 4):
        raise ValueError(f"{call}: contiguous device tensors, (B, n_evals, 4) and (B, {1 + n_challenges}, 4)")
    struct, keep = plan.marshal(k)
    made = [torch.empty((B,) + shape, dtype=getattr(torch, dtype), device=evals.device) for shape, dtype in outs]
    omega = fr_encode([omega_for(k)])[0]
    _lib.check(getattr(_lib.load(), "zkhip_" + call)(C.byref(struct), evals.data_ptr(), points.data_ptr(), k, omega.ctypes.data, B, *[t_.data_ptr() for t_ in made], stream))
    del keep
    return tuple(made)


@dataclass
class GwcPlan(FoldPlan):
    """An opening plan as the GWC verifier groups it (include/zkhip.h, zkhip_gwc_plan): `construct_intermediate_sets` grouped by rotation, so a
    set is a rotation (`set_rotation`, `query_set`: FoldPlan's `rotations`, `query_rotation`); `query_pos`: a query's position inside its set
    (the exponent of v)."""
    query_pos: List[int]

    set_rotation = property(lambda self: self.rotations)
    query_set = property(lambda self: self.query_rotation)

    @property
    def n_sets(self) -> int:
        return len(self.rotations)

    def marshal(self, k: int):
        """-> (_lib.GwcPlan, the arrays it points into): rotations reduced mod 2^k.  ValueError: two rotations of the plan are equal mod 2^k
        (their sets would be one set)"""
        return self._marshal(k, _lib.GwcPlan, (self.n_evals, self.n_sets, self.n_slots, 0), [self.query_rotation, self.query_pos, self.query_slot])


def gwc_plan(plan_triples, shared_kinds=("fixed", "sigma")) -> GwcPlan:
    """the GwcPlan of the opened (kind, index, rotation) triples (prover.opening_plan); polynomials of a kind in `shared_kinds` are the key's"""
    common, _ = FoldPlan.fields_of(plan_triples, shared_kinds)
    seen, q_pos = [0] * len(common[1]), []               # per rotation, the queries so far
    for s in common[2]:
        q_pos.append(seen[s])
        seen[s] += 1
    return GwcPlan(*common, q_pos)


def gwc_scalars_device(plan: GwcPlan, evals, points, k: int, stream=None):
    """zkhip_gwc_scalars_device: evals (B, n_evals, 4), points (B, 3, 4) = x, v, u, contiguous int64 device tensors -> (rows_a (B, n_sets +
    n_slots + 1, 4), rows_c (B, n_sets, 4)), the column layout of include/zkhip.h.  Asynchronous on `stream`."""
    return _scalars_device("gwc_scalars_device", plan, evals, points, 2, k, stream, [((plan.n_sets + plan.n_slots + 1, 4), "int64"), ((plan.n_sets, 4), "int64")])


@dataclass
class ShplonkPlan(FoldPlan):
    """An opening plan as the SHPLONK verifier groups it (include/zkhip.h, zkhip_shplonk_plan): `construct_rotation_sets` grouped by rotation,
    so the rotations are the super point set (`point_rotation`, `query_point`: FoldPlan's `rotations`, `query_rotation`).  `set_points`: per
    rotation set the indices of its rotations: polynomials with the same set of rotations share a set, sets and the polynomials inside one in
    order of first appearance; `slot_set`, `slot_pos`: a polynomial's set and its position inside it (the exponent of y)."""
    set_points: List[List[int]]
    slot_set: List[int]
    slot_pos: List[int]

    point_rotation = property(lambda self: self.rotations)
    query_point = property(lambda self: self.query_rotation)

    @property
    def n_sets(self) -> int:
        return len(self.set_points)

    @property
    def n_points(self) -> int:
        return len(self.rotations)

    def marshal(self, k: int):
        """-> (_lib.ShplonkPlan, the arrays it points into): rotations reduced mod 2^k.  ValueError: two rotations of the plan are equal mod 2^k
        (they would be one point)"""
        starts = [0]
        for pts in self.set_points:
            starts.append(starts[-1] + len(pts))
        flat = [t for pts in self.set_points for t in pts]
        return self._marshal(k, _lib.ShplonkPlan, (self.n_evals, self.n_sets, self.n_slots, self.n_points),
                             [starts, flat, self.slot_set, self.slot_pos, self.query_slot, self.query_rotation])


def shplonk_plan(plan_triples, shared_kinds=("fixed", "sigma")) -> ShplonkPlan:
    """the ShplonkPlan of the opened (kind, index, rotation) triples (prover.opening_plan); polynomials of a kind in `shared_kinds` are the key's"""
    common, keys = FoldPlan.fields_of(plan_triples, shared_kinds)
    by_poly = {}
    for key, t in zip(keys, common[2]):
        pts = by_poly.setdefault(key, [])                # a polynomial's rotations, polynomials in order of first appearance
        if t not in pts:
            pts.append(t)
    set_index, set_points, counts, set_of, pos_of = {}, [], [], {}, {}
    for key, pts in by_poly.items():
        i = set_index.setdefault(frozenset(pts), len(set_points))
        if i == len(set_points):
            set_points.append(list(pts))
            counts.append(0)
        set_of[key], pos_of[key] = i, counts[i]
        counts[i] += 1
    slot_keys = common[4] + common[5]                    # own, then shared
    return ShplonkPlan(*common, set_points, [set_of[key] for key in slot_keys], [pos_of[key] for key in slot_keys])


def shplonk_scalars_device(plan: ShplonkPlan, evals, points, k: int, stream=None):
    """zkhip_shplonk_scalars_device: evals (B, n_evals, 4), points (B, 4, 4) = x, y, v, u, contiguous int64 device tensors -> (rows_a (B, 2 +
    n_slots + 1, 4) over [H', H | own polynomials | key polynomials | G], rows_c (B, 1, 4), status (B,) int32), the column layout of
    include/zkhip.h: what `shplonk_accumulate` returns for each proof.  status[i] = 1: x Z_0 = 0 for proof i, its rows are zeros and the caller
    verifies it one by one.  Asynchronous on `stream`."""
    return _scalars_device("shplonk_scalars_device", plan, evals, points, 3, k, stream, [((2 + plan.n_slots + 1, 4), "int64"), ((1, 4), "int64"), ((), "int32")])


def fold_rows_device(rows, n_own: int, r, negate: bool, out_own, out_shared, stream=None) -> None:
    """zkhip_fr_fold_rows_device over rows (n, n_cols, 4) and multipliers r (n, 4): out_own (n * n_own elements) = +- r_i rows[i][j],
    out_shared (n_cols - n_own elements) = +- sum_i r_i rows[i][n_own + j]; either output may be None where it has no element"""
    n, n_cols = rows.shape[0], rows.shape[1]
    _lib.check(_lib.load().zkhip_fr_fold_rows_device(rows.data_ptr() if n else None, n_cols, n_own, r.data_ptr() if n else None, int(bool(negate)), n,
                                                     out_own.data_ptr() if out_own is not None and out_own.numel() else None,
                                                     out_shared.data_ptr() if out_shared is not None and out_shared.numel() else None, stream))


def _pairing_verdict(d_g1, d_g2, stream=None) -> bool:
    """THE final check of the batch verifier: zkhip_pairing_check_device over two pairs; its uint32 verdict is the only thing read back, behind the
    one host wait of a folded check.  Every folded check goes through this function (a test counts the calls)."""
    import torch

    lib = _lib.load()
    ok = torch.empty(1, dtype=torch.int32, device=d_g1.device)
    _lib.check(lib.zkhip_pairing_check_device(d_g1.data_ptr(), d_g2.data_ptr(), 2, ok.data_ptr(), stream))
    if stream:
        _lib.check(lib.zkhip_stream_sync(stream))
    return bool(int(ok.cpu()[0]))


def fold_check(params, rows_a, rows_c, own_points, shared_points, seed=None, stream_id: int = 0, stream=None) -> List[bool]:
    """The openings of B proofs decided by folded pairing checks -> B bools.  Device tensors (int64, contiguous): own_points (B, m, 8) affine, the
    multi-open's own points first; shared_points (t, 8); rows_a (B, m + t, 4), the scalars of A_i over [own points | shared points]; rows_c
    (B, c, 4), the scalars of C_i over the first c own points.  One check: r_0 .. r_(B-1) from zkhip_fr_random_device, two folds (the C side
    negated), two zkhip_msm_g1_device -- the A side over [own points | shared] with [r_i-scaled own scalars | shared sums], the C side over
    the B c own points --, zkhip_g1_batch_normalize_device on the two sums and one pairing check (`_pairing_verdict`).  A batch that fails is
    bisected with the same r_i: a failing range is split, its left half checked; if that passes the right half fails by bilinearity and is
    split in turn without a check of its own; a failing range of one proof is refused.  One bad proof among 16 costs at most 9 checks.
    seed: 32 bytes, the seed of the library's random stream (`stream_id`, elements 0 .. B - 1); None draws them from os.urandom -- the library
    holds no entropy.  A prover must not be able to predict r: a fixed seed is for tests.  r_i = 0 (probability 2^-254) is not handled.
    `stream`: None (torch's default stream, on which the tensors here are allocated) or a stream the caller keeps ordered with them."""
    import os

    import torch

    B, m = own_points.shape[0], own_points.shape[1]
    t, c = shared_points.shape[0], rows_c.shape[1]
    for name, ten, shape in (("rows_a", rows_a, (B, m + t, 4)), ("rows_c", rows_c, (B, c, 4)), ("own_points", own_points, (B, m, 8)), ("shared_points", shared_points, (t, 8))):
        if not (ten.is_cuda and ten.is_contiguous() and ten.dtype == torch.int64) or tuple(ten.shape) != shape:
            raise ValueError(f"fold_check: {name} is a contiguous int64 device tensor of shape {shape}")
    if not 1 <= c <= m:
        raise ValueError("fold_check: rows_c runs over the first c own points, 1 <= c <= m")
    if B == 0:
        return []
    if params.g2 is None or params.s_g2 is None:
        raise ValueError("the verifier needs g2 and s_g2")
    seed = os.urandom(32) if seed is None else bytes(seed)
    if len(seed) != 32:
        raise ValueError("the seed is 32 bytes")
    lib = _lib.load()
    dev = own_points.device
    r = torch.empty((B, 4), dtype=torch.int64, device=dev)
    _lib.check(lib.zkhip_fr_random_device(seed, stream_id, 0, B, r.data_ptr(), stream))
    g2 = torch.from_numpy(np.stack([np.asarray(params.g2, dtype=np.uint64).reshape(16), np.asarray(params.s_g2, dtype=np.uint64).reshape(16)]).view(np.int64)).to(dev)
    c_points = own_points[:, :c, :].contiguous()
    scal_a = torch.empty((B * m + t, 4), dtype=torch.int64, device=dev)
    scal_c = torch.empty((B * c, 4), dtype=torch.int64, device=dev)
    sums = torch.empty((2, 12), dtype=torch.int64, device=dev)
    pair = torch.empty((2, 8), dtype=torch.int64, device=dev)
    all_bases = torch.cat([own_points.reshape(B * m, 8), shared_points])

    def check(lo, hi):
        n = hi - lo
        fold_rows_device(rows_a[lo:hi], m, r[lo:hi], False, scal_a[:n * m], scal_a[n * m:n * m + t], stream)
        fold_rows_device(rows_c[lo:hi], c, r[lo:hi], True, scal_c[:n * c], None, stream)
        bases = all_bases if n == B else torch.cat([own_points[lo:hi].reshape(n * m, 8), shared_points])
        _lib.check(lib.zkhip_msm_g1_device(scal_a.data_ptr(), bases.data_ptr(), n * m + t, sums[0].data_ptr(), stream))
        _lib.check(lib.zkhip_msm_g1_device(scal_c.data_ptr(), c_points[lo:hi].data_ptr(), n * c, sums[1].data_ptr(), stream))
        _lib.check(lib.zkhip_g1_batch_normalize_device(sums.data_ptr(), 2, pair.data_ptr(), stream))
        return _pairing_verdict(pair, g2, stream)

    verdicts = [False] * B

    def accept(lo, hi):
        verdicts[lo:hi] = [True] * (hi - lo)

    def failing(lo, hi):                      # a range known to fail
        if hi - lo == 1:
            return
        mid = (lo + hi) // 2
        if check(lo, mid):
            accept(lo, mid)
            failing(mid, hi)                  # by bilinearity
            return
        failing(lo, mid)
        if check(mid, hi):
            accept(mid, hi)
        else:
            failing(mid, hi)

    if check(0, B):
        accept(0, B)
    else:
        failing(0, B)
    return verdicts

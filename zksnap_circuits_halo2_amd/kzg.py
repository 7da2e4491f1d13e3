"""`ParamsKZG<Bn256>` mirror [DEP halo2-axiom poly/kzg/commitment.rs] (setup / read / write: section 8(f) row 4):
owns `g` / `g_lagrange`, pins them in HBM once (`zkhip_register_bases`) and commits with the GPU MSM."""
from __future__ import annotations

import numpy as np

from . import _lib
from .arithmetic import best_multiexp
from .buffers import DeviceBuffer


def g_to_lagrange(g: np.ndarray, k: int) -> np.ndarray:
    """`g_to_lagrange(g_projective, k)` [DEP poly/kzg/commitment.rs]: the Lagrange-basis SRS of a monomial-basis SRS whose trapdoor is not
    known, g_lagrange[i] = (1/n) sum_j omega^(-i j) g[j] -- an inverse FFT over G1 points on the GPU (`zkhip_g_to_lagrange_device`)."""
    n = 1 << k
    g = np.ascontiguousarray(g, dtype=np.uint64).reshape(n, 8)
    with DeviceBuffer(n * 64) as d_in, DeviceBuffer(n * 64) as d_out:
        d_in.upload(g)
        _lib.check(_lib.load().zkhip_g_to_lagrange_device(d_in.ptr, k, d_out.ptr, None))
        return d_out.download((n, 8))


class ParamsKZG:
    def __init__(self, k: int, g: np.ndarray, g_lagrange: np.ndarray | None = None, g2: np.ndarray | None = None, s_g2: np.ndarray | None = None):
        self.k, self.n = k, 1 << k
        self.g = np.ascontiguousarray(g, dtype=np.uint64).reshape(self.n, 8)
        self.g_lagrange = None if g_lagrange is None else np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(self.n, 8)
        # G2Affine memory (16 u64), carried for the verifying key and the SRS file only (srs.py)
        self.g2 = None if g2 is None else np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        self.s_g2 = None if s_g2 is None else np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(16)
        lib = _lib.load()
        # The library recognises registered bases by host address (include/zkhip.h), so the registration must end before the arrays
        # are freed: `close()` / the context manager do it explicitly, and a finalizer does it when the object is collected without
        # either (the arrays are kept alive by the finalizer's own references until then).  The arrays are made read-only: the prepared
        # tables are built from their contents at registration.
        arrays = [self.g] + ([self.g_lagrange] if self.g_lagrange is not None else [])
        registered = []
        try:
            for a in arrays:
                _lib.check(lib.zkhip_register_bases(a.ctypes.data, self.n))
                registered.append(a)
        except Exception:
            for a in registered:
                lib.zkhip_unregister_bases(a.ctypes.data)
            raise
        # (np.ascontiguousarray hands back the caller's own array when it already is contiguous uint64: remember which arrays were
        # writeable and give that back when the registration ends, so that a caller's array is not left read-only for good)
        was_writeable = [bool(a.flags.writeable) for a in arrays]
        for a in arrays:
            a.flags.writeable = False
        import weakref

        self._finalizer = weakref.finalize(self, _unregister_arrays, arrays, was_writeable)

    @classmethod
    def setup(cls, k: int, s: int) -> "ParamsKZG":
        """`ParamsKZG::setup(k, rng)` [DEP poly/kzg/commitment.rs] with the trapdoor `s` given instead of drawn (what the reference's
        benches and `gen_srs` test parameters amount to: /root/reference/voter/benches/voter_circuit.rs:60): g[i] = [s^i] G and
        g_lagrange[i] = [(s^n - 1)/n * w^i / (s - w^i)] G, both computed on the GPU -- the scalar vectors with the Fr primitives
        (prefix product, row programs, batch inversion), the points with the fixed-base multiplication."""
        from . import evaluation as E
        from .fields import R_MOD, fr_encode, omega_for

        n = 1 << k
        s %= R_MOD
        omega = omega_for(k)
        assert pow(s, n, R_MOD) != 1, "the trapdoor lies in the evaluation domain"
        lib = _lib.load()
        with DeviceBuffer(n * 32) as d_sc, DeviceBuffer(n * 32) as d_tmp, DeviceBuffer(n * 64) as d_pts:
            def points() -> np.ndarray:
                _lib.check(lib.zkhip_g1_fixed_base_mul_device(d_sc.ptr, n, d_pts.ptr, None))
                return d_pts.download((n, 8))

            # s^i: exclusive prefix product of the constant vector (s, s, ...)
            d_sc.upload(np.tile(fr_encode([s]), (n, 1)))
            _lib.check(lib.zkhip_fr_prefix_product_device(d_sc.ptr, n, d_sc.ptr, None))
            g = points()
            # Lagrange scalars: (s - w^i) -> inverse -> times w^i * (s^n - 1) / n
            den = E.RowProgram(omega=omega)
            den.emit(E.OP_SUB, 0, den.constant(s), E.RowProgram.ROWPOW)
            den.run_device([], k, d_tmp.address)
            _lib.check(lib.zkhip_fr_batch_invert_device(d_tmp.ptr, n, None))
            num = E.RowProgram(omega=omega)
            num.emit(E.OP_MUL, 0, E.RowProgram.ROWPOW, num.column(0))
            num.emit(E.OP_MUL, 0, E.RowProgram.reg(0), num.constant((pow(s, n, R_MOD) - 1) * pow(n, -1, R_MOD) % R_MOD))
            num.run_device([d_tmp.address], k, d_sc.address)
            g_lagrange = points()
        from . import srs

        return cls(k, g, g_lagrange, srs.g2_encode(srs.G2_GENERATOR), srs.g2_encode(srs.g2_mul(s)))

    @classmethod
    def from_parts(cls, k: int, g: np.ndarray, g_lagrange: np.ndarray | None = None, g2: np.ndarray | None = None, s_g2: np.ndarray | None = None) -> "ParamsKZG":
        """`ParamsKZG::from_parts` [DEP]: the Lagrange basis is derived from g when it is not supplied"""
        return cls(k, g, g_to_lagrange(g, k) if g_lagrange is None else g_lagrange, g2, s_g2)

    def downsize(self, new_k: int) -> "ParamsKZG":
        """`ParamsKZG::downsize(k)` [DEP]: the first 2^k monomial-basis points, and their Lagrange basis re-derived with `g_to_lagrange`
        (the inverse FFT over G1 points on the GPU); returns a new object, as the mirror's arrays are pinned by address"""
        if new_k > self.k:
            raise ValueError("downsize: new_k > k")                                  # the reference asserts `new_k <= self.k`
        g = np.array(self.g[: 1 << new_k])
        return ParamsKZG(new_k, g, g_to_lagrange(g, new_k), self.g2, self.s_g2)

    def write(self, f) -> None:
        """`ParamsKZG::write` (SerdeFormat::RawBytes) [DEP]; layout in srs.py"""
        self.write_custom(f, "RawBytes")

    def write_custom(self, f, fmt: str, flag_layout: int = 0) -> None:
        """`ParamsKZG::write_custom(writer, format)` [DEP]: RawBytes / RawBytesUnchecked (the memory of the points) or Processed (every
        point compressed: the two tables on the GPU)"""
        from . import srs

        if self.g_lagrange is None or self.g2 is None or self.s_g2 is None:
            raise ValueError("write needs g_lagrange, g2 and s_g2")
        srs.write_params(f, self.k, self.g, self.g_lagrange, self.g2, self.s_g2, fmt, flag_layout)

    @classmethod
    def read(cls, f, check_points=None) -> "ParamsKZG":
        """`ParamsKZG::read` [DEP]: parses the file, verifies every point (one GPU pass per table: the RawBytes reader's check; pass a
        number to sample on the host instead, 0 for RawBytesUnchecked) and pins both tables in HBM"""
        from . import srs

        k, g, g_lagrange, g2, s_g2 = srs.read_params(f, check_points)
        return cls(k, g, g_lagrange, g2, s_g2)

    @classmethod
    def read_custom(cls, f, fmt: str, flag_layout: int = 0) -> "ParamsKZG":
        """`ParamsKZG::read_custom(reader, format)` [DEP]"""
        from . import srs

        k, g, g_lagrange, g2, s_g2 = srs.read_params(f, None, fmt=fmt, flag_layout=flag_layout)
        return cls(k, g, g_lagrange, g2, s_g2)

    def get_g2(self) -> np.ndarray:
        return self.g2

    def get_s_g2(self) -> np.ndarray:
        return self.s_g2

    def get_g(self) -> np.ndarray:
        return self.g

    def commit(self, poly: np.ndarray) -> np.ndarray:
        poly = np.ascontiguousarray(poly, dtype=np.uint64).reshape(-1, 4)
        assert poly.shape[0] <= self.n
        return best_multiexp(poly, self.g[: poly.shape[0]])

    def commit_lagrange(self, poly: np.ndarray) -> np.ndarray:
        assert self.g_lagrange is not None
        poly = np.ascontiguousarray(poly, dtype=np.uint64).reshape(-1, 4)
        assert poly.shape[0] <= self.n
        return best_multiexp(poly, self.g_lagrange[: poly.shape[0]])

    def commit_device(self, d_poly: int, length: int, d_out: int, lagrange: bool = False, stream: int = 0) -> None:
        """`commit` / `commit_lagrange` of a polynomial that lives in HBM (`length` elements at device address d_poly), against the
        tables this object registered: the 96-byte Jacobian result is written to device address d_out, asynchronously on `stream`"""
        bases = self.g_lagrange if lagrange else self.g
        assert bases is not None and length <= self.n
        _lib.check(_lib.load().zkhip_msm_g1_registered_device(bases.ctypes.data, d_poly, length, d_out, stream))

    def commit_many_device(self, d_polys: int, length: int, count: int, stride: int, d_out: int, lagrange: bool = False, stream: int = 0) -> None:
        """`count` polynomials that live in HBM (polynomial i: `length` elements at d_polys + i * stride elements) committed by one call
        against the registered tables -- all advice columns of a circuit: small MSMs share launch sets (include/zkhip.h
        zkhip_msm_g1_registered_batch_device); `count` Jacobian results (96 bytes each) at device address d_out, asynchronously on `stream`"""
        bases = self.g_lagrange if lagrange else self.g
        assert bases is not None and length <= self.n and stride >= length
        _lib.check(_lib.load().zkhip_msm_g1_registered_batch_device(bases.ctypes.data, d_polys, length, count, stride, d_out, stream))

    def commit_many(self, polys: np.ndarray, lagrange: bool = False) -> np.ndarray:
        """Commit to K polynomials of equal length at once ((K, len, 4) uint64) -> (K, 12) uint64: one launch set."""
        polys = np.ascontiguousarray(polys, dtype=np.uint64)
        assert polys.ndim == 3 and polys.shape[2] == 4 and polys.shape[1] <= self.n
        bases = self.g_lagrange if lagrange else self.g
        assert bases is not None
        out = np.zeros((polys.shape[0], 12), dtype=np.uint64)
        _lib.check(_lib.load().zkhip_msm_g1_batch(polys.ctypes.data, bases.ctypes.data, polys.shape[1], polys.shape[0], out.ctypes.data))
        return out

    # ---- verification (the pairing check: zkhip_pairing_check) ------------------------------------------------------------------------
    def _g_xyz(self) -> np.ndarray:
        from .multiopen import _generator_xyz

        return _generator_xyz(self)

    def verify_opening(self, commitment: np.ndarray, z: int, value: int, witness: np.ndarray) -> bool:
        """The single-point KZG check e(C - value G + z W, g2) e(-W, [s]_2) = 1: `witness` commits to (p(X) - value) / (X - z).
        commitment, witness: 12-limb Jacobian points."""
        from .arithmetic import g1_combination, pairing_check

        if self.g2 is None or self.s_g2 is None:
            raise ValueError("verify_opening needs g2 and s_g2")
        C_ = np.ascontiguousarray(commitment, dtype=np.uint64).reshape(12)
        W = np.ascontiguousarray(witness, dtype=np.uint64).reshape(12)
        left = g1_combination([1, -value, z], np.stack([C_, self._g_xyz(), W]))
        right_neg = g1_combination([-1], W.reshape(1, 12))
        return pairing_check(np.stack([left, right_neg]), np.stack([self.g2, self.s_g2]))

    def verify(self, seed: bytes) -> bool:
        """Is this a powers-of-tau string with its Lagrange table?  What `read` / `read_custom` can be followed by: a file's points are checked
        to be on the curve when it is read, but only a pairing can tell whether g[i] = [s^i] G for the s of s_g2 (nobody knows s for a real file).
        (a) every point of g and g_lagrange on the curve; g2 and s_g2 on the twist and of order r (msm_g2([r - 1], [Q]) = -Q: an Fr scalar cannot hold r);
        (b) with rho drawn from `seed`: e(sum rho_i g[i + 1], g2) = e(sum rho_i g[i], [s]_2) -- one false g[i] passes with probability 1 / r;
        (c) g[0] and g2 are not the identity;
        (d) with a second vector rho': commit_lagrange(rho') = commit(lagrange_to_coeff(rho')).
        `seed`: 32 bytes of the caller's own randomness."""
        import ctypes as C

        from . import srs
        from .arithmetic import best_multiexp, best_multiexp_g2, g1_combination, pairing_check, random_fr
        from .domain import EvaluationDomain
        from .fields import R_MOD, fr_encode

        if self.g_lagrange is None or self.g2 is None or self.s_g2 is None:
            return False
        lib = _lib.load()
        n = self.n
        # (a), (c)
        for table in (self.g, self.g_lagrange):
            bad = C.c_uint64(0)
            _lib.check(lib.zkhip_g1_check_points(table.ctypes.data, n, C.byref(bad)))
            if bad.value != n:
                return False
        if not self.g[0].any() or not self.g2.any():
            return False
        minus_one = fr_encode([R_MOD - 1])
        for q2 in (self.g2, self.s_g2):
            try:
                P = srs.g2_decode(q2)
            except Exception:   # noqa: BLE001  (not canonical)
                return False
            if P is None or not srs.g2_is_on_curve(P):
                return False
            if _g2_jacobian_to_affine(best_multiexp_g2(minus_one, q2.reshape(1, 16))) != (P[0], srs._f2sub((0, 0), P[1])):
                return False
        # (b)
        if n > 1:
            rho = random_fr(seed, n - 1, stream_id=0x5352535F52484F31)
            left = g1_combination([1], best_multiexp(rho, self.g[1:]).reshape(1, 12))
            right_neg = g1_combination([-1], best_multiexp(rho, self.g[: n - 1]).reshape(1, 12))
            if not pairing_check(np.stack([left, right_neg]), np.stack([self.g2, self.s_g2])):
                return False
        # (d)
        rho2 = random_fr(seed, n, stream_id=0x5352535F52484F32)
        dom = EvaluationDomain(2, self.k)
        coeffs = dom.lagrange_to_coeff(rho2.copy())
        lhs = g1_combination([1], self.commit_lagrange(rho2).reshape(1, 12))
        rhs = g1_combination([1], self.commit(coeffs).reshape(1, 12))
        return bool(np.array_equal(lhs, rhs))

    def close(self) -> None:
        """end the residency of g / g_lagrange (idempotent); also runs when the object is garbage-collected"""
        self._finalizer()

    def __enter__(self) -> "ParamsKZG":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def _unregister_arrays(arrays, was_writeable=()) -> None:
    try:
        lib = _lib.load()
    except Exception:   # noqa: BLE001  (interpreter shutdown)
        return
    for a in arrays:
        lib.zkhip_unregister_bases(a.ctypes.data)
    for a, w in zip(arrays, was_writeable):
        if w:
            try:
                a.flags.writeable = True
            except ValueError:   # a view of a read-only base
                pass


def _g2_jacobian_to_affine(xyz: np.ndarray):
    """24 limbs (x | y | z over Fq2, Montgomery) -> ((x0, x1), (y0, y1)) as integers, None for the identity"""
    from . import srs
    from .fields import Q_MOD

    inv_r = pow(1 << 256, -1, Q_MOD)
    v = [sum(int(w) << (64 * j) for j, w in enumerate(xyz[4 * c:4 * c + 4])) * inv_r % Q_MOD for c in range(6)]
    X, Y, Zc = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
    if Zc == (0, 0):
        return None
    zi = srs._f2inv(Zc)
    zi2 = srs._f2mul(zi, zi)
    return srs._f2mul(X, zi2), srs._f2mul(Y, srs._f2mul(zi2, zi))

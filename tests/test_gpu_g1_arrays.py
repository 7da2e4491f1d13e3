"""GPU (-m gpu): the G1 kernels that work on arrays of points -- batch normalisation, the G1 FFT / g_to_lagrange, fixed-base
multiplication, the generator walk, the Jacobian sum and the point validation -- at the sizes where their per-thread chunking switches
and on the inputs the Montgomery trick, the signed-digit carry chain and the shuffle tree get wrong first.

Every expectation comes from oracle/cpu_ref (the C restatement) or from Python integers; no library result is the expectation of
another.  Outputs are compared limb for limb (canonical Montgomery limbs), Jacobian outputs after `cref.jac_to_affine`, and whole arrays
are compared except for the 2^17 / 2^18 transforms, which get a >= 1024-index sample plus a whole-array check through the oracle's MSM."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F
from zksnap_circuits_halo2_amd.tensors import from_words

pytestmark = pytest.mark.gpu

Q, R = O.Q_MOD, O.R_MOD
THREADS = 8
limbs = lambda v: np.array(O.limbs4(v), dtype=np.uint64)
ONE_Q = limbs(O.to_mont(1, Q))
Q_LIMBS = O.limbs4(Q)
ID_HALO2 = np.concatenate([np.zeros(4, np.uint64), ONE_Q, np.zeros(4, np.uint64)])      # `G1::identity()`: (0, 1, 0)
EINVAL = -1


# ---------------------------------------------------------------- plumbing
class Dev:
    """a device buffer from zkhip_alloc; filled with 0xA5 bytes so that an element the kernel never wrote cannot pass"""

    def __init__(self, lib, nbytes, fill=True):
        self.lib, self.nbytes, self.p = lib, nbytes, C.c_void_p()
        _lib.check(lib.zkhip_alloc(max(nbytes, 256), C.byref(self.p)))
        if fill and nbytes:
            self.put(np.full(nbytes, 0xA5, dtype=np.uint8))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.zkhip_free(self.p)

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        if arr.nbytes:
            _lib.check(self.lib.zkhip_upload(self.p, arr.ctypes.data, arr.nbytes))

    def get(self, rows, cols):
        out = np.zeros((rows, cols), dtype=np.uint64)
        if out.nbytes:
            _lib.check(self.lib.zkhip_download(out.ctypes.data, self.p, out.nbytes))   # blocking copy on the stream the kernels ran on
        return out


def to_ints(a):
    """(n, 4) uint64 limbs -> the n raw integers"""
    return from_words(np.asarray(a, dtype=np.uint64).reshape(-1, 4))


def all_below_q(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    lt, eq = np.zeros(a.shape[0], dtype=bool), np.ones(a.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (a[:, i] < np.uint64(Q_LIMBS[i]))
        eq &= a[:, i] == np.uint64(Q_LIMBS[i])
    return bool(lt.all())


def same(got, exp):
    """limb-for-limb equality of two arrays, reporting the first rows that differ"""
    assert got.shape == exp.shape
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        pytest.fail(f"{bad.size} of {got.shape[0]} rows differ, first at {bad[:8].tolist()}")


def multiple_of_g(cref, k):
    return cref.jac_to_affine(cref.scalar_mul(k % R, cref.generator()))


def multiples_of_g(cref, ks):
    return np.array([multiple_of_g(cref, k) for k in ks], dtype=np.uint64).reshape(len(ks), 8)


def normalise_on_cpu(cref, xyz):
    """every Jacobian point through the oracle's jac_to_affine (one field inversion each), after checking that the limbs are canonical"""
    xyz = np.ascontiguousarray(xyz)
    assert all_below_q(xyz), "non-canonical Jacobian limbs"
    n = xyz.shape[0]
    out = np.zeros((n, 8), dtype=np.uint64)
    fn, pin, pout = cref.load().ref_jac_to_affine, xyz.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(C.c_void_p(pin + 96 * i), C.c_void_p(pout + 64 * i))
    return out


def jacobian_of(cref, affine, seed, keep_one=4):
    """another representative (x z^2, y z^3, z) of every affine point, z seeded per point; every `keep_one`-th point keeps z = 1 and
    an affine (0, 0) becomes (0, 1, 0).  Built in bulk with the oracle's Fq multiplication."""
    n = affine.shape[0]
    z = cref.gen_scalars(seed, n, 0)                 # Montgomery limbs of an Fr element: integers below r < q, canonical in Fq as they stand
    z[~z.any(axis=1)] = ONE_Q
    z[::keep_one] = ONE_Q
    x, y = np.ascontiguousarray(affine[:, :4]), np.ascontiguousarray(affine[:, 4:])
    z2 = cref.field_op(0, 3, z, z)
    z3 = cref.field_op(0, 0, z2, z)
    jac = np.empty((n, 12), dtype=np.uint64)
    jac[:, 0:4], jac[:, 4:8], jac[:, 8:12] = cref.field_op(0, 0, x, z2), cref.field_op(0, 0, y, z3), z
    jac[~affine.any(axis=1)] = ID_HALO2
    return jac


def make_identity(jac, i, encoding):
    """encoding 0: (0, 1, 0) as halo2curves writes it; 1: (x, y, 0) with the non-zero x, y the row holds"""
    if encoding == 0:
        jac[i] = ID_HALO2
    else:
        assert jac[i, 0:4].any() and jac[i, 4:8].any()
        jac[i, 8:12] = 0


def negated(cref, affine):
    out = affine.copy()
    out[:, 4:] = cref.field_op(0, 2, np.zeros((affine.shape[0], 4), dtype=np.uint64), np.ascontiguousarray(affine[:, 4:]))
    return out


# ---------------------------------------------------------------- 1. batch normalisation
NORMALIZE_SIZES = [0, 1, 2, 63, 64, 65, 1000, (1 << 17) - 1, 1 << 17, (1 << 17) + 1, (1 << 18) + 3, (1 << 19) + 1, (1 << 20) + 5, (1 << 21) + 7]
NORMALIZE_HOST_SIZES = {0, 1, 2, 63, 64, 65, 1000, (1 << 17) + 1, (1 << 19) + 1, (1 << 21) + 7}


def affine_chunk(n):
    """points that share one inversion in the final normalisation (csrc/msm.hip affine_chunk): 32 once 65536 threads have a full chunk"""
    ch = 32
    while ch > 1 and n // ch < 65536:
        ch >>= 1
    return ch


def test_chunk_lengths_the_sizes_are_chosen_around():
    assert [affine_chunk(n) for n in NORMALIZE_SIZES] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 4, 8, 16, 32]
    assert [affine_chunk((1 << k) - 1) for k in range(17, 22)] == [1, 2, 4, 8, 16]


def identity_positions(n, ch):
    """first and last of a chunk, a whole chunk, two neighbours inside a chunk (across two when ch < 4), index 0 and index n - 1"""
    if n == 0:
        return []
    nch = (n + ch - 1) // ch
    pos = {0, n - 1, (nch // 5) * ch, (nch // 4) * ch + ch - 1}
    pos.update(range((nch // 3) * ch, (nch // 3) * ch + ch))
    c = (nch // 2) * ch + max(ch // 2 - 1, 0)
    pos.update((c, c + 1))
    return sorted(p for p in pos if 0 <= p < n)


def normalize_device(lib, jac):
    n = jac.shape[0]
    with Dev(lib, n * 96, fill=False) as d_in, Dev(lib, n * 64) as d_out:
        d_in.put(jac)
        _lib.check(lib.zkhip_g1_batch_normalize_device(d_in.p, n, d_out.p, None))
        return d_out.get(n, 8)


def normalize_host(lib, jac):
    jac = np.ascontiguousarray(jac)
    out = np.full((jac.shape[0], 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    _lib.check(lib.zkhip_g1_batch_normalize(jac.ctypes.data, jac.shape[0], out.ctypes.data))
    return out


@pytest.mark.parametrize("n", NORMALIZE_SIZES)
def test_batch_normalize_whole_array(lib, cref, n):
    """Curve::batch_normalize of another Jacobian representative of every point of an oracle-made affine array gives that array back,
    without and with identities (both encodings) at every position of a shared-inversion chunk"""
    expect, _, _ = cref.gen_bases(0x6E6F726D00 + n, n)
    jac = jacobian_of(cref, expect, 0x7A7A00 + n)
    entries = [("device", normalize_device)] + ([("host", normalize_host)] if n in NORMALIZE_HOST_SIZES else [])
    for name, run in entries:
        same(run(lib, jac), expect)
    pos = identity_positions(n, affine_chunk(n))
    for t, i in enumerate(pos):
        make_identity(jac, i, t & 1)
        expect[i] = 0
    # the construction itself, against the oracle's own normalisation, on a sample and on every identity
    rng = random.Random(n)
    for i in sorted(set(pos) | {rng.randrange(n) for _ in range(min(n, 64))}):
        assert np.array_equal(cref.jac_to_affine(jac[i]), expect[i]), i
    for name, run in entries:
        same(run(lib, jac), expect)


# ---------------------------------------------------------------- 2. G1 FFT and g_to_lagrange
def fft_inputs(cref, seed, log_n):
    """points a_j G with a_j = t0 + j d from the oracle; some are the identity (a_j = 0), two copies of one point sit next to each other
    and a third half the array away, where the first butterfly adds and subtracts them"""
    n = 1 << log_n
    bases, t0, d = cref.gen_bases(seed, n)
    a = [(t0 + j * d) % R for j in range(n)]
    for j in (1, n // 2, n - 1, n // 3, n // 3 + 1):
        bases[j], a[j] = 0, 0
    for j in (3, 2 + n // 2):
        bases[j], a[j] = bases[2], a[2]
    return bases, a


def transform_scalars(cref, a, omega, log_n, divisor=None):
    arr = F.fr_encode(a)
    cref.best_fft(arr, F.fr_encode([omega])[0], log_n, THREADS)
    if divisor is not None:
        cref.scale(arr, F.fr_encode([divisor])[0])
    return F.fr_decode(arr)


def sample_indices(n, seed, count=1024):
    rng = random.Random(seed)
    return sorted({0, 1, n // 2, n - 1} | set(rng.sample(range(n), count)))


def assert_oracle_msm(cref, points_affine, e, seed):
    """whole-array check with the oracle alone: for a seeded random c, MSM_oracle(c, points) = [sum c_i e_i] G"""
    c = cref.gen_scalars(seed, len(e), 0)
    total = sum(x * y for x, y in zip(F.fr_decode(c), e)) % R
    got = cref.jac_to_affine(cref.best_multiexp(c, np.ascontiguousarray(points_affine), THREADS))
    assert np.array_equal(got, multiple_of_g(cref, total))


def g1_fft(lib, jac, log_n):
    n = 1 << log_n
    with Dev(lib, n * 96, fill=False) as d:
        d.put(jac)
        _lib.check(lib.zkhip_g1_fft_device(d.p, F.fr_encode([O.omega_for(log_n)])[0].ctypes.data, log_n, None))
        return d.get(n, 12)


@pytest.mark.parametrize("log_n", [8, 10, 13])
def test_g1_fft_every_output_point(lib, cref, log_n):
    bases, a = fft_inputs(cref, 0xF0F7 + log_n, log_n)
    out = g1_fft(lib, jacobian_of(cref, bases, 0xF0F8 + log_n, keep_one=3), log_n)
    e = transform_scalars(cref, a, O.omega_for(log_n), log_n)
    same(normalise_on_cpu(cref, out), multiples_of_g(cref, e))


def test_g1_fft_2pow17_sample_and_oracle_msm(lib, cref):
    log_n = 17
    n = 1 << log_n
    bases, a = fft_inputs(cref, 0xF117, log_n)
    out = normalise_on_cpu(cref, g1_fft(lib, jacobian_of(cref, bases, 0xF118, keep_one=3), log_n))
    e = transform_scalars(cref, a, O.omega_for(log_n), log_n)
    idx = sample_indices(n, 0xF119)
    same(out[idx], multiples_of_g(cref, [e[i] for i in idx]))
    assert_oracle_msm(cref, out, e, 0xF11A)


@pytest.mark.parametrize("k", [17, 18])
def test_g_to_lagrange_at_normalisation_chunks_2_and_4(lib, cref, k):
    """g_to_lagrange ends in the chunked normalisation: 2 points per inversion at k = 17, 4 at k = 18, with identities among the outputs'
    neighbours (zeroed inputs stay in).  Host entry: Jacobian input with mixed z; device entry: affine input."""
    n = 1 << k
    assert affine_chunk(n) == {17: 2, 18: 4}[k]
    bases, a = fft_inputs(cref, 0x1A60 + k, k)
    omega_inv, n_inv = pow(O.omega_for(k), -1, R), pow(n, -1, R)
    e = transform_scalars(cref, a, omega_inv, k, divisor=n_inv)
    idx = sample_indices(n, 0x1A70 + k)
    expect = multiples_of_g(cref, [e[i] for i in idx])

    jac = jacobian_of(cref, bases, 0x1A80 + k, keep_one=3)
    host = np.full((n, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    _lib.check(lib.zkhip_g_to_lagrange(jac.ctypes.data, k, host.ctypes.data))
    with Dev(lib, n * 64) as d_in, Dev(lib, n * 64) as d_out:
        d_in.put(bases)
        _lib.check(lib.zkhip_g_to_lagrange_device(d_in.p, k, d_out.p, None))
        dev = d_out.get(n, 8)
    for name, out in (("host", host), ("device", dev)):
        assert all_below_q(out), name
        same(out[idx], expect)
        assert_oracle_msm(cref, out, e, 0x1A90 + k)


# ---------------------------------------------------------------- 3. fixed-base multiplication
def fixed_base_mul(lib, scalars):
    n = len(scalars)
    with Dev(lib, n * 32) as d_s, Dev(lib, n * 64) as d_out:
        d_s.put(F.fr_encode(scalars))
        _lib.check(lib.zkhip_g1_fixed_base_mul_device(d_s.p, n, d_out.p, None))
        return d_out.get(n, 8)


def from_digits(digits):
    """the integer whose 16-bit windows, lowest first, are `digits`"""
    return sum(v << (16 * w) for w, v in enumerate(digits))


def fixed_base_edge_scalars():
    top = R >> 240                                                   # 0x3064: the top window of r
    assert from_digits([0xFFFF] * 15 + [top - 1]) < R < from_digits([0] * 15 + [top + 1])
    edge = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, (1 << 16) - 1, 1 << 16]
    for w in range(16):
        edge += [v for v in (1 << 16 * w, (1 << 16 * w) - 1, 1 << (16 * w + 15), (1 << (16 * w + 15)) - 1) if v < R]
    edge += [from_digits([0x8000] * 16) % R, from_digits([0x7FFF] * 16) % R]
    # digits of 2^15 in every window that fits below r (each takes the negative digit and carries), and their neighbours
    edge += [from_digits([0x8000] * 15 + [top - 1]), from_digits([0x7FFF] * 15 + [top - 1]), from_digits([0x8000] * 15)]
    # the largest value below r whose low 15 windows are all 0xffff: -1, then fifteen carries through zero digits, and the carry lifts the top
    # window to 0x3064, the largest it can be (r's own window 14 is 0x4e72 < 2^15, so with 0x3064 on top nothing carries into it).  It is also
    # the largest value below r whose low windows carry into the top one.
    edge += [from_digits([0xFFFF] * 15 + [top - 1]), from_digits([0xFFFF] * 14 + [0x7FFF, top - 1])]
    assert all(0 <= v < R for v in edge)
    return edge


def test_fixed_base_mul_edge_scalars(lib, cref):
    """signed 16-bit digits: 2^15 exactly, carries through every window, the top window at its largest; zero scalars (identities) first,
    last and alone in the middle of a 32-scalar inversion chunk, and one chunk of 32 zeros"""
    edge = [v for v in fixed_base_edge_scalars() if v]
    edge += F.fr_decode(cref.gen_scalars(0xF1BA5E, 64, 0))
    scalars = [0] + edge[:14] + [0] + edge[14:29] + [0] + [0] * 32 + edge[29:] + [0, 0]
    assert scalars[0] == scalars[31] == scalars[15] == 0 and all(scalars[1:15]) and all(scalars[16:31]) and not any(scalars[32:64])
    got = fixed_base_mul(lib, scalars)
    expect = multiples_of_g(cref, scalars)
    assert not expect[0].any() and not expect[32:64].any() and expect[1].any()
    same(got, expect)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 2047, 2048, 2049, 70001])
def test_fixed_base_mul_reproduces_gen_bases(lib, cref, n):
    expect, t0, d = cref.gen_bases(0xF1BA00 + n, n)
    same(fixed_base_mul(lib, [(t0 + i * d) % R for i in range(n)]), expect)


# ---------------------------------------------------------------- 4. generator walk
def gen_walk(lib, t0, d, n):
    t0_m, d_m = F.fr_encode([t0])[0], F.fr_encode([d])[0]
    with Dev(lib, n * 64) as d_out:
        _lib.check(lib.zkhip_g1_gen_walk_device(t0_m.ctypes.data, d_m.ctypes.data, n, d_out.p, None))
        return d_out.get(n, 8)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 2049, (1 << 16) + 1])
def test_gen_walk_reproduces_gen_bases(lib, cref, n):
    expect, t0, d = cref.gen_bases(0x3A1C00 + n, n)
    same(gen_walk(lib, t0, d, n), expect)


WALK_D = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
WALKS = {
    "t0 = d: the first step is a doubling": (WALK_D, WALK_D),
    "t0 = 0": (0, WALK_D),
    "t0 = -d": (-WALK_D % R, WALK_D),
    "t0 = -37 d: the identity inside the second chunk": (-37 * WALK_D % R, WALK_D),
    "t0 = -32 d: the identity first in a chunk": (-32 * WALK_D % R, WALK_D),
    "d = 0: n equal points": (WALK_D, 0),
    "d = 0 and t0 = 0: all identities": (0, 0),
    "d = r - 1": (0x1234567, R - 1),
}


@pytest.mark.parametrize("walk", list(WALKS))
def test_gen_walk_chosen_walks(lib, cref, walk):
    t0, d = WALKS[walk]
    n = 101
    same(gen_walk(lib, t0, d, n), multiples_of_g(cref, [t0 + i * d for i in range(n)]))


# ---------------------------------------------------------------- 5. sum of Jacobian points
SUM_SIZES = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 65, 200]
_points = {}


def random_points(cref):
    if "p" not in _points:
        _points["p"] = multiples_of_g(cref, F.fr_decode(cref.gen_scalars(0x53554D, max(SUM_SIZES) + 1, 0)))
    return _points["p"]


def fold(cref, jac):
    acc = ID_HALO2.copy()
    for row in jac:
        acc = cref.jac_add(acc, np.ascontiguousarray(row))
    return acc


def sum_cases(cref, m):
    """(name, m Jacobian points) -- every case has mixed z, so equal points meet as different representatives"""
    P = random_points(cref)[:m].copy()
    spare = random_points(cref)[m]
    seed = 0x5EED00 + m
    J = lambda affine, s=0: jacobian_of(cref, np.ascontiguousarray(affine), seed + s, keep_one=3)
    cases = [("random", J(P))]
    scattered = J(P, 1)
    for t, i in enumerate(sorted({0, m - 1, m // 2, 5, 21, 6, 7} & set(range(m)))):
        make_identity(scattered, i, t & 1)
    cases.append(("identities of both encodings", scattered))
    cases.append(("all points equal", J(np.broadcast_to(spare, (m, 8)), 2)))
    idx = np.arange(m)
    for sign in (1, -1):
        placements = [("i and i + 16", np.where(idx % 32 >= 16, idx - 16, idx))] + [(f"i and i ^ {b}", idx & ~b) for b in (1, 2, 4, 8)]
        for s, (name, src) in enumerate(placements):
            A = P[src]
            if sign < 0:
                A = np.where((src != idx)[:, None], negated(cref, A), A)
            cases.append((("equal: " if sign > 0 else "opposite: ") + name, J(A, 3 + s)))
    if m >= 2:
        head = J(P[:m - 1], 9)
        total = cref.jac_to_affine(fold(cref, head))
        cases.append(("cancels to the identity", np.vstack([head, J(negated(cref, total.reshape(1, 8)), 10)])))
    return cases


def g1_sum_device(lib, jac):
    m = jac.shape[0]
    with Dev(lib, m * 96) as d_in, Dev(lib, 96) as d_out:
        d_in.put(jac)
        _lib.check(lib.zkhip_g1_sum_device(d_in.p, m, d_out.p, None))
        return d_out.get(1, 12)[0]


def g1_sum_host(lib, jac):
    jac = np.ascontiguousarray(jac)
    out = np.full(12, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    _lib.check(lib.zkhip_g1_sum(jac.ctypes.data if jac.shape[0] else None, jac.shape[0], out.ctypes.data))
    return out


@pytest.mark.parametrize("entry", [g1_sum_device, g1_sum_host], ids=["device", "host"])
@pytest.mark.parametrize("m", SUM_SIZES)
def test_g1_sum_against_a_left_fold(lib, cref, m, entry):
    """16 quads, a strided loop for m > 16 and a shuffle tree: equal and opposite partial sums meet in every tree step, a quad adds a
    point to itself, identities of both encodings sit in the input"""
    for name, jac in sum_cases(cref, m):
        got = entry(lib, jac)
        assert all_below_q(got), (name, "non-canonical limbs")
        expect = cref.jac_to_affine(fold(cref, jac))
        assert np.array_equal(cref.jac_to_affine(got), expect), name
        if name == "all points equal":
            assert np.array_equal(expect, cref.jac_to_affine(cref.scalar_mul(m, random_points(cref)[m]))), name
        if name == "cancels to the identity" or m == 0:
            assert not expect.any(), name
        if name == "cancels to the identity":
            assert np.array_equal(got, ID_HALO2), "the identity is stored as (0, 1, 0)"


# ---------------------------------------------------------------- 6. point validation
def point_is_valid(xr, yr):
    """G1Affine::read_raw's check on the raw limbs: both coordinates canonical, and (0, 0) or y^2 = x^3 + 3"""
    if xr >= Q or yr >= Q:
        return False
    if xr == 0 and yr == 0:
        return True
    x, y = O.from_mont(xr, Q), O.from_mont(yr, Q)
    return (y * y - x * x * x - 3) % Q == 0


def first_bad(table):
    xs, ys = to_ints(table[:, :4]), to_ints(table[:, 4:])
    return next((i for i, (x, y) in enumerate(zip(xs, ys)) if not point_is_valid(x, y)), len(xs))


def raw_point(x, y):
    assert x < 1 << 256 and y < 1 << 256
    return np.array(O.limbs4(x) + O.limbs4(y), dtype=np.uint64)


CORRUPTIONS = {
    "low bit of x flipped": lambda x, y: (x ^ 1, y),
    "top bit of y flipped": lambda x, y: (x, y ^ (1 << 255)),
    "x + q": lambda x, y: (x + Q, y),
    "y + q": lambda x, y: (x, y + Q),
    "x = q, y = 0": lambda x, y: (Q, 0),
    "(0, y)": lambda x, y: (0, y),
    "(x, 0)": lambda x, y: (x, 0),
    "(q, q)": lambda x, y: (Q, Q),
}
CHECK_N = 5000
CHECK_AT = [0, 255, 256, 4095, 4096, CHECK_N - 1]


def check_table(cref):
    table, _, _ = cref.gen_bases(0xC4EC, CHECK_N)
    table[10] = 0
    table[257] = 0
    table[4998] = 0
    table[1::7] = negated(cref, table[1::7])
    assert first_bad(table) == CHECK_N
    return table


def check_device(lib, table, n=None):
    n = table.shape[0] if n is None else n
    bad = C.c_uint64(0xA5A5A5A5)
    with Dev(lib, table.nbytes) as d:
        d.put(table)
        _lib.check(lib.zkhip_g1_check_points_device(d.p, n, C.byref(bad), None))
    return bad.value


def check_host(lib, table, n=None):
    n = table.shape[0] if n is None else n
    bad = C.c_uint64(0xA5A5A5A5)
    _lib.check(lib.zkhip_g1_check_points(table.ctypes.data, n, C.byref(bad)))
    return bad.value


CHECK_ENTRIES = pytest.mark.parametrize("entry", [check_device, check_host], ids=["device", "host"])


@CHECK_ENTRIES
@pytest.mark.parametrize("what", list(CORRUPTIONS))
def test_check_points_names_the_corrupted_index(lib, cref, entry, what):
    table = check_table(cref)
    for i in CHECK_AT:
        t = table.copy()
        x, y = to_ints(t[i, :4])[0], to_ints(t[i, 4:])[0]
        assert x and y
        t[i] = raw_point(*CORRUPTIONS[what](x, y))
        assert first_bad(t) == i, "the predicate itself refuses the corrupted point"
        assert entry(lib, t) == i, (what, i)


@CHECK_ENTRIES
def test_check_points_smallest_index_empty_table_and_null(lib, cref, entry):
    table = check_table(cref)
    assert entry(lib, table) == CHECK_N                                    # untouched: n
    assert entry(lib, table, 0) == 0                                       # n = 0
    for group in ([4096, 300, 4999], [4999, 4097, 4096], [256, 255], [4999]):
        t = table.copy()
        for j, i in enumerate(group):
            t[i] = raw_point(*list(CORRUPTIONS.values())[j](to_ints(t[i, :4])[0], to_ints(t[i, 4:])[0]))
        assert first_bad(t) == min(group)
        assert entry(lib, t) == min(group), group
    if entry is check_host:
        assert lib.zkhip_g1_check_points(table.ctypes.data, CHECK_N, None) == EINVAL
    else:
        with Dev(lib, table.nbytes) as d:
            d.put(table)
            assert lib.zkhip_g1_check_points_device(d.p, CHECK_N, None, None) == EINVAL


def test_check_points_host_second_upload_chunk(lib, cref):
    """the host entry uploads 2^24 points at a time: a bad point in the second upload is reported at its index in the whole array, and
    a bad point that ends the first upload wins over it"""
    tile, _, _ = cref.gen_bases(0xC4ED, 1 << 16)
    assert first_bad(tile) == 1 << 16
    n = (1 << 24) + 1000
    big = np.empty((n, 8), dtype=np.uint64)
    big[:1 << 24].reshape(1 << 8, 1 << 16, 8)[:] = tile
    big[1 << 24:] = tile[:1000]
    i = (1 << 24) + 7
    big[i] = raw_point(to_ints(big[i, :4])[0] ^ 1, to_ints(big[i, 4:])[0])
    assert not point_is_valid(to_ints(big[i, :4])[0], to_ints(big[i, 4:])[0])
    assert check_host(lib, big) == i
    j = (1 << 24) - 1
    big[j] = raw_point(to_ints(big[j, :4])[0], to_ints(big[j, 4:])[0] + Q)
    assert check_host(lib, big) == j

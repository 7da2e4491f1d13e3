"""Structured inputs of the Fr transform tests (a helper module: no tests, no fixtures; nothing here imports the package under test).

Everything works on the external Montgomery-256 WORDS as integers below r.  The transform is linear and the Montgomery map x -> x 2^256 is
linear too, so for words a[j] and the true root omega the output words are  out[i] = sum_j a[j] omega^(i j) mod r  -- no encoding or decoding
is needed to state an expectation.  Each family returns its input together with its transform in closed form, from Python integers alone:
tests/test_ntt_cases_host.py pins the closed forms to an O(N^2) sum and to the oracle's best_fft before a GPU sees them."""
import collections
import concurrent.futures
import functools
import hashlib
import os
import threading

import numpy as np

from oracle import bn254 as O

R = O.R_MOD


def enc(x):
    """the Montgomery-256 word of the field value x"""
    return x % R * (1 << 256) % R


# ---- constants M -----------------------------------------------------------------------------------------------------------------------------
LOW_LIMBS_FULL = ((R >> 232) << 232) - 1          # the raw word whose eight low 29-bit limbs are all ones
assert LOW_LIMBS_FULL < R and all((LOW_LIMBS_FULL >> (29 * i)) & 0x1FFFFFFF == 0x1FFFFFFF for i in range(8))
SEEDED = int.from_bytes(hashlib.sha256(b"ntt-cases-seeded-constant").digest(), "big") % R
CONSTANTS = collections.OrderedDict([
    ("enc0", enc(0)), ("enc1", enc(1)), ("enc_r_minus_1", enc(R - 1)),       # the encodings of 0, 1 and r - 1
    ("raw_r_minus_1", R - 1),                                              # the largest raw input word
    ("raw_low_limbs_full", LOW_LIMBS_FULL),
    ("raw1", 1),
    ("seeded", SEEDED),
])
assert all(0 <= m < R for m in CONSTANTS.values()) and CONSTANTS["enc0"] == 0

# ---- sizes: log2 N, with the pass structure (ntt.hip build_plan) each one exists for -----------------------------------------------------------
SIZES = collections.OrderedDict([
    (0, "k_ntt_tiny"), (1, "k_ntt_tiny"), (2, "k_ntt_tiny"),
    (3, "one pass, rounds of 2 + 1 stages"),
    (4, "one pass, 2 + 2"),
    (5, "one pass, 2 + 2 + 1"),
    (9, "one pass, 512-element tile"),
    (10, "two passes 5 + 5, J = 32: the first multi-pass split"),
    (11, "two passes 6 + 5"),
    (18, "two passes 9 + 9, J = 2"),
    (19, "three passes 7 + 6 + 6"),
])
DFT_SIZES = list(range(7))                         # where the O(N^2) sum is affordable


# ---- words <-> numpy ---------------------------------------------------------------------------------------------------------------------------
def words(values):
    """ints below 2^256 -> (n, 4) uint64, the memory of &[Fr]"""
    buf = b"".join(v.to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def word(v):
    return words([v])[0]


def ints(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def omega(L):
    return O.omega_for(L)


@functools.lru_cache(maxsize=2)
def _powers(L):
    w, out, cur = omega(L), [], 1
    for _ in range(1 << L):
        out.append(cur)
        cur = cur * w % R
    assert cur == 1
    return out


@functools.lru_cache(maxsize=2)
def _int_table(L, m):
    if m == 1:
        return _powers(L)
    if R - m in (1, enc(1)):                                                # -x = r - x, x != 0: a subtraction instead of a product
        return [R - x for x in _int_table(L, R - m)]
    return [m * p % R for p in _powers(L)]


@functools.lru_cache(maxsize=16)                                            # the tables of the two large sizes stay: 170 MB
def _table_locked(L, m):
    t = np.zeros((1 << L, 4), dtype=np.uint64) if m == 0 else words(_int_table(L, m))
    t.setflags(write=False)
    return t


_table_lock = threading.Lock()


def _table(L, m):
    """(N, 4) words of m omega^i, i < N; made once, also when for_each asks from several threads"""
    with _table_lock:
        return _table_locked(L, m)


# ---- families ----------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "family param mname")


def case_id(c):
    return f"{c.family}{'' if c.param is None else c.param}-{c.mname}"


def _spike(N, at, value):
    out = np.zeros((N, 4), dtype=np.uint64)
    out[at] = word(value % R)
    return out


def _zero(L, m, _):
    N = 1 << L
    return np.zeros((N, 4), dtype=np.uint64), np.zeros((N, 4), dtype=np.uint64)


def _constant(L, m, _):
    N = 1 << L
    return np.tile(word(m), (N, 1)), _spike(N, 0, N * m)                    # sum_j omega^(i j) = N at i = 0, 0 elsewhere


def _alternating(L, m, _):
    N = 1 << L
    a = np.tile(word(m), (N, 1))
    a[1::2] = word(-m % R)                                                  # (-1)^j = omega^(j N/2): the geometric family at k = N/2
    return a, _spike(N, N // 2, N * m)


def _half(L, m, _):
    N = 1 << L
    a = np.empty((N, 4), dtype=np.uint64)
    a[0::2] = word(m)
    a[1::2] = word(R - m if m else 0)                                       # r - M as a word of its own (r itself is not a canonical word)
    return a, _spike(N, N // 2, N * m)


def _geometric(L, m, k):
    N = 1 << L
    j = np.arange(N, dtype=np.int64)
    return _table(L, m)[(-(j * k)) % N], _spike(N, k, N * m)                # sum_j omega^(j (i - k)) = N at i = k


def _delta(L, m, j):
    N = 1 << L
    i = np.arange(N, dtype=np.int64)
    return _spike(N, j, m), _table(L, m)[(i * j) % N]                       # out[i] = M omega^(i j)


_FAMILIES = {"zero": _zero, "constant": _constant, "alternating": _alternating, "half": _half, "geometric": _geometric, "delta": _delta}


def geometric_ks(L):
    N = 1 << L
    return sorted({k for k in (1, N - 1) + ((1023, 1024) if N > 1024 else ()) if 0 <= k < N})


def delta_js(L):
    N = 1 << L
    return sorted({j for j in (0, 1, N // 2, N - 1) if 0 <= j < N})


def cases(L):
    """every member of every family at size 2^L: `zero` once, the others once per constant"""
    out = [Case("zero", None, "enc0")]
    for mname in CONSTANTS:
        out.append(Case("constant", None, mname))
        if L >= 1:
            out.append(Case("alternating", None, mname))
            out.append(Case("half", None, mname))
        out += [Case("geometric", k, mname) for k in geometric_ks(L)]
        out += [Case("delta", j, mname) for j in delta_js(L)]
    return out


def vector(L, c):
    """(input, expected transform) of one case: two fresh (2^L, 4) uint64 arrays"""
    a, e = _FAMILIES[c.family](L, CONSTANTS[c.mname], c.param)
    return np.ascontiguousarray(a), np.ascontiguousarray(e)


# ---- the oracle's transform of many vectors ----------------------------------------------------------------------------------------------------
def for_each(fn, count, L):
    """[fn(i) for i < count]; the oracle's transforms of independent vectors run side by side at the large sizes (ctypes drops the GIL)"""
    if L < 12:
        return [fn(i) for i in range(count)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        return list(pool.map(fn, range(count)))

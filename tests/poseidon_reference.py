"""Poseidon over BN254's Fr (T = 3, RATE = 2, R_F = 8, R_P = 57) restated with Python integers from the Poseidon paper and the
normative text of include/zkhip.h ("Poseidon"): Grain LFSR constants, the plain permutation, the sponge, the Merkle tree and the
transcript.  Independent of the library's code: it is what tests/test_poseidon_host.py and the GPU tests compare against.
About 1 ms per permutation."""
from __future__ import annotations

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
T, RATE, R_F, R_P = 3, 2, 8, 57
ROUNDS = R_F + R_P


class Grain:
    def __init__(self):
        bits = []
        for value, width in ((1, 2), (0, 4), (254, 12), (T, 12), (R_F, 10), (R_P, 10)):
            bits += [(value >> (width - 1 - i)) & 1 for i in range(width)]
        bits += [1] * 30
        assert len(bits) == 80
        self.state = bits
        for _ in range(160):
            self._step()

    def _step(self) -> int:
        s = self.state
        new = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0]
        self.state = s[1:] + [new]
        return new

    def bit(self) -> int:
        while True:
            first, second = self._step(), self._step()
            if first:
                return second

    def integer(self, nbits: int = 254) -> int:
        v = 0
        for _ in range(nbits):
            v = (v << 1) | self.bit()
        return v


def _constants():
    g = Grain()
    rc = []
    while len(rc) < ROUNDS * T:
        v = g.integer()
        if v < R:
            rc.append(v)
    xy = [g.integer() % R for _ in range(2 * T)]
    xs, ys = xy[:T], xy[T:]
    mds = [[pow(xs[i] + ys[j], R - 2, R) for j in range(T)] for i in range(T)]
    return [rc[r * T:(r + 1) * T] for r in range(ROUNDS)], mds


ROUND_CONSTANTS, MDS = _constants()


def permute(state):
    s = list(state)
    for r in range(ROUNDS):
        s = [(s[i] + ROUND_CONSTANTS[r][i]) % R for i in range(T)]
        if r < R_F // 2 or r >= R_F // 2 + R_P:
            s = [pow(x, 5, R) for x in s]
        else:
            s[0] = pow(s[0], 5, R)
        s = [sum(MDS[i][j] * s[j] for j in range(T)) % R for i in range(T)]
    return s


class Sponge:
    def __init__(self):
        self.state = [1 << 64, 0, 0]
        self.buf = []

    def update(self, *values):
        self.buf += [v % R for v in values]

    def squeeze(self) -> int:
        buf, self.buf = self.buf, []
        while len(buf) >= RATE:
            chunk, buf = buf[:RATE], buf[RATE:]
            for i, v in enumerate(chunk):
                self.state[1 + i] = (self.state[1 + i] + v) % R
            self.state = permute(self.state)
        for i, v in enumerate(buf + [1]):
            self.state[1 + i] = (self.state[1 + i] + v) % R
        self.state = permute(self.state)
        return self.state[1]


def hash(*values) -> int:
    s = Sponge()
    s.update(*values)
    return s.squeeze()


def merkle_levels(leaves):
    """[level 0 = the leaves, level 1, ..., [root]]; len(leaves) a power of two"""
    n = len(leaves)
    assert n >= 1 and n & (n - 1) == 0
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        prev = levels[-1]
        levels.append([hash(prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
    return levels


class Transcript:
    """snark-verifier's PoseidonTranscript with the native loader: no prefix bytes, points as (x mod r, y mod r)"""

    def __init__(self):
        self.sponge = Sponge()

    def common_scalar(self, s: int):
        self.sponge.update(s)

    def common_point(self, x: int, y: int):
        assert (x, y) != (0, 0)
        self.sponge.update(x % R, y % R)

    def squeeze(self) -> int:
        return self.sponge.squeeze()

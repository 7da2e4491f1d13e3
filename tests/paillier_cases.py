"""The moduli and edge operands the Paillier tests share (a helper module: no tests, no fixtures).  Everything is a Python integer; the oracle of
every test is Python's own `pow`, `*` and `%`."""
import random

_rng = random.Random(0x5041494C)
N_SMALL = 3                                                     # the smallest modulus the C ABI takes: n^2 = 9
N_176 = _rng.getrandbits(176) | (1 << 175) | 1                  # the reference's ENC_BIT_LEN: n^2 has 351 or 352 bits
N_TOP = (1 << 192) - 237                                        # n^2 just under 2^384: the 13th carry word of a product is used
N_LOW1 = (_rng.getrandbits(150) << 32) | (1 << 181) | 1         # n = 2^32 k + 1: the low limb of n^2 is 1
MODULI = {"n3": N_SMALL, "n176": N_176, "ntop": N_TOP, "nlow1": N_LOW1}
FULL = (1 << 384) - 1                                           # the largest unreduced input


def edge_operands(n):
    N = n * n
    return [0, 1, N - 1, N, FULL]


def rng(tag):
    return random.Random(f"paillier-{tag}")

"""The Paillier side of the aggregator's inputs (include/zkhip.h, "Paillier tally"): `paillier_enc_native` / `paillier_add_native` [DEP
paillier_chip] as the reference's `generate_wrapper_circuit_input` uses them (/root/reference/aggregator/src/utils.rs:298-341).

`enc_native` and `add_native` are the host forms on Python integers, in the reference's names.  `mul_device`, `encrypt_many_device` and
`tally_device` run the kernels over device tensors of canonical integers, six little-endian 64-bit words each; `tally_device` returns every
round's `prev_vote` and the final tally of a batch of ballots from one call, beside `poseidon.IndexedMerkleTree.insert_batch`.

The kernels' arithmetic is Montgomery's and needs an odd n, which the C ABI insists on.  The reference's own generators draw n as a random
176-bit number, even half the time: for an even n -- and only then -- this layer computes the same tensors on the host with integers.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import _lib
from .tensors import from_words, raw_tensor, stream_of, to_words

WORDS = _lib.ZKHIP_PAILLIER_WORDS
MAX_N_BITS = _lib.ZKHIP_PAILLIER_MAX_N_BITS


def enc_native(n: int, g: int, m: int, r: int) -> int:
    """`paillier_enc_native`: g^m r^n mod n^2"""
    n2 = n * n
    return pow(g, m, n2) * pow(r, n, n2) % n2


def add_native(n: int, a: int, b: int) -> int:
    """`paillier_add_native`: the ciphertext of the sum of two votes, a b mod n^2"""
    return a * b % (n * n)


def encode(values, device=None):
    """integers below 2^384, nested to any depth -> a [..., 6] int64 tensor on the current device (or `device`)"""
    return raw_tensor(values, WORDS, device)


def encode_exponents(values, device=None):
    """votes below 2^256 (`fe_to_biguint` of an Fr) -> [..., 4] int64"""
    return raw_tensor(values, 4, device)


def encode_randomness(values, device=None):
    """the r of every encryption, below 2^192 -> [..., 3] int64"""
    return raw_tensor(values, 3, device)


def decode(tensor):
    """a [..., w] int64 tensor of little-endian words -> integers, nested as the leading dimensions are"""
    return from_words(tensor)


def _n_words(n: int) -> np.ndarray:
    n = int(n)
    if not 0 <= n < 1 << MAX_N_BITS:
        raise ValueError(f"n must be below 2^{MAX_N_BITS}")
    return to_words(n, 3)


def _on_host(n: int) -> bool:
    """an even n: the kernels cannot run it (Montgomery), the host computes the same tensors"""
    if int(n) < 2:
        raise ValueError("n must be at least 2")
    return int(n) % 2 == 0


def _want(t, words: int, who: str, dims=None):
    import torch

    if t.dtype != torch.int64 or t.dim() < 1 or t.shape[-1] != words or (dims is not None and t.dim() != dims):
        raise ValueError(f"{who}: an int64 tensor whose last dimension is {words}")
    return t.contiguous()


def _device_call(who: str, *tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{who}: an odd n runs on the device and takes device tensors (there is no CPU fallback for it)")


def mul_device(n: int, a, b, out=None, stream=None):
    """a, b: [..., 6] tensors of ciphertexts -> a[i] b[i] mod n^2, `add_native` element by element; `out` may be a or b"""
    import torch

    a, b = _want(a, WORDS, "mul_device"), _want(b, WORDS, "mul_device")
    if a.shape != b.shape:
        raise ValueError("mul_device: a and b differ in shape")
    if out is None:
        out = torch.empty_like(a)
    elif out.shape != a.shape or out.dtype != torch.int64 or not out.is_contiguous():
        raise ValueError("mul_device: out must be a contiguous tensor of a's shape")
    if _on_host(n):
        flat_a, flat_b = decode(a.reshape(-1, WORDS)), decode(b.reshape(-1, WORDS))
        out.copy_(raw_tensor([add_native(n, x, y) for x, y in zip(flat_a, flat_b)], WORDS, out.device).reshape(out.shape))
        return out
    _device_call("mul_device", a, b, out)
    nw = _n_words(n)
    _lib.check(_lib.load().zkhip_paillier_mul_device(nw.ctypes.data, a.data_ptr(), b.data_ptr(), a.numel() // WORDS, out.data_ptr(), stream_of(stream)))
    return out


def encrypt_many_device(n: int, g: int, m, r, stream=None):
    """m: [count, 4] votes, r: [count, 3] randomness (tensors, or lists of integers) -> [count, 6]: enc_native(n, g, m[i], r[i]) for every i"""
    import torch

    if isinstance(m, (list, tuple)):
        m = encode_exponents(list(m), r.device if hasattr(r, "device") else None)
    if isinstance(r, (list, tuple)):
        r = encode_randomness(list(r), m.device)
    m, r = _want(m, 4, "encrypt_many_device", 2), _want(r, 3, "encrypt_many_device", 2)
    if m.shape[0] != r.shape[0]:
        raise ValueError("encrypt_many_device: as many r as m")
    g = int(g)
    if not 0 <= g < 1 << 384:
        raise ValueError("encrypt_many_device: g must be below 2^384")
    if _on_host(n):
        return raw_tensor([enc_native(n, g, x, y) for x, y in zip(decode(m), decode(r))], WORDS, m.device).reshape(m.shape[0], WORDS)
    _device_call("encrypt_many_device", m, r)
    out = torch.empty((m.shape[0], WORDS), dtype=torch.int64, device=m.device)
    nw, gw = _n_words(n), to_words(g, WORDS)
    _lib.check(_lib.load().zkhip_paillier_encrypt_device(nw.ctypes.data, gw.ctypes.data, m.data_ptr(), r.data_ptr(), m.shape[0], out.data_ptr(), stream_of(stream)))
    return out


class Tally:
    """the running sums of one `tally_device`: `running` is the [B + 1, C, 6] device tensor, row i the `prev_vote` of round i, the last row the
    tally; `ballots` the [B, C, 6] tensor it was computed from"""

    def __init__(self, n: int, ballots, running):
        self.n, self.ballots, self.running = int(n), ballots, running
        self.rounds, self.cols = ballots.shape[0], ballots.shape[1]

    def total(self) -> List[int]:
        """the final tally, one ciphertext per column"""
        return decode(self.running[-1])

    def round(self, i: int) -> Tuple[List[int], List[int]]:
        """(incoming_vote, prev_vote) of round i as integer lists, in the order `StateTransitionInput::new` takes them; incoming_vote is taken
        mod n^2, as every later use of it is"""
        if not 0 <= i < self.rounds:
            raise IndexError("round: no such ballot")
        n2 = self.n * self.n
        return [v % n2 for v in decode(self.ballots[i])], decode(self.running[i])


def tally_device(n: int, ballots, init=None, stream=None) -> Tally:
    """ballots: a [B, C, 6] tensor of ciphertexts, ballot-major; init: [C, 6], the prev_vote of round 0 (None: 1) -> a Tally; no host wait"""
    import torch

    ballots = _want(ballots, WORDS, "tally_device", 3)
    B, C = ballots.shape[0], ballots.shape[1]
    if C == 0:
        raise ValueError("tally_device: a ballot has at least one column")
    if init is not None:
        init = _want(init, WORDS, "tally_device", 2)
        if init.shape[0] != C or init.device != ballots.device:
            raise ValueError("tally_device: init is [C, 6] on the ballots' device")
    if _on_host(n):
        n2 = int(n) * int(n)
        rows = [[v % n2 for v in decode(init)] if init is not None else [1 % n2] * C]
        for ballot in decode(ballots):
            rows.append([add_native(n, acc, v) for acc, v in zip(rows[-1], ballot)])
        return Tally(n, ballots, raw_tensor(rows, WORDS, ballots.device))
    _device_call("tally_device", ballots, init)
    running = torch.empty((B + 1, C, WORDS), dtype=torch.int64, device=ballots.device)
    nw = _n_words(n)
    _lib.check(_lib.load().zkhip_paillier_tally_device(nw.ctypes.data, ballots.data_ptr() if B else None, B, C, init.data_ptr() if init is not None else None,
                                                       running.data_ptr(), stream_of(stream)))
    return Tally(n, ballots, running)

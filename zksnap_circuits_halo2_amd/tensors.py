"""Python integers <-> the int64 tensors the library reads: the one place that makes the conversion.

`to_words` / `from_words` / `raw_tensor` carry canonical integers as little-endian 64-bit words (plume.py, paillier.py); the `fr_*` functions
carry Fr elements as Montgomery words through `fields.fr_encode` / `fields.fr_decode` (the prover, Poseidon, the witness checks).  torch is
imported inside the functions, so the module and the host-only calls built on it work where there is no torch and no device; every
function that takes `device` also takes "cpu".
"""
from __future__ import annotations

import functools

import numpy as np

from .fields import fr_decode, fr_encode


def stream_of(stream) -> int:
    return int(stream) if stream is not None else 0


def device_of(device=None):
    """None: the current CUDA device"""
    import torch

    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


# ---- canonical integers as little-endian words ---------------------------------------------------------------------------------------------------
def _shape_of(values):
    shape = []
    while isinstance(values, (list, tuple)):
        shape.append(len(values))
        if not values:
            break
        values = values[0]
    return shape


def _flat(values):
    if isinstance(values, (list, tuple)):
        for v in values:
            yield from _flat(v)
    else:
        yield int(values)


def _host(a) -> np.ndarray:
    """a tensor or an array -> a contiguous uint64 view of its words on the host"""
    a = a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def to_words(values, words: int) -> np.ndarray:
    """integers, nested to any depth -> a [..., words] uint64 array of little-endian words"""
    shape = _shape_of(values)
    flat = list(_flat(values))
    if int(np.prod(shape, dtype=np.int64)) != len(flat):
        raise ValueError("a ragged list of integers")
    for v in flat:
        if not 0 <= v < 1 << (64 * words):
            raise ValueError(f"an integer outside [0, 2^{64 * words})")
    raw = b"".join(v.to_bytes(8 * words, "little") for v in flat)
    return np.frombuffer(raw, dtype=np.uint64).reshape(shape + [words]).copy()


def from_words(a):
    """a [..., w] tensor or array of little-endian words -> integers, nested as the leading dimensions are"""
    a = _host(a)
    words = a.shape[-1]
    raw = a.tobytes()
    flat = [int.from_bytes(raw[8 * words * i:8 * words * (i + 1)], "little") for i in range(a.size // words)]

    def nest(shape, at):
        if not shape:
            return flat[at], at + 1
        out = []
        for _ in range(shape[0]):
            v, at = nest(shape[1:], at)
            out.append(v)
        return out, at

    return nest(list(a.shape[:-1]), 0)[0]


def raw_tensor(values, words: int, device=None):
    """`to_words` as an int64 tensor on the current device (or `device`)"""
    import torch

    return torch.from_numpy(to_words(values, words).view(np.int64)).to(device_of(device))


# ---- Fr elements as Montgomery words -------------------------------------------------------------------------------------------------------------
def fr_words(values, device=None):
    """integers (taken mod r) -> an [n, 4] int64 tensor of Montgomery words"""
    import torch

    return torch.from_numpy(fr_encode(values).view(np.int64)).to(device_of(device))


def fr_ints(a):
    """a tensor or array of Montgomery words, 4 to an element -> the canonical integers, flat"""
    return fr_decode(_host(a).reshape(-1, 4))


def fr_empty(*shape, device=None):
    import torch

    return torch.empty(shape + (4,), dtype=torch.int64, device=device_of(device))


def fr_random(m, device=None):
    """uniformly random canonical word patterns = random field elements"""
    import torch

    device = device_of(device)
    a = torch.randint(-(1 << 63), (1 << 63) - 1, (m, 4), dtype=torch.int64, device=device)
    a[:, 3] = torch.randint(0, 1 << 61, (m,), dtype=torch.int64, device=device)
    return a


@functools.lru_cache(maxsize=None)
def _to_mont():
    from . import evaluation as E

    return E.to_mont_program()


def fr_from_small(v, k, stream=None):
    """an int64 device tensor of 2^k small non-negative integers -> their Montgomery words, on v's device; no host wait.  The words are
    staged on torch's current stream and multiplied on `stream` (None: the default stream): pass the current stream when it is a side stream"""
    import torch

    a = torch.zeros((v.shape[0], 4), dtype=torch.int64, device=v.device)
    a[:, 0] = v
    out = torch.empty_like(a)
    _to_mont().run_device([a.data_ptr()], k, out.data_ptr(), stream=stream_of(stream))
    return out

"""Poseidon over Fr with T = 3, RATE = 2, R_F = 8, R_P = 57 (include/zkhip.h, "Poseidon"): the hash of the reference's membership Merkle trees
(`MerkleTree`, /root/reference/voter/src/merkletree/native.rs) and of its `gen_snark` transcript (transcript.PoseidonWrite).

`permute` and `hash` are the library's host form (Python integers in and out, no GPU touched); `hash_many_device` and `MerkleTree` run the
kernels over device tensors of Montgomery limbs.  Nothing here computes: there is no CPU fallback for the device calls.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .fields import fr_decode, fr_encode

MAX_WIDTH = _lib.ZKHIP_POSEIDON_MAX_WIDTH
SUBTREE = _lib.ZKHIP_POSEIDON_SUBTREE      # elements of a level one workgroup of the tree kernel folds: sizes around it take different paths


def _stream_of(stream) -> int:
    return int(stream) if stream is not None else 0


def constants() -> Tuple[List[List[int]], List[List[int]]]:
    """(65 x 3 round constants, the 3 x 3 matrix) as the library's Grain made them, canonical integers"""
    out = np.zeros((204, 4), dtype=np.uint64)
    _lib.check(_lib.load().zkhip_poseidon_constants(out.ctypes.data))
    v = [int.from_bytes(row.tobytes(), "little") for row in out]
    return [v[3 * r:3 * r + 3] for r in range(65)], [v[195 + 3 * i:198 + 3 * i] for i in range(3)]


def permute(states: Sequence[Sequence[int]]) -> List[List[int]]:
    """the permutation of every (word 0, word 1, word 2) given"""
    flat = [int(x) for s in states for x in s]
    if len(flat) != 3 * len(states):
        raise ValueError("permute: a state is three field elements")
    w = fr_encode(flat)
    _lib.check(_lib.load().zkhip_poseidon_permute(w.ctypes.data, len(states)))
    out = fr_decode(w)
    return [out[3 * i:3 * i + 3] for i in range(len(states))]


def hash(values: Sequence[int]) -> int:
    """a fresh sponge over the values: `hash.update(values); hash.squeeze_and_reset()`"""
    w = fr_encode([int(v) for v in values])
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.load().zkhip_poseidon_hash(w.ctypes.data if len(w) else None, len(w), out.ctypes.data))
    return fr_decode(out.reshape(1, 4))[0]


def hash_many_device(messages, out=None, stream=None):
    """messages: an (n, width, 4) int64 device tensor of Montgomery limbs, width in 1 .. MAX_WIDTH -> (n, 4): the hash of every row, one launch"""
    import torch

    if messages.dim() != 3 or messages.shape[2] != 4 or not messages.is_cuda or messages.dtype != torch.int64:
        raise ValueError("hash_many_device: an (n, width, 4) int64 tensor on the device")
    messages = messages.contiguous()
    n, width = messages.shape[0], messages.shape[1]
    if out is None:
        out = torch.empty((n, 4), dtype=torch.int64, device=messages.device)
    _lib.check(_lib.load().zkhip_poseidon_hash_many_device(messages.data_ptr(), n, width, out.data_ptr(), _stream_of(stream)))
    return out


def merkle_device(leaves, stream=None):
    """leaves: (n, 4) int64 device tensor, n a power of two -> the (n - 1, 4) inner nodes, level 1 first, the root last; no host wait"""
    import torch

    if leaves.dim() != 2 or leaves.shape[1] != 4 or not leaves.is_cuda or leaves.dtype != torch.int64:
        raise ValueError("merkle_device: an (n, 4) int64 tensor on the device")
    leaves = leaves.contiguous()
    n = leaves.shape[0]
    nodes = torch.empty((max(n - 1, 0), 4), dtype=torch.int64, device=leaves.device)
    _lib.check(_lib.load().zkhip_poseidon_merkle_device(leaves.data_ptr(), n, nodes.data_ptr() if n > 1 else None, _stream_of(stream)))
    return nodes


class MerkleTree:
    """`MerkleTree::new(hash, leaves)` over a device tensor of leaves: every level stays in HBM; `get_root`, `get_proof` and `verify_proof`
    move a handful of elements to the host and return Python integers, as the reference returns field elements."""

    def __init__(self, leaves, stream=None):
        self.n = leaves.shape[0]
        self.leaves = leaves.contiguous()
        self.nodes = merkle_device(self.leaves, stream)          # ValueError / ZkhipError on anything but a power of two
        self.depth = self.n.bit_length() - 1

    def level(self, L: int):
        """level L as a device tensor: 0 the leaves, `depth` the root"""
        if L == 0:
            return self.leaves
        start = self.n - (self.n >> (L - 1))
        return self.nodes[start:start + (self.n >> L)]

    def get_root(self) -> int:
        top = self.nodes[-1:] if self.n > 1 else self.leaves[:1]
        return fr_decode(top.cpu().numpy().view(np.uint64))[0]

    def get_proof(self, index: int) -> Tuple[List[int], List[int]]:
        """(siblings from the leaf's level up, 1 where the node on the path is a left child else 0)"""
        if not 0 <= index < self.n:
            raise IndexError("get_proof: no such leaf")
        import torch

        rows, helper = [], []
        for L in range(self.depth):
            rows.append(self.level(L)[index ^ 1])
            helper.append(1 if index % 2 == 0 else 0)
            index //= 2
        if not rows:
            return [], []
        return fr_decode(torch.stack(rows).cpu().numpy().view(np.uint64)), helper

    @staticmethod
    def verify_proof(leaf: int, index: int, root: int, proof: Sequence[int]) -> bool:
        """the reference's `verify_proof`: the path recomputed with the library's host hash"""
        acc = int(leaf)
        for sibling in proof:
            acc = hash([acc, sibling]) if index % 2 == 0 else hash([sibling, acc])
            index //= 2
        return acc == int(root)

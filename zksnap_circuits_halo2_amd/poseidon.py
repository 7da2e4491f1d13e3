"""Poseidon over Fr with T = 3, RATE = 2, R_F = 8, R_P = 57 (include/zkhip.h, "Poseidon"): the hash of the reference's membership Merkle trees
(`MerkleTree`, /root/reference/voter/src/merkletree/native.rs) and of its `gen_snark` transcript (transcript.PoseidonWrite).

`permute` and `hash` are the library's host form (Python integers in and out, no GPU touched); `hash_many_device` and `MerkleTree` run the
kernels over device tensors of Montgomery limbs.  `IndexedMerkleTree` is the nullifier tree of the state-transition circuit
(`generate_state_transition_circuit_inputs`, /root/reference/aggregator/src/utils.rs): a whole batch of insertions and their witnesses in one
device call; `imt_link` is its host half alone.  Nothing here computes: there is no CPU fallback for the device calls.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .fields import fr_decode, fr_encode
from .tensors import device_of, fr_empty, fr_ints, fr_words, stream_of

MAX_WIDTH = _lib.ZKHIP_POSEIDON_MAX_WIDTH
SUBTREE = _lib.ZKHIP_POSEIDON_SUBTREE      # elements of a level one workgroup of the tree kernel folds: sizes around it take different paths


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
    _lib.check(_lib.load().zkhip_poseidon_hash_many_device(messages.data_ptr(), n, width, out.data_ptr(), stream_of(stream)))
    return out


def compress_nullifier(point: Tuple[int, int]) -> List[int]:
    """`compress_native_nullifier` (/root/reference/aggregator/src/utils.rs:355) of a secp256k1 affine point (x, y): the tag -- 2 for an even
    y, 3 for an odd one -- then the 11-, 11- and 10-byte little-endian chunks of x's 32 bytes.  Host; integers in and out."""
    x, y = int(point[0]), int(point[1])
    if not (0 <= x < 1 << 256 and 0 <= y < 1 << 256):
        raise ValueError("compress_nullifier: a coordinate is 32 bytes")
    raw = x.to_bytes(32, "little")
    return [2 + (y & 1)] + [int.from_bytes(raw[at:at + 11], "little") for at in (0, 11, 22)]


LAYOUT_NULLIFIER, LAYOUT_MEMBER = 0, 1


def _is_point_tensor(points) -> bool:
    return hasattr(points, "data_ptr") and hasattr(points, "is_cuda")


def hash_points_device(points, layout: int, stream=None):
    """points: an (n, 8) int64 device tensor of secp256k1 points as plume.py holds them (canonical x then y, four little-endian words each; any
    256-bit values) -> (n, 4): the hash of every point's packed message, LAYOUT_NULLIFIER (`compress_nullifier`) or LAYOUT_MEMBER
    (`pack_member`); the packing runs in the kernel, one launch, no host round trip"""
    import torch

    if points.dim() != 2 or points.shape[1] != 8 or not points.is_cuda or points.dtype != torch.int64:
        raise ValueError("hash_points_device: an (n, 8) int64 tensor on the device (there is no CPU fallback)")
    points = points.contiguous()
    n = points.shape[0]
    out = torch.empty((n, 4), dtype=torch.int64, device=points.device)
    _lib.check(_lib.load().zkhip_poseidon_hash_points_device(points.data_ptr() if n else None, n, int(layout), out.data_ptr() if n else None, stream_of(stream)))
    return out


def nullifier_values(points, stream=None):
    """secp256k1 affine points -- a sequence of (x, y) integers, or an (n, 8) int64 device tensor (`plume.sign_many_device(..).nullifier`) -> the
    (n, 4) device tensor of the values the state-transition circuit inserts into the nullifier tree: the width-4 hash of every compressed
    point, one launch.  A tensor is packed on the device.  `IndexedMerkleTree.insert_batch` takes its host copy."""
    if _is_point_tensor(points):
        return hash_points_device(points, LAYOUT_NULLIFIER, stream)
    return hash_many_device(fr_words([v for P in points for v in compress_nullifier(P)]).reshape(len(points), 4, 4), stream=stream)


def pack_member(point: Tuple[int, int]) -> List[int]:
    """the six values behind a leaf of the members tree (reference aggregator/src/utils.rs:224-254): the 11-, 11- and 10-byte little-endian
    chunks of pk.x's 32 bytes, then those of pk.y's.  Host; integers in and out."""
    out = []
    for v in (int(point[0]), int(point[1])):
        if not 0 <= v < 1 << 256:
            raise ValueError("pack_member: a coordinate is 32 bytes")
        raw = v.to_bytes(32, "little")
        out += [int.from_bytes(raw[at:at + 11], "little") for at in (0, 11, 22)]
    return out


def member_leaves(points, stream=None):
    """secp256k1 public keys -- a sequence of (x, y) integers, or an (n, 8) int64 device tensor (`plume.sign_many_device(..).pk`) -> the (n, 4)
    device tensor of the members tree's leaves: the width-6 hash of every packed key, one launch.  A tensor is packed on the device."""
    if _is_point_tensor(points):
        return hash_points_device(points, LAYOUT_MEMBER, stream)
    return hash_many_device(fr_words([v for P in points for v in pack_member(P)]).reshape(len(points), 6, 4), stream=stream)


def merkle_device(leaves, stream=None):
    """leaves: (n, 4) int64 device tensor, n a power of two -> the (n - 1, 4) inner nodes, level 1 first, the root last; no host wait"""
    import torch

    if leaves.dim() != 2 or leaves.shape[1] != 4 or not leaves.is_cuda or leaves.dtype != torch.int64:
        raise ValueError("merkle_device: an (n, 4) int64 tensor on the device")
    leaves = leaves.contiguous()
    n = leaves.shape[0]
    nodes = torch.empty((max(n - 1, 0), 4), dtype=torch.int64, device=leaves.device)
    _lib.check(_lib.load().zkhip_poseidon_merkle_device(leaves.data_ptr(), n, nodes.data_ptr() if n > 1 else None, stream_of(stream)))
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
        return fr_ints(top)[0]

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
        return fr_ints(torch.stack(rows)), helper

    @staticmethod
    def verify_proof(leaf: int, index: int, root: int, proof: Sequence[int]) -> bool:
        """the reference's `verify_proof`: the path recomputed with the library's host hash"""
        acc = int(leaf)
        for sibling in proof:
            acc = hash([acc, sibling]) if index % 2 == 0 else hash([sibling, acc])
            index //= 2
        return acc == int(root)


IMT_MAX_DEPTH = _lib.ZKHIP_IMT_MAX_DEPTH


def _helper(index: int, depth: int) -> List[int]:
    return [1 - ((index >> L) & 1) for L in range(depth)]


def imt_link(used_vals: Sequence[int], new_vals: Sequence[int]) -> List[int]:
    """the low leaf of every new value (include/zkhip.h, zkhip_imt_link): host only, no GPU touched.  used_vals: the vals of leaves 0, 1, ..
    in index order, leaf 0 the head with val 0 ([] stands for the empty tree).  ZkhipError with `.index` on a refusal."""
    used, new = fr_encode([int(v) for v in used_vals]), fr_encode([int(v) for v in new_vals])
    low = np.zeros(max(len(new), 1), dtype=np.uint32)
    bad = _lib.C.c_size_t(0)
    rc = _lib.load().zkhip_imt_link(used.ctypes.data if len(used) else None, len(used), new.ctypes.data if len(new) else None, len(new), low.ctypes.data,
                                    _lib.C.byref(bad))
    _check_index(rc, bad)
    return [int(x) for x in low[:len(new)]]


def _check_index(rc: int, bad) -> None:
    if rc != 0:
        err = _lib.ZkhipError(rc, _lib.load().zkhip_last_error().decode(errors="replace"))
        err.index = None if bad.value == _lib.C.c_size_t(-1).value else int(bad.value)      # the first refused value of the batch
        raise err


class ImtBatch:
    """the witnesses of one `insert_batch`, device tensors of Montgomery limbs: `roots` (n + 1, 4), `low_leaves` and `new_leaves` (n, 3, 4),
    `low_indices` (n,) int32, `low_proofs` and `new_proofs` (n, depth, 4); insertion i went to leaf `first_index + i`"""

    def __init__(self, n: int, depth: int, first_index: int, device):
        import torch

        self.n, self.depth, self.first_index = n, depth, first_index
        self.roots, self.low_leaves, self.new_leaves = (fr_empty(*shape, device=device) for shape in ((n + 1,), (n, 3), (n, 3)))
        self.low_indices = torch.empty((n,), dtype=torch.int32, device=device)
        self.low_proofs, self.new_proofs = fr_empty(n, depth, device=device), fr_empty(n, depth, device=device)

    def _c(self):
        return _lib.ImtWitness(*(t.data_ptr() for t in (self.roots, self.low_leaves, self.new_leaves, self.low_indices, self.low_proofs, self.new_proofs)))

    def round(self, i: int):
        """the arguments of `IndexedMerkleTreeInput::new` for insertion i, Python integers: (old_root, low_leaf, low_leaf_proof,
        low_leaf_proof_helper, new_root, new_leaf, new_leaf_index, new_leaf_proof, new_leaf_proof_helper, is_new_leaf_largest); a leaf is
        (val, next_val, next_idx)"""
        if not 0 <= i < self.n:
            raise IndexError("round: no such insertion")
        old_root, new_root = fr_ints(self.roots[i:i + 2])
        low_leaf, new_leaf = tuple(fr_ints(self.low_leaves[i])), tuple(fr_ints(self.new_leaves[i]))
        low, index = int(self.low_indices[i].item()), self.first_index + i
        return (old_root, low_leaf, fr_ints(self.low_proofs[i]), _helper(low, self.depth), new_root, new_leaf, index, fr_ints(self.new_proofs[i]),
                _helper(index, self.depth), 1 if new_leaf[1] == 0 else 0)


class IndexedMerkleTree:
    """the nullifier tree of the state-transition circuit (include/zkhip.h, "indexed Merkle tree"): leaves (val, next_val, next_idx), leaf 0 the
    head, values inserted at the first free index.  `insert_batch` computes the witnesses of a whole batch on the device; a single insertion is
    better served by the host hash."""

    def __init__(self, depth: int):
        h = _lib.C.c_void_p()
        _lib.check(_lib.load().zkhip_imt_create(int(depth), _lib.C.byref(h)))
        self._h, self.depth, self.n = h, int(depth), 1 << int(depth)

    def close(self) -> None:
        if self._h is not None:
            _lib.load().zkhip_imt_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def used(self) -> int:
        """used leaves, the head included: the index the next insertion goes to"""
        u = _lib.C.c_uint32()
        _lib.check(_lib.load().zkhip_imt_size(self._h, None, _lib.C.byref(u)))
        return u.value

    def insert_batch(self, values: Sequence[int], witness: bool = True, stream=None):
        """values in insertion order -- integers, or an (n, 4) uint64 array of Montgomery limbs -- -> an ImtBatch (None with witness=False: the
        tree alone is updated); no host wait"""
        if isinstance(values, np.ndarray) and values.dtype == np.uint64 and values.ndim == 2 and values.shape[1] == 4:
            w = np.ascontiguousarray(values)
        else:
            w = fr_encode([int(v) for v in values])
        first = self.used
        out = ImtBatch(len(w), self.depth, first, device_of()) if witness else None
        c = out._c() if out is not None else None
        bad = _lib.C.c_size_t(0)
        rc = _lib.load().zkhip_imt_insert(self._h, w.ctypes.data if len(w) else None, len(w), _lib.C.byref(c) if c is not None else None, _lib.C.byref(bad),
                                          stream_of(stream))
        _check_index(rc, bad)
        if out is not None and len(w) == 0:
            out.roots[0] = self.export()[1][-1]
        return out

    def get_root(self) -> int:
        out = np.zeros((1, 4), dtype=np.uint64)
        _lib.check(_lib.load().zkhip_imt_root(self._h, out.ctypes.data))
        return fr_decode(out)[0]

    def leaf(self, index: int) -> Tuple[int, int, int]:
        """(val, next_val, next_idx) of leaf `index`"""
        if not 0 <= index < self.n:
            raise IndexError("leaf: no such leaf")
        out = np.zeros((3, 4), dtype=np.uint64)
        _lib.check(_lib.load().zkhip_imt_leaf(self._h, index, out.ctypes.data))
        return tuple(fr_decode(out))

    def get_proof(self, index: int) -> Tuple[List[int], List[int]]:
        """(siblings from the leaf's level up, 1 where the node on the path is a left child else 0), as MerkleTree.get_proof"""
        if not 0 <= index < self.n:
            raise IndexError("get_proof: no such leaf")
        out = np.zeros((self.depth, 4), dtype=np.uint64)
        _lib.check(_lib.load().zkhip_imt_proof(self._h, index, out.ctypes.data))
        return fr_decode(out), _helper(index, self.depth)

    @staticmethod
    def verify_proof(leaf: Sequence[int], index: int, root: int, proof: Sequence[int]) -> bool:
        """the path from hash(val, next_val, next_idx) up, recomputed with the library's host hash"""
        return MerkleTree.verify_proof(hash(list(leaf)), index, root, proof)

    def export(self, stream=None):
        """(leaves (n, 4), inner nodes (n - 1, 4) in merkle_device's order, preimages (n, 3, 4)): device copies of the tree as it stands"""
        leaves, nodes, pre = fr_empty(self.n), fr_empty(self.n - 1), fr_empty(self.n, 3)
        _lib.check(_lib.load().zkhip_imt_export_device(self._h, leaves.data_ptr(), nodes.data_ptr(), pre.data_ptr(), stream_of(stream)))
        return leaves, nodes, pre

"""GPU (-m gpu): the indexed Merkle tree (include/zkhip.h, "indexed Merkle tree"; csrc/imt.hip) against the model written here: a sequential
insertion that scans for the low leaf and recomputes only the two paths, with the library's host hash (pinned by tests/test_poseidon_host.py)
or, for the reference's own depth-3 tree, with the big-integer restatement.  Every comparison is exact and over every element: all fields of
all witnesses of every batch, and after each batch the whole exported tree -- its preimages against the model's, its leaves against
`hash_many_device` of them and its inner nodes against `merkle_device` of the leaves, device against device (tests/test_gpu_poseidon.py pins
both).  Batch sizes 31, 32 and 33 put 62, 64 and 66 leaf updates around one wave, 200 makes several workgroups; ascending order makes every low
leaf the previous new leaf, descending order sends every step to leaf 0, and depth 1 makes the two leaves of an insertion siblings."""
import ctypes as C
import random

import pytest
import torch

import poseidon_reference as PR
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F, poseidon as PS
from zksnap_circuits_halo2_amd.tensors import fr_ints as ints

pytestmark = pytest.mark.gpu
R = O.R_MOD
EINVAL = -1


class Model:
    """one insertion at a time: scan for the low leaf, rewrite two leaves, rehash their two paths"""

    def __init__(self, depth, H):
        self.depth, self.H, self.used = depth, H, 1
        n = 1 << depth
        self.pre = [(0, 0, 0)] * n
        z = H([0, 0, 0])
        self.levels = [[z] * n]
        for L in range(depth):
            z = H([z, z])
            self.levels.append([z] * (n >> (L + 1)))

    def root(self):
        return self.levels[self.depth][0]

    def proof(self, i):
        return [self.levels[L][(i >> L) ^ 1] for L in range(self.depth)]

    def helper(self, i):
        return [1 - ((i >> L) & 1) for L in range(self.depth)]

    def _set(self, i, pre):
        self.pre[i] = pre
        self.levels[0][i] = self.H(list(pre))
        for L in range(self.depth):
            i >>= 1
            self.levels[L + 1][i] = self.H([self.levels[L][2 * i], self.levels[L][2 * i + 1]])

    def insert(self, v):
        """-> the arguments of IndexedMerkleTreeInput::new, in order"""
        j = self.used
        assert 0 < v < R and j < len(self.pre)
        low = max((i for i in range(j) if self.pre[i][0] < v), key=lambda i: self.pre[i][0])
        assert self.pre[low][1] == 0 or self.pre[low][1] > v
        old_root, low_leaf, low_proof = self.root(), self.pre[low], self.proof(low)
        self._set(low, (low_leaf[0], v, j))
        new_leaf, new_proof = (v, low_leaf[1], low_leaf[2]), self.proof(j)
        self._set(j, new_leaf)
        self.used += 1
        return (old_root, low_leaf, low_proof, self.helper(low), self.root(), new_leaf, j, new_proof, self.helper(j), 1 if new_leaf[1] == 0 else 0)

    def nodes(self):
        return [v for L in range(1, self.depth + 1) for v in self.levels[L]]


def host_hash(values):
    return PS.hash(values)


def ref_hash(values):
    return PR.hash(*values)


def witnesses(batch):
    """every insertion of a batch as `round(i)` words it, from whole-tensor copies"""
    d, n = batch.depth, batch.n
    roots, low, new = ints(batch.roots), ints(batch.low_leaves), ints(batch.new_leaves)
    lp, np_, idx = ints(batch.low_proofs), ints(batch.new_proofs), [int(x) for x in batch.low_indices.cpu()]
    out = []
    for i in range(n):
        j = batch.first_index + i
        new_leaf = tuple(new[3 * i:3 * i + 3])
        out.append((roots[i], tuple(low[3 * i:3 * i + 3]), lp[d * i:d * i + d], [1 - ((idx[i] >> L) & 1) for L in range(d)], roots[i + 1], new_leaf, j,
                    np_[d * i:d * i + d], [1 - ((j >> L) & 1) for L in range(d)], 1 if new_leaf[1] == 0 else 0))
    return out


def check_export(tree, model):
    leaves, nodes, pre = tree.export()
    assert ints(pre) == [x for p in model.pre for x in p]
    assert torch.equal(leaves, PS.hash_many_device(pre))
    assert torch.equal(nodes, PS.merkle_device(leaves))
    assert tree.get_root() == model.root() and tree.used == model.used


def distinct(seed, n, taken=()):
    gen, out, seen = O.SplitMix64(seed), [], set(taken)
    while len(out) < n:
        v = gen.fr()
        if v and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def ordered(vals, order, seed):
    vals = sorted(vals)
    if order == "descending":
        vals.reverse()
    elif order == "random":
        random.Random(seed).shuffle(vals)
    return vals


def test_depth_3_filled_against_the_restatement(lib):
    """the reference's own tree: depth 3, seven insertions fill it; the model hashes with the big-integer restatement"""
    vals = [5, R - 1, 1, 1 << 200, 3, (1 << 64) + 9, 4]
    model = Model(3, ref_hash)
    with PS.IndexedMerkleTree(3) as tree:
        leaves, nodes, pre = tree.export()
        assert ints(leaves) == [PR.hash(0, 0, 0)] * 8 and ints(pre) == [0] * 24
        assert ints(nodes) == model.nodes() and tree.get_root() == model.root() and tree.used == 1
        batch = tree.insert_batch(vals)
        want = [model.insert(v) for v in vals]
        assert witnesses(batch) == want
        assert [batch.round(i) for i in range(7)] == want
        leaves, nodes, pre = tree.export()
        assert ints(pre) == [x for p in model.pre for x in p]
        assert ints(leaves) == model.levels[0] and ints(nodes) == model.nodes()
        assert tree.used == 8 and tree.get_root() == model.root()
        assert [tree.leaf(i) for i in range(8)] == model.pre


def test_depth_1_the_two_leaves_are_siblings(lib):
    model = Model(1, host_hash)
    with PS.IndexedMerkleTree(1) as tree:
        batch = tree.insert_batch([77])
        want = model.insert(77)
        assert witnesses(batch) == [want] and batch.round(0) == want
        assert want[7] == [PS.hash([0, 77, 1])]                                     # the new leaf's proof: the low leaf AFTER its update in the same step
        assert want[2] == [PS.hash([0, 0, 0])]
        check_export(tree, model)
        with pytest.raises(_lib.ZkhipError) as e:
            tree.insert_batch([78])
        assert e.value.code == EINVAL and e.value.index == 0                        # full


@pytest.fixture(scope="module")
def empty_10():
    """the levels of the empty depth-10 tree: eleven host hashes, computed once"""
    return Model(10, host_hash)


def model_10(empty_10):
    m = Model.__new__(Model)
    m.depth, m.H, m.used = 10, host_hash, 1
    m.pre, m.levels = list(empty_10.pre), [list(level) for level in empty_10.levels]
    return m


@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 200])
def test_depth_10_one_batch(lib, empty_10, n, order):
    vals = ordered(distinct(1000 + n, n), order, n)
    model = model_10(empty_10)
    with PS.IndexedMerkleTree(10) as tree:
        batch = tree.insert_batch(vals)
        want = [model.insert(v) for v in vals]
        got = witnesses(batch)
        assert got == want
        assert [int(x) for x in batch.low_indices.cpu()] == ([0] * n if order == "descending" else list(range(n)) if order == "ascending" else PS.imt_link([], vals))
        check_export(tree, model)


@pytest.mark.parametrize("sizes", [(40, 60), (20, 30, 50)])
def test_batches_on_one_object(lib, empty_10, sizes):
    """siblings come from the tree the batch before left; the middle one of three batches runs with out = NULL and the third reads what it wrote"""
    vals = distinct(0xBA7C4 + len(sizes), sum(sizes) - 2) + [1, R - 1]
    random.Random(len(sizes)).shuffle(vals)
    model = model_10(empty_10)
    with PS.IndexedMerkleTree(10) as tree:
        at = 0
        for b, size in enumerate(sizes):
            part = vals[at:at + size]
            at += size
            silent = len(sizes) == 3 and b == 1
            batch = tree.insert_batch(part, witness=not silent)
            want = [model.insert(v) for v in part]
            if silent:
                assert batch is None
            else:
                assert witnesses(batch) == want and batch.first_index == model.used - size
            check_export(tree, model)
        assert tree.insert_batch([]).n == 0 and tree.used == model.used             # an empty batch: nothing happens
        check_export(tree, model)


def test_refusals_leave_everything_as_it_was(lib):
    model = Model(3, host_hash)
    with PS.IndexedMerkleTree(3) as tree:
        for v in (50, 20, 70):
            model.insert(v)
        tree.insert_batch([50, 20, 70])
        check_export(tree, model)
        before = [t.clone() for t in tree.export()]
        cases = [([0], 0), ([30, 0], 1), ([20], 0), ([10, 30, 70, 40], 2), ([10, 30, 40, 30], 3), ([1, 2, 3, 4, 5], 4), ([1, 2, 3, 4, 4], 4)]
        for vals, bad in cases:
            n = len(vals)
            bufs = [torch.full((rows, 4), 0x55, dtype=torch.int64, device="cuda") for rows in (n + 1, 3 * n, 3 * n, n, 3 * n, 3 * n)]
            w = _lib.ImtWitness(*(b.data_ptr() for b in bufs))
            words = F.fr_encode(vals)
            first = C.c_size_t(99)
            assert lib.zkhip_imt_insert(tree._h, words.ctypes.data, n, C.byref(w), C.byref(first), None) == EINVAL, vals
            assert first.value == bad, vals
            assert lib.zkhip_imt_insert(tree._h, words.ctypes.data, n, None, C.byref(first), None) == EINVAL and first.value == bad
            with pytest.raises(_lib.ZkhipError) as e:
                tree.insert_batch(vals)
            assert e.value.code == EINVAL and e.value.index == bad
            torch.cuda.synchronize()
            assert all(bool((b == 0x55).all()) for b in bufs), vals
            assert tree.used == 4 and tree.get_root() == model.root()
            assert all(torch.equal(a, b) for a, b in zip(before, tree.export()))
        # a null or misaligned witness pointer: refused before the linking, the index does not advance
        good = F.fr_encode([10])
        bufs = [torch.full((8, 4), 0x55, dtype=torch.int64, device="cuda") for _ in range(6)]
        first = C.c_size_t(99)
        for k in range(6):
            ptrs = [b.data_ptr() for b in bufs]
            ptrs[k] = 0
            assert lib.zkhip_imt_insert(tree._h, good.ctypes.data, 1, C.byref(_lib.ImtWitness(*ptrs)), C.byref(first), None) == EINVAL
            ptrs[k] = bufs[k].data_ptr() + (2 if k == 3 else 8)
            assert lib.zkhip_imt_insert(tree._h, good.ctypes.data, 1, C.byref(_lib.ImtWitness(*ptrs)), C.byref(first), None) == EINVAL
            assert b"aligned" in lib.zkhip_last_error() and first.value == C.c_size_t(-1).value
        assert lib.zkhip_imt_insert(tree._h, None, 1, None, C.byref(first), None) == EINVAL
        torch.cuda.synchronize()
        assert all(bool((b == 0x55).all()) for b in bufs) and tree.used == 4
        # and the tree still takes the four values that fit
        batch = tree.insert_batch([10, 30, 40, 60])
        assert witnesses(batch) == [model.insert(v) for v in (10, 30, 40, 60)]
        check_export(tree, model)


def test_read_backs(lib, empty_10):
    vals = ordered(distinct(0x2EAD, 37), "random", 5)
    model = model_10(empty_10)
    with PS.IndexedMerkleTree(10) as tree:
        assert tree.get_proof(0) == (model.proof(0), model.helper(0)) and tree.leaf(0) == (0, 0, 0)
        batch = tree.insert_batch(vals)
        want = [model.insert(v) for v in vals]
        assert batch.round(0) == want[0] and batch.round(36) == want[36]
        with pytest.raises(IndexError):
            batch.round(37)
        root = tree.get_root()
        assert root == model.root()
        for index in (0, 37, 38, 1023):                                             # the head, the last used leaf, the first unused one, the last leaf
            proof, helper = tree.get_proof(index)
            assert (proof, helper) == (model.proof(index), model.helper(index))
            leaf = tree.leaf(index)
            assert leaf == model.pre[index]
            assert PS.IndexedMerkleTree.verify_proof(leaf, index, root, proof)
            # with the index's lowest bit flipped the path verifies only where the two sibling leaves are equal (two unused ones)
            assert PS.IndexedMerkleTree.verify_proof(leaf, index ^ 1, root, proof) == (model.levels[0][index] == model.levels[0][index ^ 1]) == (index >= 38)
            assert not PS.IndexedMerkleTree.verify_proof((leaf[0], leaf[1], (leaf[2] + 1) % R), index, root, proof)
        for call in (tree.get_proof, tree.leaf):
            with pytest.raises(IndexError):
                call(1024)
        out = (C.c_uint64 * 40)()
        assert lib.zkhip_imt_proof(tree._h, 1024, out) == EINVAL and lib.zkhip_imt_leaf(tree._h, 1024, out) == EINVAL
        depth, used = C.c_uint32(), C.c_uint32()
        assert lib.zkhip_imt_size(tree._h, C.byref(depth), C.byref(used)) == 0 and (depth.value, used.value) == (10, 38)

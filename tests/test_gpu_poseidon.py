"""GPU (-m gpu): the Poseidon kernels (include/zkhip.h, "Poseidon"; csrc/poseidon.hip) bit for bit against the big-integer restatement
(tests/poseidon_reference.py).  `hash_many_device` at every width's framing (a lone element, whole chunks, a half chunk, the cap) and at
message counts around the workgroup of 128 lanes; `merkle_device` at the sizes where the tree kernel changes its path -- a part of a run, one
run (one workgroup folding to the root), two and four workgroups handing their nodes on through one ticket -- with EVERY node compared, then
one tree of 2^15 leaves (four tiers of tickets) against `hash_many_device` level by level.  The restatement costs about 1 ms per
permutation: the tree reference is computed once, for 4 SUBTREE leaves, and every smaller tree is a left subtree of it."""
import numpy as np
import pytest
import torch

import poseidon_reference as PR
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F, poseidon as PS
from zksnap_circuits_halo2_amd.tensors import fr_ints as to_ints

pytestmark = pytest.mark.gpu
R = O.R_MOD
EINVAL = -1
S = PS.SUBTREE                        # csrc/poseidon.hip PM_SUBTREE through include/zkhip.h
EDGE = [0, 1, R - 1, 1 << 64, (1 << 253) + 5, R - (1 << 64)]


def to_device(ints, *shape):
    return torch.from_numpy(F.fr_encode(ints).view(np.int64)).reshape(*shape, 4).to("cuda")


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, PS.MAX_WIDTH])
def test_hash_many_edge_values_in_every_position(lib, width):
    """message i has edge value i % 6 in position i // 6 % width and small distinct values elsewhere; then every position at an edge value at once"""
    msgs = []
    for pos in range(width):
        for e in EDGE:
            m = [1000 * pos + j + 2 for j in range(width)]
            m[pos] = e
            msgs.append(m)
    msgs += [[e] * width for e in EDGE]
    got = to_ints(PS.hash_many_device(to_device([v for m in msgs for v in m], len(msgs), width)))
    assert got == [PR.hash(*m) for m in msgs]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_hash_many_message_counts(lib, n):
    """one lane, a part-filled wave, a whole wave, one lane of a second wave, a third workgroup; width 3: a whole chunk and a half one"""
    gen = O.SplitMix64(7000 + n)
    flat = [gen.fr() for _ in range(3 * n)]
    d_out = torch.zeros((n + 1, 4), dtype=torch.int64, device="cuda")
    PS.hash_many_device(to_device(flat, n, 3), out=d_out)
    got = to_ints(d_out)
    assert got[:n] == [PR.hash(*flat[3 * i:3 * i + 3]) for i in range(n)]
    assert got[n] == 0                                                              # nothing behind the last digest is written
    assert got[:n] == [PS.hash(flat[3 * i:3 * i + 3]) for i in range(n)]            # the library's host form agrees


def test_hash_many_refuses_bad_widths(lib):
    d = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    for width in (0, PS.MAX_WIDTH + 1):
        assert lib.zkhip_poseidon_hash_many_device(d.data_ptr(), 1, width, d.data_ptr(), None) == EINVAL
    assert lib.zkhip_poseidon_hash_many_device(d.data_ptr(), 0, 1, d.data_ptr(), None) == 0


@pytest.fixture(scope="module")
def tree():
    """4 S leaves (edge values first) and every level of their tree, from the restatement: computed once, read only"""
    gen = O.SplitMix64(0x7EE)
    leaves = EDGE + [gen.fr() for _ in range(4 * S - len(EDGE))]
    return leaves, PR.merkle_levels(leaves)


@pytest.mark.parametrize("n", [1, 2, 4, S // 2, S, 2 * S, 4 * S])
def test_merkle_every_node_against_the_restatement(lib, tree, n):
    leaves, levels = tree
    want = [v for L in range(1, n.bit_length()) for v in levels[L][:n >> L]]        # the tree over the first n leaves is a left subtree
    assert len(want) == n - 1
    d_leaves = to_device(leaves[:n], n)
    nodes = PS.merkle_device(d_leaves)
    assert nodes.shape == (n - 1, 4)
    assert to_ints(nodes) == want
    assert to_ints(d_leaves) == leaves[:n]                                          # the leaves are read, not written


def test_merkle_large_against_hash_many_level_by_level(lib):
    """2^15 leaves: 128 workgroups, nodes handed on through tickets at four tiers.  Device against device: hash_many_device is pinned above."""
    n = 1 << 15
    gen = O.SplitMix64(0xB16)
    d_leaves = to_device([gen.fr() for _ in range(n)], n)
    t = PS.MerkleTree(d_leaves)
    assert t.depth == 15
    for L in range(1, 16):
        want = PS.hash_many_device(t.level(L - 1).reshape(n >> L, 2, 4))
        assert torch.equal(t.level(L), want), L
    # a second tree on the same stream right behind the first: the tickets are cleared per call
    again = PS.merkle_device(d_leaves)
    assert torch.equal(again, t.nodes)


@pytest.mark.parametrize("n", [3, 6, 0])
def test_merkle_refuses_anything_but_a_power_of_two(lib, n):
    d_leaves = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    d_nodes = torch.full((8, 4), 0x55, dtype=torch.int64, device="cuda")
    assert lib.zkhip_poseidon_merkle_device(d_leaves.data_ptr(), n, d_nodes.data_ptr(), None) == EINVAL
    assert b"power of two" in lib.zkhip_last_error()
    torch.cuda.synchronize()
    assert bool((d_nodes == 0x55).all())                                            # nothing written
    if n:
        with pytest.raises(_lib.ZkhipError):
            PS.MerkleTree(d_leaves[:n])


def test_merkle_tree_proofs(lib, tree):
    leaves, levels = tree
    n = 2 * S
    t = PS.MerkleTree(to_device(leaves[:n], n))
    root = t.get_root()
    assert root == levels[n.bit_length() - 1][0]
    for index in (0, n - 1, n // 2 + 3):
        proof, helper = t.get_proof(index)
        assert proof == [levels[L][(index >> L) ^ 1] for L in range(t.depth)]
        assert helper == [1 - ((index >> L) & 1) for L in range(t.depth)]           # the reference's is-left flags
        assert PS.MerkleTree.verify_proof(leaves[index], index, root, proof)
        assert not PS.MerkleTree.verify_proof(leaves[index], index ^ 1, root, proof)
        assert not PS.MerkleTree.verify_proof((leaves[index] + 1) % R, index, root, proof)
    one = PS.MerkleTree(to_device(leaves[:1], 1))
    assert one.get_root() == leaves[0] and one.get_proof(0) == ([], []) and PS.MerkleTree.verify_proof(leaves[0], 0, leaves[0], [])
    with pytest.raises(IndexError):
        t.get_proof(n)

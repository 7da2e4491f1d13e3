"""CPU: the linking of the indexed Merkle tree (include/zkhip.h, "indexed Merkle tree"; csrc/imt.hpp) through `zkhip_imt_link`, the call the tree
object runs before it enqueues a batch -- against a brute-force scan over every used leaf, which is what the reference's `update_idx_leaf`
does -- its refusals with the index of the first bad value, and the new symbols declared the same way in the header and the ctypes table.
Nothing here touches a GPU: the last test runs the call in a process that sees none."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import abi_header as AH
from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F, poseidon as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R_MOD
EINVAL = -1
NONE = C.c_size_t(-1).value


def scan_link(used, new):
    """the low leaf of every new value by a scan: the used leaf with the greatest val below it; `used` grows as the batch goes"""
    vals, out = list(used) if used else [0], []
    for v in new:
        assert 0 < v < R and v not in vals
        best = max((x for x in vals if x < v))
        out.append(vals.index(best))
        vals.append(v)
    return out


def values(seed, n):
    gen = O.SplitMix64(seed)
    out = []
    while len(out) < n:
        v = gen.fr()
        if v and v not in out:
            out.append(v)
    return out


@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
@pytest.mark.parametrize("n", [1, 2, 33, 200])
def test_link_on_an_empty_tree(lib, order, n):
    new = sorted(values(100 + n, n))
    if order == "descending":
        new.reverse()
    elif order == "random":
        random.Random(n).shuffle(new)
    want = scan_link([], new)
    assert PS.imt_link([], new) == want
    assert PS.imt_link([0], new) == want                                            # the head named: the same tree
    if order == "ascending":
        assert want == list(range(n))                                               # the low leaf is always the previous new leaf
    if order == "descending":
        assert want == [0] * n                                                      # always the head


def test_link_the_smallest_and_the_largest_value(lib):
    assert PS.imt_link([], [1]) == [0]
    assert PS.imt_link([], [R - 1]) == [0]
    assert PS.imt_link([], [R - 1, 1, 2, R - 2]) == scan_link([], [R - 1, 1, 2, R - 2]) == [0, 0, 2, 3]
    assert PS.imt_link([0, 1 << 64, 1 << 128, 1 << 192], [(1 << 64) + 1, (1 << 64) - 1, 1 << 200, (1 << 128) - 1]) == [1, 0, 3, 4]


def test_link_on_a_tree_with_leaves(lib):
    old = values(7, 50)
    new = values(8, 70)
    new = [v for v in new if v not in old]
    assert PS.imt_link([0] + old, new) == scan_link([0] + old, new)
    assert PS.imt_link([0] + old, []) == []


@pytest.mark.parametrize("used, new, bad", [
    ([], [0], 0),
    ([], [5, 0, 6], 1),
    ([], [5, 6, 7, 6], 3),                      # a duplicate within the batch: the later one
    ([0, 9, 4], [3, 8, 4, 1], 2),               # a duplicate of an existing value
    ([0, 9, 4], [9], 0),
])
def test_link_refusals_name_the_first_bad_value(lib, used, new, bad):
    with pytest.raises(_lib.ZkhipError) as e:
        PS.imt_link(used, new)
    assert e.value.code == EINVAL and e.value.index == bad
    assert f"value {bad}" in str(e.value)


def test_link_refuses_unreduced_words_and_bad_arguments(lib):
    low = (C.c_uint32 * 4)(7, 7, 7, 7)
    bad = C.c_size_t(5)
    r_words = np.array([(R >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)     # the modulus itself: not a reduced element
    two = np.concatenate([F.fr_encode([3])[0], r_words]).astype(np.uint64)
    assert lib.zkhip_imt_link(None, 0, two.ctypes.data, 2, low, C.byref(bad)) == EINVAL and bad.value == 1
    assert list(low) == [7, 7, 7, 7]                                                # nothing written on a refusal
    one = F.fr_encode([3])
    assert lib.zkhip_imt_link(None, 1, one.ctypes.data, 1, low, C.byref(bad)) == EINVAL and bad.value == NONE
    assert lib.zkhip_imt_link(None, 0, None, 1, low, C.byref(bad)) == EINVAL and bad.value == NONE
    assert lib.zkhip_imt_link(None, 0, one.ctypes.data, 1, None, C.byref(bad)) == EINVAL
    assert lib.zkhip_imt_link(one.ctypes.data, 1, one.ctypes.data, 1, low, None) == EINVAL       # leaf 0 must hold 0
    assert b"head" in lib.zkhip_last_error()
    dup = F.fr_encode([0, 4, 4])
    assert lib.zkhip_imt_link(dup.ctypes.data, 3, one.ctypes.data, 1, low, C.byref(bad)) == EINVAL and bad.value == NONE
    assert lib.zkhip_imt_link(None, 0, None, 0, None, None) == 0


def test_tree_calls_check_their_arguments_before_any_device(lib):
    h = C.c_void_p(1)
    for depth in (0, _lib.ZKHIP_IMT_MAX_DEPTH + 1):
        assert lib.zkhip_imt_create(depth, C.byref(h)) == EINVAL and h.value is None
        assert b"depth" in lib.zkhip_last_error()
        h = C.c_void_p(1)
    assert lib.zkhip_imt_create(3, None) == EINVAL
    assert lib.zkhip_imt_destroy(None) == 0
    out = (C.c_uint64 * 12)()
    assert lib.zkhip_imt_root(None, out) == EINVAL and lib.zkhip_imt_leaf(None, 0, out) == EINVAL and lib.zkhip_imt_proof(None, 0, out) == EINVAL
    assert lib.zkhip_imt_size(None, None, None) == EINVAL and lib.zkhip_imt_insert(None, None, 0, None, None, None) == EINVAL
    assert lib.zkhip_imt_export_device(None, out, out, out, None) == EINVAL


HEADER = {
    "zkhip_imt_create": ["uint32_t depth", "zkhip_imt **t"],
    "zkhip_imt_destroy": ["zkhip_imt *t"],
    "zkhip_imt_insert": ["zkhip_imt *t", "const uint64_t *values", "size_t n_new", "const zkhip_imt_witness *out", "size_t *first_bad", "void *stream"],
    "zkhip_imt_root": ["zkhip_imt *t", "uint64_t out[4]"],
    "zkhip_imt_leaf": ["zkhip_imt *t", "uint32_t index", "uint64_t out[12]"],
    "zkhip_imt_proof": ["zkhip_imt *t", "uint32_t index", "uint64_t *out"],
    "zkhip_imt_size": ["const zkhip_imt *t", "uint32_t *depth", "uint32_t *used"],
    "zkhip_imt_export_device": ["zkhip_imt *t", "void *d_leaves", "void *d_nodes", "void *d_preimages", "void *stream"],
    "zkhip_imt_link": ["const uint64_t *used_vals", "size_t n_used", "const uint64_t *new_vals", "size_t n_new", "uint32_t *low_index_out", "size_t *first_bad"],
}


def test_header_declares_the_calls_the_struct_and_the_cap():
    for name, params in HEADER.items():
        assert AH.params(name) == params
    assert AH.structs()["zkhip_imt_witness"] == [("void *", f) for f, _ in _lib.ImtWitness._fields_]
    assert all(ty is C.c_void_p for _, ty in _lib.ImtWitness._fields_) and C.sizeof(_lib.ImtWitness) == 6 * C.sizeof(C.c_void_p)
    assert AH.defines()["ZKHIP_IMT_MAX_DEPTH"] == _lib.ZKHIP_IMT_MAX_DEPTH >= 20
    text = " ".join(open(os.path.join(ROOT, "include", "zkhip.h")).read().replace("\n *", " ").split())
    for needle in ("parity with it is unpinned", "permanent head", "greatest val < v", "nothing is enqueued and the tree is unchanged",
                   "is_new_leaf_largest = (new_leaf.next_val == 0)", "removal of leaves", "never initialises HIP"):
        assert needle in text, needle


def test_library_exports_the_calls(lib):
    for name in HEADER:
        assert hasattr(lib, name), f"libzkhip.so does not export {name}"
    from zksnap_circuits_halo2_amd.poseidon import IndexedMerkleTree, ImtBatch

    for name in ("insert_batch", "get_root", "get_proof", "verify_proof", "leaf", "export", "__enter__", "__exit__"):
        assert callable(getattr(IndexedMerkleTree, name))
    assert callable(ImtBatch.round)


def test_link_runs_in_a_process_without_a_device():
    """a fresh process that sees no GPU: the linking answers, and creating a tree says ZKHIP_ENODEV instead of computing anywhere else"""
    code = (
        "import ctypes as C, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from zksnap_circuits_halo2_amd import _lib, poseidon as PS\n"
        "print(PS.imt_link([], [5, 3, 9, 4]))\n"
        "h = C.c_void_p()\n"
        "print(_lib.load().zkhip_imt_create(3, C.byref(h)), h.value)\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == ["[0, 0, 1, 2]", "-2 None"]

"""CPU: `zkhip_lookup_permute_many_device` / `zkhip_lookup_products_device` are declared the same way everywhere they are declared -- the header,
the ctypes table, the C++ mirror and the Rust shim -- and libzkhip.so exports both; and the restatement the permute call implements (a histogram
over the sorted table instead of a sort of the input column) is `permute_expression_pair`, pinned here in plain Python, independently of the GPU."""
import os
import random
import re

import pytest

import abi_header as AH
from oracle import bn254 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkhip_lookup_permute_many_device", "zkhip_lookup_products_device")
HEADER = {
    NAMES[0]: ["const void *const *d_inputs", "const void *const *d_tables", "uint32_t n_lookups", "uint32_t log_n", "size_t usable_rows",
               "void *d_permuted_inputs", "void *d_permuted_tables", "void *stream"],
    NAMES[1]: ["const void *const *d_inputs", "const void *const *d_tables", "const void *d_permuted_inputs", "const void *d_permuted_tables",
               "uint32_t n_lookups", "uint32_t log_n", "size_t usable_rows", "const uint64_t beta[4]", "const uint64_t gamma[4]", "void *d_z", "void *stream"],
}
RUST = {
    NAMES[0]: ["d_inputs: *const *const c_void", "d_tables: *const *const c_void", "n_lookups: u32", "log_n: u32", "usable_rows: usize",
               "d_permuted_inputs: *mut c_void", "d_permuted_tables: *mut c_void", "stream: *mut c_void"],
    NAMES[1]: ["d_inputs: *const *const c_void", "d_tables: *const *const c_void", "d_permuted_inputs: *const c_void", "d_permuted_tables: *const c_void",
               "n_lookups: u32", "log_n: u32", "usable_rows: usize", "beta: *const u64", "gamma: *const u64", "d_z: *mut c_void", "stream: *mut c_void"],
}


def test_header_declares_both_calls():
    for name in NAMES:
        assert AH.params(name) == HEADER[name]


def test_cpp_mirror_and_rust_shim_agree_with_the_header():
    hpp = open(os.path.join(ROOT, "include", "zkhip.hpp")).read()
    for name, mirror in zip(NAMES, ("permute_expression_pairs_device", "lookup_products_device")):
        assert re.search(r"inline void " + mirror + r"\(", hpp), f"include/zkhip.hpp has no {mirror}"
        assert AH.hpp_call_arities(name), f"include/zkhip.hpp never calls {name}"
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust-shim", "zkhip_ffi.rs")).read())
    for name in NAMES:
        assert AH.rust_functions().get(name) == ("c_int", RUST[name]), f"rust-shim/zkhip_ffi.rs does not declare {name} this way"
    methods = set(re.findall(r"pub\(crate\) fn (\w+)", ffi))
    assert {"lookup_permute_many", "lookup_products"} <= methods
    patch = open(os.path.join(ROOT, "rust-shim", "prover_patch.rs")).read()
    assert "base.lookup_permute_many(" in patch and "base.lookup_products(" in patch
    from zksnap_circuits_halo2_amd import evaluation as E

    assert callable(E.permute_expression_pairs_device) and callable(E.lookup_products_device)


def test_library_exports_both_calls(lib):
    for name in NAMES:
        assert hasattr(lib, name), f"libzkhip.so does not export {name}"


# ---- the algorithm, in plain Python ---------------------------------------------------------------------------------------------------------
def histogram_permute(inputs, table, u):
    """The restatement the device call implements.  t = the table's canonical values ascending; every input row is counted into the slot of its
    lower bound in t (so only the first instance of a value ever receives a count); A' is t[j] repeated cnt[j] times; S' is t[j] at the first row
    of run j; the repeated rows, numbered 0 .. R - 1 in row order, take the unused instances (cnt == 0, ascending): rank r takes rank R - 1 - r."""
    import bisect

    t = sorted(v % O.R_MOD for v in table[:u])
    cnt = [0] * u
    for v in inputs[:u]:
        v %= O.R_MOD
        j = bisect.bisect_left(t, v)
        if j == u or t[j] != v:
            raise ValueError("ConstraintSystemFailure: lookup input value not in table")
        cnt[j] += 1
    unused = [j for j in range(u) if cnt[j] == 0]
    repeated_total = sum(max(c - 1, 0) for c in cnt)
    assert repeated_total == len(unused)
    pa, ps, r = [], [], 0
    for j in range(u):
        for e in range(cnt[j]):
            pa.append(t[j])
            if e == 0:
                ps.append(t[j])
            else:
                ps.append(t[unused[repeated_total - 1 - r]])
                r += 1
    return pa, ps


def _cases():
    rng = random.Random(0x10061)
    full = lambda: rng.randrange(O.R_MOD)
    for trial in range(120):
        u = rng.choice([1, 2, 3, 7, 16, 33, 100, 250])
        kind = trial % 6
        if kind == 0:                      # duplicate-heavy range table: i mod 2^bits, skewed input (padding zeros)
            bits = rng.randrange(0, 6)
            table = [i % (1 << bits) for i in range(u)]
            inputs = [rng.choice(table) if rng.random() < 0.5 else 0 for _ in range(u)]
        elif kind == 1:                    # full-width table, inputs drawn from it
            table = [full() for _ in range(u)]
            inputs = [rng.choice(table) for _ in range(u)]
        elif kind == 2:                    # values on both sides of 2^64
            table = [(1 << 64) + rng.randrange(-4, 5) for _ in range(u)]
            inputs = [rng.choice(table) for _ in range(u)]
        elif kind == 3:                    # all inputs equal
            table = [rng.randrange(8) for _ in range(u)]
            inputs = [table[rng.randrange(u)]] * u
        elif kind == 4:                    # every input distinct: a shuffle of a table of distinct values
            table = [(i << 40) + rng.randrange(1 << 40) for i in rng.sample(range(1 << 30), u)]
            inputs = table[:]
            rng.shuffle(inputs)
        else:                              # full-width values with duplicates in the table
            pool = [full() for _ in range(max(1, u // 3))]
            table = [rng.choice(pool) for _ in range(u)]
            inputs = [rng.choice(table) for _ in range(u)]
        yield inputs, table, u


def test_histogram_restatement_is_permute_expression_pair():
    count = 0
    for inputs, table, u in _cases():
        assert histogram_permute(inputs, table, u) == O.permute_expression_pair(inputs, table, u), (inputs, table, u)
        count += 1
    assert count == 120


def test_histogram_restatement_rejects_a_missing_value():
    table = [i % 16 for i in range(64)]
    for bad in (16, 1 << 64, (1 << 64) + 3, O.R_MOD - 1):           # a wide value whose low 64 bits are in the table is still missing
        inputs = [3] * 63 + [bad]
        with pytest.raises(ValueError):
            O.permute_expression_pair(inputs, table, 64)
        with pytest.raises(ValueError):
            histogram_permute(inputs, table, 64)

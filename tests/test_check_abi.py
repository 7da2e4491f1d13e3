"""CPU: the three witness checks (`zkhip_check_rows_device`, `zkhip_check_copies_device`, `zkhip_check_lookups_device`) are declared the same
way in the header, the ctypes table, the C++ mirror and the Rust shim, the record is 16 bytes everywhere, libzkhip.so exports the names -- and
`mock.verify_host`, which the GPU tests take their expected values from, is pinned here on hand-written cases."""
import ctypes as C
import os
import re
import subprocess

import abi_header as AH
from zksnap_circuits_halo2_amd import evaluation as E, fields as F, mock as M
from zksnap_circuits_halo2_amd.keygen import Assembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkhip_check_rows_device", "zkhip_check_copies_device", "zkhip_check_lookups_device")
HEADER = {
    NAMES[0]: ["const zkhip_vm_program *progs", "uint32_t n_progs", "const void *const *d_columns", "uint32_t n_columns", "uint32_t log_rows", "uint64_t row0",
               "uint64_t count", "void *d_reports", "void *stream"],
    NAMES[1]: ["const void *const *d_columns", "uint32_t n_columns", "uint32_t log_n", "const void *d_map_col", "const void *d_map_row", "void *d_report",
               "void *stream"],
    NAMES[2]: ["const void *const *d_inputs", "const void *const *d_tables", "uint32_t n_lookups", "uint32_t log_n", "size_t usable_rows", "void *d_reports",
               "void *stream"],
}
RUST = {
    NAMES[0]: ["progs: *const VmProgram", "n_progs: u32", "d_columns: *const *const c_void", "n_columns: u32", "log_rows: u32", "row0: u64", "count: u64",
               "d_reports: *mut c_void", "stream: *mut c_void"],
    NAMES[1]: ["d_columns: *const *const c_void", "n_columns: u32", "log_n: u32", "d_map_col: *const c_void", "d_map_row: *const c_void", "d_report: *mut c_void",
               "stream: *mut c_void"],
    NAMES[2]: ["d_inputs: *const *const c_void", "d_tables: *const *const c_void", "n_lookups: u32", "log_n: u32", "usable_rows: usize", "d_reports: *mut c_void",
               "stream: *mut c_void"],
}


def test_header_declares_the_three_calls_and_the_record():
    from zksnap_circuits_halo2_amd import _lib

    for name in NAMES:
        assert AH.params(name) == HEADER[name]
    assert AH.structs()["zkhip_check_report"] == [("uint64_t", "failures"), ("uint64_t", "first")]
    assert C.sizeof(_lib.CheckReport) == 16 and _lib.CheckReport.failures.offset == 0 and _lib.CheckReport.first.offset == 8


def test_cpp_mirror_and_rust_shim_agree_with_the_header():
    hpp = open(os.path.join(ROOT, "include", "zkhip.hpp")).read()
    for name, mirror in zip(NAMES, ("check_rows_device", "check_copies_device", "check_lookups_device")):
        assert re.search(r"inline (?:std::vector<zkhip_check_report>|zkhip_check_report) " + mirror + r"\(", hpp), f"include/zkhip.hpp has no {mirror}"
        assert AH.hpp_call_arities(name), f"include/zkhip.hpp never calls {name}"
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust-shim", "zkhip_ffi.rs")).read())
    for name in NAMES:
        assert AH.rust_functions().get(name) == ("c_int", RUST[name]), f"rust-shim/zkhip_ffi.rs does not declare {name} this way"
    rec = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub\(crate\) struct CheckReport\s*\{(.*?)\}", ffi, flags=re.S)
    assert rec and [" ".join(d.replace("pub ", "").split()) for d in rec.group(1).split(",") if d.strip()] == ["failures: u64", "first: u64"]
    methods = set(re.findall(r"pub\(crate\) fn (\w+)", re.search(r"impl DevCols \{.*?\n\}", ffi, flags=re.S).group(0)))
    assert {"check_rows", "check_copies", "check_lookups"} <= methods
    patch = open(os.path.join(ROOT, "rust-shim", "prover_patch.rs")).read()
    assert "pub(crate) fn mock_on_device(" in patch
    for call in ("DevCols::check_rows(", "DevCols::check_copies(", "DevCols::check_lookups("):
        assert call in patch, call


def test_record_is_16_bytes_in_c(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "zkhip.h"\nint main(void) { printf("%zu %zu\\n", sizeof(zkhip_check_report), sizeof(((zkhip_check_report *)0)->first)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "8"]


def test_library_exports_the_three_calls(lib):
    for name in NAMES:
        assert hasattr(lib, name), f"libzkhip.so does not export {name}"


# ---- verify_host, pinned on cases small enough to check by eye --------------------------------------------------------------------------------
K, N = 4, 16
U = N - 6                       # blinding_factors = 5: rows 0 .. 9 are usable


def _vertical_gate_circuit():
    """one advice column with q (a + b c - d) on rows 0 and 4, one lookup column against a fixed table, copies over advice 0 / advice 1 / fixed 1"""
    cs = E.ConstraintSystem(num_fixed=3, num_advice=2, gates=[[E.Fixed(0) * (E.Advice(0, 0) + E.Advice(0, 1) * E.Advice(0, 2) - E.Advice(0, 3))]],
                            lookups=[E.Lookup([E.Advice(1)], [E.Fixed(2)])], permutation_columns=[("advice", 0), ("advice", 1), ("fixed", 1)])
    q = [1 if r in (0, 4) else 0 for r in range(N)]
    a = [3, 5, 7, 38, 2, 9, 4, 38] + [11] * 8                          # 3 + 5 * 7 = 38, 2 + 9 * 4 = 38
    table = [r % 8 for r in range(N)]
    table[12] = 99                                                     # 99 occurs in the table only at a row that is not usable
    look = [r % 8 for r in range(N)]
    const = [0] * N
    return cs, [q, const, table], [a, look]


def test_verify_host_accepts_a_satisfied_witness():
    cs, fixed, advice = _vertical_gate_circuit()
    assert M.verify_host(cs, K, fixed, advice, (), Assembly(N, 3)) == []


def test_verify_host_locates_a_gate_failing_at_one_known_row():
    cs, fixed, advice = _vertical_gate_circuit()
    advice[0][7] = 39                                                  # the gate at row 4 reads rows 4 .. 7
    assert M.verify_host(cs, K, fixed, advice, (), None) == [("gate", 0, 0, 4, 1)]
    advice[0][3] = 0                                                   # ... and the one at row 0 reads row 3
    assert M.verify_host(cs, K, fixed, advice, (), None) == [("gate", 0, 0, 0, 2)]
    fixed[0][14] = 1                                                   # a selector behind the usable rows constrains nothing
    assert M.verify_host(cs, K, fixed, advice, (), None) == [("gate", 0, 0, 0, 2)]


def test_verify_host_gate_rotations_wrap():
    cs = E.ConstraintSystem(num_fixed=0, num_advice=1, gates=[[E.Advice(0, 0) - E.Advice(0, -1)]], blinding_factors=5)
    col = [5] * N
    col[N - 1] = 6                                                     # row 0 reads row -1 = row 15
    assert M.verify_host(cs, K, [], [col], (), None) == [("gate", 0, 0, 0, 1)]


def test_verify_host_three_cycle_with_one_cell_changed():
    cs, fixed, advice = _vertical_gate_circuit()
    asm = Assembly(N, 3)
    asm.copy(0, 9, 1, 2)                                               # advice0[9] = advice1[2] = fixed1[13]
    asm.copy(1, 2, 2, 13)
    advice[0][9], advice[1][2], fixed[1][13] = 2, 2, 2
    assert M.verify_host(cs, K, fixed, advice, (), asm) == []
    fixed[1][13] = 3
    # the cell that differs from its neighbours in the cycle fails, and so does the cell that maps to it: two cells of the three
    got = M.verify_host(cs, K, fixed, advice, (), asm)
    assert len(got) == 1 and got[0][0] == "copy" and got[0][3] == 2
    cycle = {(0, 9): None, (1, 2): None, (2, 13): None}
    for c, r in cycle:
        cycle[(c, r)] = (int(asm.map_col[c, r]), int(asm.map_row[c, r]))
    vals = {(0, 9): 2, (1, 2): 2, (2, 13): 3}
    bad = sorted(cell for cell, to in cycle.items() if vals[cell] != vals[to])
    assert (got[0][1], got[0][2]) == bad[0] and len(bad) == 2


def test_verify_host_lookup_value_only_behind_the_usable_rows():
    cs, fixed, advice = _vertical_gate_circuit()
    advice[1][6] = 99                                                  # in the table, but only at row 12 >= usable rows
    assert M.verify_host(cs, K, fixed, advice, (), None) == [("lookup", 0, 6, 1)]
    advice[1][2] = 8                                                   # nowhere in the table
    assert M.verify_host(cs, K, fixed, advice, (), None) == [("lookup", 0, 2, 2)]
    advice[1][13] = 1234                                               # an input behind the usable rows is not looked up
    assert M.verify_host(cs, K, fixed, advice, (), None) == [("lookup", 0, 2, 2)]


def test_verify_host_reads_word_arrays_like_integers():
    cs, fixed, advice = _vertical_gate_circuit()
    advice[0][7] = 39
    enc = lambda cols: [F.fr_encode(c) for c in cols]
    assert M.verify_host(cs, K, enc(fixed), enc(advice), (), None) == [("gate", 0, 0, 4, 1)]


def test_gate_programs_one_per_gate_polynomial():
    cs = E.halo2_lib_shape(5, 2)
    progs = M.gate_programs(cs)
    assert len(progs) == sum(len(g) for g in cs.gates) == 5 and len(M.gate_polynomials(cs)) == 5
    qc = E.quotient_columns(cs)
    for i, p in enumerate(progs):
        assert p.rot_scale == 1 and p.omega is None and sorted(p.rotations) == [0, 1, 2, 3]
        cols = {o[1] for ins in p.insns for o in ins[2:5] if o[0] == E.SRC_COLUMN}
        assert cols == {qc.fixed + i, qc.advice + i}                   # gate i reads its selector and its advice column, nothing else
    two = E.ConstraintSystem(num_fixed=1, num_advice=1, gates=[[E.Advice(0), E.Fixed(0) * E.Advice(0, 1)], [E.Advice(0) - E.Fixed(0)]])
    assert [(g, p) for g, p, _ in M.gate_polynomials(two)] == [(0, 0), (0, 1), (1, 0)] and len(M.gate_programs(two)) == 3

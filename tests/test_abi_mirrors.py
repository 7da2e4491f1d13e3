"""CPU: include/zkhip.h is the declaration of record, and every hand-written mirror of it agrees with it, function by function over the whole
header: the ctypes table `_lib._SIGS` (return type, arity, every parameter's type), the `ctypes.Structure` mirrors (the C compiler's sizes, field sizes and
offsets), the Python constants that restate a macro or an enumerator, the `extern "C"` block of rust-shim/zkhip_ffi.rs (names, order and
types of the parameters) and the calls of include/zkhip.hpp (arity).  A wrong entry in any of them is a corrupted call on the device; here it
is a failing case that names the function.  The declarations are read by tests/abi_header.py, nowhere else."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_header as AH
from zksnap_circuits_halo2_amd import _lib, evaluation as E

SCALAR = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
RESTYPE = {"int": C.c_int, "void": None, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "const char *": C.c_char_p, "zkhip_transcript *": C.c_void_p}
MIRRORS = {"zkhip_vm_operand": _lib.VmOperand, "zkhip_vm_insn": _lib.VmInsn, "zkhip_vm_program": _lib.VmProgram, "zkhip_row_shard_ref": E._ShardRef,
           "zkhip_prover_query": _lib.ProverQueryC, "zkhip_check_report": _lib.CheckReport, "zkhip_imt_witness": _lib.ImtWitness}
CONSTANTS = [(_lib, "ZKHIP_MAX_ROOTS", "ZKHIP_MAX_ROOTS"), (_lib, "ZKHIP_MAX_PAIRS", "ZKHIP_MAX_PAIRS"), (_lib, "ZKHIP_POSEIDON_MAX_WIDTH", "ZKHIP_POSEIDON_MAX_WIDTH"),
             (_lib, "ZKHIP_POSEIDON_SUBTREE", "ZKHIP_POSEIDON_SUBTREE"), (_lib, "ZKHIP_IMT_MAX_DEPTH", "ZKHIP_IMT_MAX_DEPTH"), (_lib, "VM_REGS", "ZKHIP_VM_REGS"),
             (E, "COL_COEFF", "ZKHIP_COL_COEFF"), (E, "COL_EXTENDED", "ZKHIP_COL_EXTENDED"), (E, "COL_ROW_SHARDS", "ZKHIP_COL_ROW_SHARDS")]
CONSTANTS += [(E, name[len("ZKHIP_"):], name) for name in AH.enums()]                 # evaluation.SRC_* / OP_*
RUST_SCALAR = {"int": "c_int", "uint32_t": "u32", "uint64_t": "u64", "size_t": "usize"}
RUST_POINTEE = dict(RUST_SCALAR, void="c_void", char="c_char", uint8_t="u8")
RUST_RETURN = {"int": "c_int", "void": None, "const char *": "*const c_char"}
CALLED = [name for name in sorted(AH.functions()) if AH.hpp_call_arities(name)]


def test_the_parsers_see_the_whole_surface():
    """a parser that went blind would leave the parametrised tests below without cases, not failing"""
    assert len(AH.functions()) >= 150 and len(AH.rust_functions()) >= 47 and len(CALLED) >= 73 and len(AH.structs()) >= 7


# ---- ctypes -----------------------------------------------------------------------------------------------------------------------------
def _pointee(ty, suffix):
    """what a pointer or array parameter points at, qualifiers dropped: "uint64_t", "void *"; None for a pointer to an array"""
    if "(*)" in ty:
        return None
    return " ".join(re.sub(r"\bconst\b", "", ty if suffix else ty[:ty.rindex("*")]).split())


@pytest.mark.parametrize("name", sorted(AH.functions()))
def test_ctypes_signature_agrees_with_the_header(name):
    ret, params = AH.functions()[name]
    assert name in _lib._SIGS, f"{name} is declared in include/zkhip.h but has no entry in _lib._SIGS"
    restype, argtypes = _lib._SIGS[name]
    assert restype is RESTYPE[ret], (name, ret)
    assert len(argtypes) == len(params), (name, len(argtypes), len(params))
    for got, (ty, pname, suffix) in zip(argtypes, params):
        if "*" not in ty and not suffix:
            assert got is SCALAR[ty], (name, pname, ty)
        elif got is C.c_char_p:
            assert _pointee(ty, suffix) in ("char", "uint8_t"), (name, pname, ty)
        elif got is not C.c_void_p:                          # a typed pointer names the header's pointee
            pointee = _pointee(ty, suffix) or ""
            target = C.c_void_p if "*" in pointee else SCALAR.get(pointee, MIRRORS.get(pointee))
            assert target is not None and got is C.POINTER(target), (name, pname, ty + suffix)


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{"struct": [sizeof], "struct.field": [offsetof, sizeof]} of every struct of the header, as one C99 program prints them"""
    lines = []
    for name, fields in AH.structs().items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));' for _, field in fields]
    tmp = tmp_path_factory.mktemp("layout")
    src, exe = tmp / "layout.c", tmp / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zkhip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(AH.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {key: [int(v) for v in values] for key, *values in (line.split() for line in out.splitlines())}


@pytest.mark.parametrize("name", sorted(AH.structs()))
def test_ctypes_structure_has_the_layout_of_the_c_struct(name, c_layout):
    assert name in MIRRORS, f"include/zkhip.h defines {name}; MIRRORS names no ctypes.Structure for it"
    mirror = MIRRORS[name]
    assert [field[0] for field in mirror._fields_] == [field for _, field in AH.structs()[name]], name
    assert [C.sizeof(mirror)] == c_layout[name], name
    for field, *_ in mirror._fields_:
        assert [getattr(mirror, field).offset, getattr(mirror, field).size] == c_layout[f"{name}.{field}"], (name, field)


def test_every_structure_mirrors_one_struct():
    assert set(MIRRORS) <= set(AH.structs()) and len(set(MIRRORS.values())) == len(MIRRORS)


@pytest.mark.parametrize("module, attr, name", CONSTANTS, ids=[c[2] for c in CONSTANTS])
def test_python_constant_restates_the_header(module, attr, name):
    assert getattr(module, attr) == dict(AH.defines(), **AH.enums())[name], name


# ---- Rust -------------------------------------------------------------------------------------------------------------------------------
def _rust_type(ty, suffix):
    """a C parameter type as a regular expression over its Rust spelling: `const void *const *` is `*const *const c_void` (a raw pointer is
    `*const` where what it points at is const), an array parameter is a pointer, a struct is whatever the shim calls it"""
    base, *levels = [part.split() for part in ty.split("*")]
    levels += [[]] if suffix else []
    if not levels:
        return re.escape(RUST_SCALAR[ty])
    const = ["const" in level for level in [base] + levels[:-1]]
    name = next(word for word in base if word != "const")
    stars = re.escape("".join("*const " if c else "*mut " for c in reversed(const)))
    return stars + (re.escape(RUST_POINTEE[name]) if name in RUST_POINTEE else r"[A-Z]\w*")


@pytest.mark.parametrize("name", sorted(AH.rust_functions()))
def test_rust_declaration_agrees_with_the_header(name):
    assert name in AH.functions(), f"{name} is declared in rust-shim/zkhip_ffi.rs but not in include/zkhip.h"
    rret, rparams = AH.rust_functions()[name]
    ret, params = AH.functions()[name]
    assert ret in RUST_RETURN and rret == RUST_RETURN[ret], (name, rret, ret)
    assert len(rparams) == len(params), (name, len(rparams), len(params))
    for rust, (ty, pname, suffix) in zip(rparams, params):
        rname, rtype = [part.strip() for part in rust.split(":", 1)]
        assert rname == pname, (name, rname, pname)
        assert re.fullmatch(_rust_type(ty, suffix), rtype), (name, rust, ty + suffix)


# ---- C++ --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CALLED)
def test_cpp_mirror_passes_as_many_arguments_as_the_header_declares(name):
    arities = AH.hpp_call_arities(name)
    assert arities == [len(AH.params(name))] * len(arities), (name, arities)

"""CPU: `zkhip_fr_divide_by_roots(_device)` is declared the same way everywhere it is declared -- the header, the ctypes table, the C++ mirror and
the Rust shim -- and libzkhip.so exports both forms."""
import os

import abi_header as AH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkhip_fr_divide_by_roots", "zkhip_fr_divide_by_roots_device")


def test_header_declares_both_forms_and_the_limit():
    from zksnap_circuits_halo2_amd import _lib

    assert AH.defines()["ZKHIP_MAX_ROOTS"] == 8 == _lib.ZKHIP_MAX_ROOTS
    host, dev = AH.params(NAMES[0]), AH.params(NAMES[1])
    assert host == ["const uint64_t *a", "size_t n", "const uint64_t *roots", "uint32_t m", "uint64_t *q", "uint64_t *evals"]
    assert dev == ["const void *d_a", "size_t n", "const uint64_t *roots", "uint32_t m", "void *d_q", "void *d_evals", "void *stream"]


def test_cpp_mirror_and_rust_shim_agree_with_the_header():
    hpp = open(os.path.join(ROOT, "include", "zkhip.hpp")).read()
    for name in NAMES:
        assert AH.hpp_call_arities(name), f"include/zkhip.hpp never calls {name}"
    assert "detail::divide_by_roots(*acc, rs.points, *tmp)" in hpp           # ShplonkProver::begin: one division per rotation set
    rust = ["d_a: *const c_void", "n: usize", "roots: *const u64", "m: u32", "d_q: *mut c_void", "d_evals: *mut c_void", "stream: *mut c_void"]
    assert AH.rust_functions().get(NAMES[1]) == ("c_int", rust), "rust-shim/zkhip_ffi.rs does not declare zkhip_fr_divide_by_roots_device this way"


def test_library_exports_both_forms(lib):
    for name in NAMES:
        assert hasattr(lib, name), f"libzkhip.so does not export {name}"

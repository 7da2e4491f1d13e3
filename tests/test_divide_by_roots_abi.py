"""CPU: `zkhip_fr_divide_by_roots(_device)` is declared the same way everywhere it is declared -- the header, the ctypes table, the C++ mirror and
the Rust shim -- and libzkhip.so exports both forms."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkhip_fr_divide_by_roots", "zkhip_fr_divide_by_roots_device")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zkhip.h")).read(), flags=re.S)


def _header_params(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S)
    assert m, f"include/zkhip.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_both_forms_and_the_limit():
    assert re.search(r"^#define ZKHIP_MAX_ROOTS 8\s*$", _header(), flags=re.M)
    host, dev = _header_params(NAMES[0]), _header_params(NAMES[1])
    assert host == ["const uint64_t *a", "size_t n", "const uint64_t *roots", "uint32_t m", "uint64_t *q", "uint64_t *evals"]
    assert dev == ["const void *d_a", "size_t n", "const uint64_t *roots", "uint32_t m", "void *d_q", "void *d_evals", "void *stream"]


def test_ctypes_table_agrees_with_the_header():
    import ctypes as C

    from zksnap_circuits_halo2_amd import _lib

    assert _lib.ZKHIP_MAX_ROOTS == 8
    for name in NAMES:
        res, args = _lib._SIGS[name]
        params = _header_params(name)
        assert res is C.c_int and len(args) == len(params), name
        for ty, p in zip(args, params):
            want = C.c_void_p if "*" in p else {"size_t": C.c_size_t, "uint32_t": C.c_uint32}[p.split()[0]]
            assert ty is want, (name, p)


def test_cpp_mirror_and_rust_shim_agree_with_the_header():
    hpp = open(os.path.join(ROOT, "include", "zkhip.hpp")).read()
    for name in NAMES:
        calls = re.findall(r"\b" + name + r"\(", hpp)
        assert calls, f"include/zkhip.hpp never calls {name}"
    # the calls of the mirror pass as many arguments as the header declares
    for name in NAMES:
        for m in re.finditer(r"\b" + name + r"\(", hpp):
            depth, i, args = 1, m.end(), 1
            while depth:
                ch = hpp[i]
                depth += ch in "([{"
                depth -= ch in ")]}"
                args += ch == "," and depth == 1
                i += 1
            assert args == len(_header_params(name)), (name, args)
    assert "detail::divide_by_roots(*acc, rs.points, *tmp)" in hpp           # ShplonkProver::begin: one division per rotation set
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust-shim", "zkhip_ffi.rs")).read())
    m = re.search(r"fn\s+zkhip_fr_divide_by_roots_device\s*\((.*?)\)\s*->\s*c_int\s*;", ffi, flags=re.S)
    assert m, "rust-shim/zkhip_ffi.rs does not declare zkhip_fr_divide_by_roots_device"
    rust = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert rust == ["d_a: *const c_void", "n: usize", "roots: *const u64", "m: u32", "d_q: *mut c_void", "d_evals: *mut c_void", "stream: *mut c_void"]


def test_library_exports_both_forms(lib):
    for name in NAMES:
        assert hasattr(lib, name), f"libzkhip.so does not export {name}"
    from zksnap_circuits_halo2_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(NAMES) <= exported

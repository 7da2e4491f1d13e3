"""CPU: `zkhip_pairing_check` / `zkhip_pairing_check_device` and ZKHIP_MAX_PAIRS are declared the same way everywhere they are declared -- the
header, the ctypes table, the C++ mirror and the Rust shim -- libzkhip.so exports them (and the tower hook), and the argument checks answer
before any device is looked for: n = 65 is ZKHIP_EINVAL, and without a device the host form is ZKHIP_ENODEV."""
import ctypes as C
import os
import re
import subprocess
import sys

import abi_header as AH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkhip_pairing_check", "zkhip_pairing_check_device")
HEADER = {
    NAMES[0]: ["const uint64_t *g1", "const uint64_t *g2", "size_t n", "int *ok"],
    NAMES[1]: ["const void *d_g1", "const void *d_g2", "size_t n", "void *d_ok", "void *stream"],
}
RUST = {
    NAMES[0]: ["g1: *const u64", "g2: *const u64", "n: usize", "ok: *mut c_int"],
    NAMES[1]: ["d_g1: *const c_void", "d_g2: *const c_void", "n: usize", "d_ok: *mut c_void", "stream: *mut c_void"],
}
EINVAL, ENODEV = -1, -2


def test_header_declares_the_two_calls_and_the_constant():
    from zksnap_circuits_halo2_amd import _lib

    for name in NAMES:
        assert AH.params(name) == HEADER[name]
    assert AH.defines()["ZKHIP_MAX_PAIRS"] == 64 == _lib.ZKHIP_MAX_PAIRS
    assert AH.params("zkhip_test_fq12_op") == ["int op", "const uint64_t *a", "const uint64_t *b", "uint64_t *out"]


def test_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "zkhip.h")).read().replace("\n *", " ").split())
    for needle in ("(0,0) = identity", "contributes 1", "n = 0 gives 1", "NOT checked", "ZKHIP_EINVAL", "only the verdict leaves the device", "16-byte aligned"):
        assert needle in text, needle


def test_cpp_mirror_and_rust_shim_agree_with_the_header():
    hpp = open(os.path.join(ROOT, "include", "zkhip.hpp")).read()
    assert re.search(r"inline bool pairing_check\(const std::vector<G1Affine>& g1, const std::vector<G2Affine>& g2\)", hpp)
    assert re.search(r"\bzkhip_pairing_check\([^;]*\)\s*,\s*\"pairing_check\"", hpp) and AH.hpp_call_arities(NAMES[0]) == [len(HEADER[NAMES[0]])]
    for name in ("inline bool verify_opening(", "class VerifierGWC", "class VerifierSHPLONK", "struct VerifierQuery"):
        assert name in hpp, name
    ffi = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust-shim", "zkhip_ffi.rs")).read())
    for name in NAMES:
        assert AH.rust_functions().get(name) == ("c_int", RUST[name]), f"rust-shim/zkhip_ffi.rs does not declare {name} this way"
    assert re.search(r"pub\(crate\) const MAX_PAIRS: usize = 64;", ffi)
    assert re.search(r"pub\(crate\) fn pairing_check<A: 'static, B: 'static>\(g1: &\[A\], g2: &\[B\]\) -> Option<bool>", ffi)
    patch = open(os.path.join(ROOT, "rust-shim", "prover_patch.rs")).read()
    assert "pub(crate) fn verify_on_device<" in patch and "zkhip_ffi::pairing_check(" in patch and "ZKHIP_VERIFY_ON_DEVICE" in patch
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert patch.rstrip() in doc and open(os.path.join(ROOT, "rust-shim", "zkhip_ffi.rs")).read().rstrip() in doc
    from zksnap_circuits_halo2_amd import arithmetic as A, kzg, multiopen as M

    assert callable(A.pairing_check) and callable(kzg.ParamsKZG.verify_opening) and callable(kzg.ParamsKZG.verify)
    assert callable(M.VerifierGWC.verify_proof) and callable(M.VerifierSHPLONK.verify_proof)


def test_library_exports_the_calls(lib):
    for name in NAMES + ("zkhip_test_fq12_op",):
        assert hasattr(lib, name)


def test_more_than_64_pairs_and_null_pointers_are_einval(lib):
    """answered from the arguments alone: nothing is enqueued, no device is needed"""
    ok = C.c_int(7)
    g1, g2 = (C.c_uint64 * (65 * 8))(), (C.c_uint64 * (65 * 16))()
    assert lib.zkhip_pairing_check(g1, g2, 65, C.byref(ok)) == EINVAL
    assert lib.zkhip_pairing_check(None, g2, 1, C.byref(ok)) == EINVAL
    assert lib.zkhip_pairing_check(g1, g2, 1, None) == EINVAL
    assert lib.zkhip_pairing_check_device(g1, g2, 65, g1, None) == EINVAL
    assert lib.zkhip_pairing_check_device(g1, None, 2, g1, None) == EINVAL
    # the `_device` form reads the pairs with 16-byte vector loads: a pointer that is only 8-byte aligned is refused, not loaded from
    base = C.addressof(g1)
    assert base % 16 == 0 or (base + 8) % 16 == 0
    off = 8 if base % 16 == 0 else 0
    assert lib.zkhip_pairing_check_device(C.c_void_p(base + off), C.c_void_p(C.addressof(g2) // 16 * 16), 1, g1, None) == EINVAL
    assert lib.zkhip_pairing_check_device(C.c_void_p(base // 16 * 16), C.c_void_p(C.addressof(g2) // 16 * 16 + 8), 1, g1, None) == EINVAL
    assert lib.zkhip_pairing_check_device(C.c_void_p(base // 16 * 16), C.c_void_p(C.addressof(g2) // 16 * 16), 1, C.c_void_p(base + 2), None) == EINVAL
    assert b"aligned" in lib.zkhip_last_error()
    assert ok.value == 7


def test_host_form_without_a_device_is_enodev():
    """a fresh process that sees no GPU: the host form of a well-formed call answers ZKHIP_ENODEV (n = 0 included: the verdict needs the kernel)"""
    code = (
        "import ctypes as C, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from zksnap_circuits_halo2_amd import _lib\n"
        "lib = _lib.load()\n"
        "ok = C.c_int(7)\n"
        "g1, g2 = (C.c_uint64 * 16)(), (C.c_uint64 * 32)()\n"
        "print(lib.zkhip_pairing_check(g1, g2, 2, C.byref(ok)), lib.zkhip_pairing_check(None, None, 0, C.byref(ok)), ok.value)\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(ENODEV), str(ENODEV), "7"]

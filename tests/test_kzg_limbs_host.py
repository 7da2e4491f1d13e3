"""CPU (`-m "not gpu"`): KZG accumulators, everything of them that needs no device.

  csrc/kzg_limbs.hpp and csrc/row_msm.hpp compiled for the host under ASan + UBSan (tests/cpp/kzg_limbs_host_check.cpp) against Python integers
      (tests/accumulator_reference.py): encode over the coordinates 0, 1, 2^88 - 1, 2^88, 2^176 - 1, 2^176, q - 1 and random ones; decode over
      honest points and every refusal; the header's pins; the row MSM's chunk and stage counts around every switch
  the library's host forms (zkhip_kzg_limbs_encode / _decode) on the same cases, and accumulator.fe_to_limbs / fe_from_limbs
  every ZKHIP_EINVAL of the new calls, in a process that sees no device
  the header's declarations"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import abi_header as AH
import accumulator_reference as AR
from oracle import bn254 as O
from test_identity_host import EINVAL, FAKE, ROOT, SAN, _run
from zksnap_circuits_halo2_amd import _lib

Q, R = O.Q_MOD, O.R_MOD
fq_word = lambda v: f"{O.to_mont(v, Q):x}"
fr_word = lambda v: f"{O.to_mont(v, R):x}"
NAMES = ["zkhip_g1_row_msm_device", "zkhip_kzg_limbs_encode", "zkhip_kzg_limbs_decode", "zkhip_kzg_limbs_encode_device", "zkhip_kzg_limbs_decode_device"]
LANES, MAX_BLOCKS = 64, 1 << 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("kzg_limbs") / "kzg_limbs_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "kzg_limbs_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return str(out)


def _lines(exe, lines):
    run = _run([exe], input="\n".join(lines) + "\n")
    assert run.returncode == 0 and f"kzg limbs host check done: {len(lines)} cases" in run.stdout, run.stdout[-2000:]
    return run.stdout.splitlines()[:-1]


def test_encode_of_the_header_splits_coordinates_as_the_integers_do(exe):
    cases = AR.encode_cases(random.Random("limbs-encode"))
    assert {x for x, _ in cases} >= set(AR.EDGE_COORDINATES)
    out = _lines(exe, [f"enc {fq_word(x)} {fq_word(y)}" for x, y in cases])
    for (x, y), line in zip(cases, out):
        assert [O.from_mont(int(w, 16), R) for w in line.split()] == AR.fe_to_limbs(x) + AR.fe_to_limbs(y), (hex(x), hex(y))
        assert all(int(w, 16) < R for w in line.split())                              # canonical words


def test_decode_of_the_header_is_strict(exe):
    cases = AR.decode_cases(random.Random("limbs-decode"))
    assert {st for _, (st, _) in cases} == {0, 1, 2, 3}
    out = _lines(exe, ["dec " + " ".join(fr_word(v) for v in limbs) for limbs, _ in cases])
    for (limbs, (status, point)), line in zip(cases, out):
        st, x, y = line.split()
        assert int(st) == status, [hex(v) for v in limbs]
        assert (int(x, 16), int(y, 16)) == ((0, 0) if point is None else (O.to_mont(point[0], Q), O.to_mont(point[1], Q))), [hex(v) for v in limbs]


def test_decode_refuses_words_that_are_no_canonical_fr(exe):
    good = [fr_word(v) for v in AR.point_to_limbs((1, 2))]
    for pos in range(6):
        for raw in (R, (1 << 256) - 1):
            words = list(good)
            words[pos] = f"{raw:x}"
            assert _lines(exe, ["dec " + " ".join(words)]) == ["1 " + "0" * 64 + " " + "0" * 64]


def test_the_pins_of_the_header(exe):
    values = [int(w, 16) for w in _lines(exe, ["pins"])[0].split()]
    assert values[:6] == [1, 0, 0, 2, 0, 0]
    assert values[6:] == [0x71ca8d3c208c16d87cfd46, 0x45b68181585d97816a9168, 0x30644e72e131a029b850] == AR.fe_to_limbs(Q - 1)
    text = open(os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc", "kzg_limbs.hpp")).read()
    assert "[1, 0, 0,  2, 0, 0]" in text and "[0x71ca8d3c208c16d87cfd46, 0x45b68181585d97816a9168, 0x30644e72e131a029b850]" in text
    assert "#define ZKHIP_KZG_LIMBS 3" in text and "#define ZKHIP_KZG_LIMB_BITS 88" in text
    assert AH.defines()["ZKHIP_KZG_LIMBS"] == 3 and AH.defines()["ZKHIP_KZG_LIMB_BITS"] == 88


def plan_reference(rows, cols):
    """(valid, chunks, stages, units, grid1, grid2, partial_bytes): the statement of csrc/row_msm.hpp's comment"""
    if cols == 0 or rows * cols > 1 << 31 or rows > 1 << 31 or cols > 1 << 31:
        return [0, 0, 0, 0, 0, 0, 0]
    if rows == 0:
        return [1, 0, 0, 0, 0, 0, 0]
    chunks = -(-cols // LANES)
    two = chunks > 1
    return [1, chunks, 2 if two else 1, rows * chunks, min(rows * chunks, MAX_BLOCKS), min(rows, MAX_BLOCKS) if two else 0, rows * chunks * 144 if two else 0]


def test_row_msm_plan_around_every_switch(exe):
    shapes = [(rows, cols) for rows in (0, 1, 2, 3, 65) for cols in (0, 1, 2, 33, 63, 64, 65, 127, 128, 129, 954, 4095, 4096, 4097)]
    shapes += [(MAX_BLOCKS - 1, 1), (MAX_BLOCKS, 1), (MAX_BLOCKS + 1, 1), (MAX_BLOCKS // 2, 65), (MAX_BLOCKS + 1, 65), (4096, 33), (64, 954)]
    shapes += [(1 << 31, 1), ((1 << 31) + 1, 1), (1, 1 << 31), (1, (1 << 31) + 1), (1 << 16, 1 << 15), ((1 << 16) + 1, 1 << 15), (1 << 40, 1 << 40), (1 << 63, 2)]
    out = _lines(exe, [f"plan {rows} {cols}" for rows, cols in shapes])
    for (rows, cols), line in zip(shapes, out):
        assert [int(v) for v in line.split()] == plan_reference(rows, cols), (rows, cols)


def test_glv_header_is_the_text_of_msm_hip():
    """csrc/glv.hpp restates `namespace glv` of csrc/msm.hip (whose constants tests/test_oracle.py derives): line for line the same body"""
    def body(name):
        lines = open(os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc", name)).read().split("\n")
        return lines[lines.index("namespace glv {") + 1:lines.index("}  // namespace glv")]
    assert body("glv.hpp") == body("msm.hip") and len(body("glv.hpp")) > 60


# ---- the library's host forms --------------------------------------------------------------------------------------------------------------------
def _words(values, p):
    return np.array([O.limbs4(O.to_mont(v, p)) for v in values], dtype=np.uint64)


def test_the_library_host_forms_agree_with_the_integers(lib):
    from zksnap_circuits_halo2_amd import accumulator as A

    enc = AR.encode_cases(random.Random("limbs-lib"))
    pts = _words([c for pair in enc for c in pair], Q).reshape(len(enc), 8)
    out = np.zeros((len(enc), 6, 4), dtype=np.uint64)
    assert lib.zkhip_kzg_limbs_encode(pts.ctypes.data, len(enc), out.ctypes.data) == 0
    assert [[O.fr_from_limbs([int(w) for w in limb]) for limb in row] for row in out] == [AR.fe_to_limbs(x) + AR.fe_to_limbs(y) for x, y in enc]
    assert all(A.fe_to_limbs(x) == AR.fe_to_limbs(x) and A.fe_from_limbs(AR.fe_to_limbs(x)) == x for x, _ in enc)
    dec = AR.decode_cases(random.Random("limbs-lib"))
    limbs = _words([v for case, _ in dec for v in case], R).reshape(len(dec), 6, 4)
    back, status = np.full((len(dec), 8), 0xAB, dtype=np.uint64), np.full(len(dec), 9, dtype=np.uint32)
    assert lib.zkhip_kzg_limbs_decode(limbs.ctypes.data, len(dec), back.ctypes.data, status.ctypes.data) == 0
    assert status.tolist() == [st for _, (st, _) in dec]
    assert [O.affine_from_limbs([int(w) for w in row]) for row in back] == [point for _, (_, point) in dec]
    assert lib.zkhip_kzg_limbs_encode(None, 0, None) == 0 and lib.zkhip_kzg_limbs_decode(None, 0, None, None) == 0
    for bad in ([1 << 88, 0, 0], [0, 0, 1 << 80], AR.fe_to_limbs(Q - 1)[:2] + [AR.fe_to_limbs(Q - 1)[2] + 1], [0, 0]):
        with pytest.raises(ValueError):
            A.fe_from_limbs(bad)
    with pytest.raises(ValueError):
        A.fe_to_limbs(Q)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_calls():
    assert AH.params("zkhip_g1_row_msm_device") == ["const void *d_rows", "size_t n_cols", "const void *d_own_points", "size_t n_own", "size_t own_stride",
                                                    "const void *d_shared_points", "size_t n_rows", "void *d_out_xyz", "void *stream"]
    assert AH.params("zkhip_kzg_limbs_decode_device") == ["const void *d_fr_in", "size_t n", "void *d_affine", "void *d_status", "void *stream"]
    for name in NAMES:
        assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported() and name in AH.rust_functions()
        assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"


def _row_msm(lib, rows=FAKE, n_cols=33, own=FAKE + (1 << 30), n_own=20, stride=20, shared=FAKE + (2 << 30), n_rows=3, out=FAKE + (3 << 30)):
    return lib.zkhip_g1_row_msm_device(rows, n_cols, own, n_own, stride, shared, n_rows, out, None)


def row_msm_refusals(lib):
    """every refusal of the row MSM; a call that reaches the device would read FAKE addresses"""
    assert _row_msm(lib, n_cols=0, n_own=0, stride=0) == EINVAL
    assert _row_msm(lib, n_own=34, stride=34) == EINVAL and _row_msm(lib, stride=19) == EINVAL
    assert _row_msm(lib, n_rows=(1 << 31) // 33 + 1) == EINVAL and _row_msm(lib, n_cols=(1 << 31) + 1, n_rows=1) == EINVAL
    assert _row_msm(lib, stride=(1 << 39) + 1) == EINVAL and _row_msm(lib, stride=(1 << 40) + 1, n_rows=2) == EINVAL      # (n_rows - 1) * own_stride above 2^40 elements
    assert b"2^40" in lib.zkhip_last_error()
    for arg in ("rows", "own", "shared", "out"):
        assert _row_msm(lib, **{arg: None}) == EINVAL and _row_msm(lib, **{arg: FAKE + 8 + (5 << 30)}) == EINVAL, arg
    rows_bytes, own_bytes, out_bytes = 3 * 33 * 32, (2 * 23 + 20) * 64, 3 * 96
    assert _row_msm(lib, out=FAKE + rows_bytes - 16) == EINVAL and _row_msm(lib, rows=FAKE + out_bytes - 16, out=FAKE) == EINVAL
    assert _row_msm(lib, stride=23, out=FAKE + (1 << 30) + own_bytes - 16) == EINVAL
    assert _row_msm(lib, out=FAKE + (2 << 30) + 13 * 64 - 16) == EINVAL
    assert b"g1_row_msm" in lib.zkhip_last_error()
    assert _row_msm(lib, n_rows=0) == 0 and _row_msm(lib, n_rows=0, rows=None, own=None, shared=None, out=None) == 0      # nothing to write: no device asked
    assert lib.zkhip_kzg_limbs_encode_device(None, 1, FAKE, None) == EINVAL and lib.zkhip_kzg_limbs_encode_device(FAKE, 1, FAKE + 8, None) == EINVAL
    assert lib.zkhip_kzg_limbs_encode_device(FAKE, (1 << 31) + 1, FAKE + (1 << 40), None) == EINVAL
    assert lib.zkhip_kzg_limbs_decode_device(FAKE, 1, FAKE + 4096, None, None) == EINVAL and lib.zkhip_kzg_limbs_decode_device(FAKE, 1, FAKE + 4096, FAKE + 8194, None) == EINVAL
    assert lib.zkhip_kzg_limbs_decode_device(FAKE + 8, 1, FAKE + 4096, FAKE + 8192, None) == EINVAL
    assert lib.zkhip_kzg_limbs_encode_device(None, 0, None, None) == 0 and lib.zkhip_kzg_limbs_decode_device(None, 0, None, None, None) == 0
    assert lib.zkhip_kzg_limbs_encode(None, 1, None) == EINVAL and lib.zkhip_kzg_limbs_decode(None, 1, None, None) == EINVAL


def test_the_refusals(lib):
    row_msm_refusals(lib)


def test_the_refusals_and_the_host_forms_need_no_device():
    """a fresh process in which HIP sees no device: the refusals are decided before it would be asked, the host forms never ask"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_kzg_limbs_host as T\n"
            "lib = T._lib.load()\n"
            "T.row_msm_refusals(lib)\n"
            "T.test_the_library_host_forms_agree_with_the_integers(lib)\n"
            "print('refused without a device')\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0 and "refused without a device" in done.stdout, done.stdout + done.stderr

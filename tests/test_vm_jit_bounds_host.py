"""CPU: the run-time compiler of row programs (csrc/rowvm_jit.hip) at its own magnitude thresholds.  Every program of jit_bounds.DIRECTED puts
a register just under or just over one threshold: the generated text must hold exactly the reductions and `Fr::PK_S1` constants the entry
names, pass the worst-case replay `jit_bounds.check_magnitudes` (exact integers against the preconditions of csrc/fp29.hpp, never the
generator's own bounds) and compile with hiprtc; seeded random programs whose bounds climb must pass the replay too.  The borrow-proof
multiples of the moduli that the subtractions use are checked against K p.  On the GPU the same programs run through both executors
(tests/test_gpu_vm_jit_bounds.py)."""
import ctypes as C
import os
import re

import pytest

import jit_bounds as J
from zksnap_circuits_halo2_amd import _lib, fields as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 2000


@pytest.mark.parametrize("name", [d.name for d in J.DIRECTED])
def test_directed_program_reduces_where_its_threshold_says(lib, name):
    d = J.DIRECTED_BY_NAME[name]
    src = J.source_of(lib, d.prog, 2, 6)
    condsub2, soft, pk = J.reductions_of(src)
    print(name, "condsub2", condsub2, "soft", soft, "P", pk)
    assert (condsub2, soft, pk) == (d.condsub2, d.soft, d.pk)
    body = J.kernel_body(src)
    for text in d.contains:
        assert text in body, text
    assert J.check_magnitudes(src) < 3 * J.R
    code = C.c_size_t(0)
    P, keep = d.prog._marshal()
    _lib.check(lib.zkhip_vm_jit_compile(C.byref(P), 2, 6, C.byref(code)))
    del keep
    assert code.value > 1000


def test_directed_table_covers_every_threshold():
    """one entry on each side of every threshold of the generator, and the class whose result is an exact multiple of r"""
    names = set(J.DIRECTED_BY_NAME)
    for pair in (("mul_first_factor_5", "mul_first_factor_6"), ("mul_second_factor_5", "mul_second_factor_6"), ("sqr_2", "sqr_3"), ("sqr_3", "sqr_5"),
                 ("sub_subtrahend_15", "sub_subtrahend_16"), ("neg_15", "neg_16"), ("sub_minuend_40", "sub_minuend_41"), ("dbl_30", "dbl_31"),
                 ("add_30_30", "add_31_30"), ("mad_addend_60", "mad_addend_61"), ("result_bound_3", "result_bound_4"), ("result_bound_4", "result_bound_62"),
                 ("rowpow_by_3", "rowpow_by_4"), ("prev_by_3", "prev_by_4")):
        assert set(pair) <= names, pair
    assert [J.DIRECTED_BY_NAME["sub_subtrahend_%d" % m].pk for m in (1, 2, 3, 5, 7, 9, 11, 15, 16)] == [[2], [3], [4], [6], [8], [10], [12], [16], [4]]
    assert [J.DIRECTED_BY_NAME["neg_%d" % m].pk for m in (1, 2, 3, 5, 7, 9, 11, 15, 16)] == [[2], [3], [4], [6], [8], [10], [12], [16], [4]]
    assert {"neg_of_product", "neg_of_sum", "mov_of_neg_of_product", "mov_of_neg_of_sum", "x_minus_x_1", "x_minus_x_2", "x_minus_x_5",
            "register_read_before_written"} <= names


def test_the_replay_refuses_what_the_preconditions_forbid():
    """check_magnitudes on hand-written kernels: the value that is exactly 3r, a borrow, a repack of 2^256, an unknown statement"""
    head = 'extern "C" __global__ void k(const jit_args A) {\n  fe r0 = fe_zero(), r1 = fe_zero();\n'
    tail = "  { uint32_t w[8]; fe_pack(fe_canon_lt3p<Fr>(r1), w); store_words(A.out + row * 8, w); }\n}\n"
    load = "  const fe t0 = ldx<0>(A.cols[0], (row + 0ull) & (A.rows - 1));\n"
    ok = head + load + "  r0 = t0;\n  r1 = fe_norm(fe_sub_red(t0, r0, Fr::P2_S1));\n" + tail
    assert J.check_magnitudes(ok) == 3 * J.R - 1
    with pytest.raises(J.MagnitudeError, match="exactly 3 r"):
        J.check_magnitudes(head + load + "  r0 = t0;\n  r1 = fe_norm(fe_neg_red(r0, Fr::P3_S1));\n" + tail)
    with pytest.raises(J.MagnitudeError, match="borrows"):
        J.check_magnitudes(head + load + "  r0 = fe_norm(fe_add(t0, t0));\n  r1 = fe_norm(fe_neg_red(r0, Fr::P2_S1));\n  r1 = condsub2(r1);\n" + tail)
    six = "  r0 = fe_norm(fe_dbl(t0));\n  r0 = fe_norm(fe_add(r0, fe_norm(fe_dbl(r0))));\n"
    with pytest.raises(J.MagnitudeError, match="2\\^256"):
        J.check_magnitudes(head + load + six + "  r1 = fe_mul<Fr, false>(t0, times32(r0));\n" + tail)
    with pytest.raises(J.MagnitudeError, match="condsub2"):
        J.check_magnitudes(head + load + six + "  r1 = condsub2(r0);\n" + tail)
    with pytest.raises(J.MagnitudeError, match="scaled"):
        J.check_magnitudes(head + load + "  r1 = fe_mul<Fr, false>(t0, t0);\n" + tail)
    with pytest.raises(ValueError):
        J.check_magnitudes(head + load + "  r1 = fe_canon<Fr>(t0);\n" + tail)
    # condsub2 gives 2r only for an input that can be exactly 4r; fe_reduce_soft stays below 2r + 2^233
    four = head + load + "  r0 = fe_norm(fe_neg_red(t0, Fr::P4_S1));\n  r0 = condsub2(r0);\n  r1 = r0;\n" + tail
    assert J.check_magnitudes(four) == 2 * J.R
    soft = head + load + six + "  r0 = fe_reduce_soft<Fr>(r0);\n  r1 = r0;\n" + tail
    assert J.check_magnitudes(soft) == 2 * J.R + (1 << 233) - 1


def test_random_programs_with_climbing_bounds_pass_the_replay(lib):
    """seeded programs of up to 256 instructions, skewed towards add / sub / neg / dbl, with and without omega^row and PREV"""
    reduced = large = 0
    for seed in range(N_RANDOM):
        p = J.random_program(seed)
        src = J.source_of(lib, p, 2, 6)
        try:
            top = J.check_magnitudes(src)
        except J.MagnitudeError as e:
            raise AssertionError("seed %d: %s" % (seed, e))
        c, s, _ = J.reductions_of(src)
        reduced += bool(c or s)
        large += top >= 2 * J.R
    print("programs with a reduction:", reduced, "results that can reach 2r:", large)
    assert reduced > N_RANDOM // 2 and large > N_RANDOM // 20               # the programs do reach the thresholds


@pytest.mark.parametrize("field", ["Fq", "Fr"])
def test_borrow_proof_multiples_of_the_modulus(field):
    """bn254_constants.hpp: every PK_S1 is K p, with limbs 0..7 at least 2^29 (so that no limb of `PK_S1 - b`, b in N form, borrows)"""
    text = open(os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc", "bn254_constants.hpp")).read()
    body = re.search(r"struct %sParams \{(.*?)\n\};" % field, text, flags=re.S).group(1)
    mod = F.Q_MOD if field == "Fq" else F.R_MOD
    limbs = lambda s: [int(x.rstrip("u"), 16) for x in s.split(",")]
    value = lambda l: sum(v << (29 * i) for i, v in enumerate(l))
    assert value(limbs(re.search(r"uint32_t P\[9\] = \{([^}]*)\}", body).group(1))) == mod
    found = {int(k): limbs(v) for k, v in re.findall(r"uint32_t P(\d+)_S1\[9\] = \{([^}]*)\}", body)}
    assert sorted(found) == [2, 3, 4, 6, 8, 10, 12, 16, 32, 64]
    for k, l in found.items():
        assert len(l) == 9 and value(l) == k * mod, k
        assert all((1 << 29) <= v < (1 << 32) for v in l[:8]) and l[8] < (1 << 32), k
        # the top limb covers that of any b <= (K-1) p in N form
        assert l[8] >= ((k - 1) * mod) >> 232, k


def test_the_counter_of_compiled_launches_is_exported(lib):
    assert _lib._SIGS["zkhip_test_rows_compiled_count"] == (C.c_uint64, [])
    before = lib.zkhip_test_rows_compiled_count()
    d = J.DIRECTED[0]
    P, keep = d.prog._marshal()
    _lib.check(lib.zkhip_vm_jit_compile(C.byref(P), 2, 6, None))
    del keep
    assert lib.zkhip_test_rows_compiled_count() == before                        # a compile-only run launches nothing

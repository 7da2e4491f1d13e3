"""CPU (`-m "not gpu"`): the quotient identity at x, everything of it that needs no device.

  csrc/identity_points.hpp compiled for the host under ASan + UBSan (tests/cpp/identity_host_check.cpp) against identity_reference.domain_values,
      value by value: k in {1, 3, 13, 28}, usable_rows in {n - 1, n - 6, 1} where the call allows them, x in {0, 1, omega, omega^u, omega^(n-1),
      2, r - 1} and seeded random points; points of the domain raise the flag and give four zeros
  evaluation.identity_program: no rotation, no PREV / ROWPOW, at most ZKHIP_VM_REGS registers, every column below n_evals + 9 -- and, run by a
      twenty-line interpreter on Python integers, the value identity_reference.identity_value computes from the ConstraintSystem directly
  its ValueErrors; the prover's programs still byte for byte what the parent commit exported
  the refusals of the two C calls: ZKHIP_EINVAL, decided on the host in a process that never initialises HIP"""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import pytest

import abi_header as AH
import identity_reference as IR
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F, prover as P, verifier as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
R = F.R_MOD
EINVAL = -1
FAKE = 0x7000_0000_1000           # a non-null, 64-byte aligned address nothing lives at: a refused call never reads it
SHAPES = [(1, 1), (3, 2), (2, 0), (5, 3)]


def _run(cmd, **kw):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600, **kw)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("identity") / "identity_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "identity_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return str(out)


def domain_cases():
    """(k, u, x) over the shapes and the edge points; u where 1 <= u < n and n - u <= 64"""
    rng = random.Random("identity-points")
    cases = []
    for k in (1, 3, 13, 28):
        n, w = 1 << k, F.omega_for(k)
        for u in sorted({n - 1, n - 6, 1}):
            if not (1 <= u < n and n - u <= 64):
                continue
            points = [0, 1, w, pow(w, u, R), pow(w, n - 1, R), 2, R - 1] + [rng.randrange(R) for _ in range(6)]
            points += [pow(w, u + 1, R), pow(w, rng.randrange(n), R)]                # a blinding row's point (or omega^0), any power
            cases += [(k, u, x) for x in points]
    return cases


def test_domain_values_of_the_header_agree_with_python_integers(exe):
    cases = domain_cases()
    assert {k for k, _, _ in cases} == {1, 3, 13, 28} and len(cases) >= 100
    lines = "".join(f"{k} {u} {F.omega_for(k):x} {pow(1 << k, R - 2, R):x} {x:x}\n" for k, u, x in cases)
    run = _run([exe], input=lines)
    assert run.returncode == 0 and f"identity host check done: {len(cases)} cases" in run.stdout, run.stdout
    flagged = 0
    for (k, u, x), line in zip(cases, run.stdout.splitlines()):
        *values, flag = line.split()
        xn, l0, l_last, l_active, inside = IR.domain_values(x, k, u)
        assert int(flag) == int(inside), (k, u, hex(x))
        assert [int(v, 16) for v in values] == ([0, 0, 0, 0] if inside else [xn, l0, l_last, l_active]), (k, u, hex(x))
        flagged += int(flag)
    assert flagged >= 4 * 7                                                          # 1, omega, omega^u, omega^(n-1) ... of every (k, u)


def test_the_reference_domain_values_are_the_lagrange_basis():
    """the closed form against the defining property, where the domain is small enough to interpolate: sum_i l_i(x) p(omega^i) = p(x)"""
    k, n, w, rng = 3, 8, F.omega_for(3), random.Random(3)
    coeffs = [rng.randrange(R) for _ in range(n)]
    p = lambda t: sum(c * pow(t, i, R) for i, c in enumerate(coeffs)) % R
    for x in (0, 2, R - 1, rng.randrange(R), w, pow(w, 5, R)):
        assert sum(IR.lagrange(i, x, k) * p(pow(w, i, R)) for i in range(n)) % R == p(x)
    xn, l0, l_last, l_active, inside = IR.domain_values(5, k, 2)
    assert not inside and (l_active + sum(IR.lagrange(i, 5, k) for i in range(2, n))) % R == 1 and l_last == IR.lagrange(2, 5, k) and l0 == IR.lagrange(0, 5, k)


# ---- the program -------------------------------------------------------------------------------------------------------------------------------
def plan_of(cs, gate_cols, lookups, k, order="halo2", random_poly=True):
    return P.opening_plan(cs, gate_cols, lookups, (1 << k) - (cs.blinding_factors + 1), random_poly, order)


def interpret(prog, columns):
    """a RowProgram over one row of Python integers"""
    regs = [0] * _lib.VM_REGS

    def value(o):
        kind, index, rot = o
        if kind == E.SRC_COLUMN:
            assert prog.rotations[rot] == 0
            return columns[index]
        return {E.SRC_CONST: prog.constants, E.SRC_REG: regs}[kind][index]

    for op, dst, a, b, c in prog.insns:
        regs[dst] = {E.OP_MOV: lambda: value(a), E.OP_ADD: lambda: value(a) + value(b), E.OP_SUB: lambda: value(a) - value(b), E.OP_MUL: lambda: value(a) * value(b),
                     E.OP_NEG: lambda: -value(a), E.OP_DBL: lambda: 2 * value(a), E.OP_SQR: lambda: value(a) ** 2, E.OP_MAD: lambda: value(a) * value(b) + value(c)}[op]() % R
    return regs[prog.result_reg]


@pytest.mark.parametrize("gate_cols, lookups", SHAPES + [(256, 8)])
def test_identity_program_names_one_row_of_columns_and_nothing_else(gate_cols, lookups):
    k = 13 if gate_cols > 8 else 7
    cs = E.halo2_lib_shape(gate_cols, lookups)
    plan = plan_of(cs, gate_cols, lookups, k)
    prog = E.identity_program(cs, plan, k)
    assert prog.rotations == [0] and prog.rot_scale == 1 and prog.omega is None
    assert prog.registers_used() <= AH.defines()["ZKHIP_VM_REGS"] == _lib.VM_REGS
    operands = [o for ins in prog.insns for o in ins[2:5]]
    assert not any(o[0] in (E.SRC_PREV, E.SRC_ROWPOW) for o in operands)
    columns = {o[1] for o in operands if o[0] == E.SRC_COLUMN}
    assert max(columns) < len(plan) + 9 == prog.n_columns
    # beta, gamma, y, x and every derived column are read; theta is not: these lookups compress ONE expression each (theta^0)
    assert {len(plan) + j for j in range(9)} - columns == {len(plan) + E.ID_THETA}
    assert ("random", 0, 0) in plan and plan.index(("random", 0, 0)) not in columns   # the vanishing argument's random polynomial is no part of the identity
    unread = {("random", 0, 0)} | ({("fixed", gate_cols + 1, 0)} if lookups == 0 else set())      # ... nor is the table of a circuit without lookups
    assert {plan[i] for i in set(range(len(plan))) - columns} == unread              # every other evaluation is


@pytest.mark.parametrize("gate_cols, lookups", SHAPES)
@pytest.mark.parametrize("order", ["halo2", "seeded"])
def test_identity_program_computes_what_the_reference_computes(gate_cols, lookups, order):
    k, rng = 7, random.Random(f"{gate_cols}-{lookups}-{order}")
    cs = E.halo2_lib_shape(gate_cols, lookups)
    plan = plan_of(cs, gate_cols, lookups, k, order, random_poly=order == "halo2")
    prog = E.identity_program(cs, plan, k)
    for _ in range(4):
        evals, challenges = [rng.randrange(R) for _ in plan], tuple(rng.randrange(R) for _ in range(5))
        derived = list(IR.device_domain_values(challenges[4], k, (1 << k) - 6))
        assert interpret(prog, evals + list(challenges) + derived) == IR.identity_value(cs, plan, k, evals, challenges) != 0
        solved = IR.solve_h0(cs, plan, k, evals, challenges)
        assert interpret(prog, solved + list(challenges) + derived) == 0 and IR.status(cs, plan, k, solved, challenges) == 0


def test_identity_program_compresses_a_lookup_of_two_expressions_with_theta():
    k, rng = 7, random.Random("theta")
    cs = E.halo2_lib_shape(2, 1)
    cs.lookups = [E.Lookup([E.Advice(2), E.Advice(0, 1) * E.Fixed(0)], [E.Fixed(3), E.Fixed(2) * 5])]
    plan = plan_of(cs, 2, 1, k)
    prog = E.identity_program(cs, plan, k)
    assert len(plan) + E.ID_THETA in {o[1] for ins in prog.insns for o in ins[2:5] if o[0] == E.SRC_COLUMN}
    evals, challenges = [rng.randrange(R) for _ in plan], tuple(rng.randrange(R) for _ in range(5))
    derived = list(IR.device_domain_values(challenges[4], k, (1 << k) - 6))
    assert interpret(prog, evals + list(challenges) + derived) == IR.identity_value(cs, plan, k, evals, challenges) != 0


def test_identity_program_refuses_what_is_not_built_and_what_is_not_opened():
    k, cs = 7, E.halo2_lib_shape(3, 2)
    plan = plan_of(cs, 3, 2, k)
    for missing in (("advice", 1, 2), ("perm", 0, (1 << k) - 6), ("lookup_pa", 1, -1), ("sigma", 4, 0), ("h", 1, 0)):
        with pytest.raises(ValueError, match=f"{missing[0]} {missing[1]} at rotation"):
            E.identity_program(cs, [t for t in plan if t != missing], k)
    with pytest.raises(ValueError, match="instance columns"):
        E.identity_program(E.ConstraintSystem(num_fixed=1, num_advice=1, num_instance=1, gates=[[E.Advice(0) - E.Instance(0)]]), [("advice", 0, 0)], k)
    with pytest.raises(ValueError, match="instance columns"):
        E.identity_program(E.ConstraintSystem(num_fixed=1, num_advice=1, gates=[[E.Advice(0)]], permutation_columns=[("instance", 0)]), [("advice", 0, 0)], k)
    with pytest.raises(ValueError, match="Challenge"):
        E.identity_program(E.ConstraintSystem(num_fixed=1, num_advice=1, gates=[[E.Advice(0) * E.Challenge(0)]]), [("advice", 0, 0)] + [("h", i, 0) for i in range(3)], k)


def test_a_key_without_its_constraint_system_cannot_verify():
    from zksnap_circuits_halo2_amd import keygen as KG
    import numpy as np

    vk = KG.VerifyingKey(7, np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 8), dtype=np.uint64))
    with pytest.raises(ValueError, match="constraint system"):
        V.identity_program_of(vk, [("h", i, 0) for i in range(3)], 7)
    with pytest.raises(ValueError, match="constraint system"):
        V.verify_transcript_proof(None, vk, 7, b"", {"advice": 0, "lookups": 0, "permutation_sets": 0, "random_poly": False}, [("h", i, 0) for i in range(3)])
    vk.cs = E.halo2_lib_shape(1, 1)
    plan = plan_of(vk.cs, 1, 1, 7)
    assert V.identity_program_of(vk, plan, 7) is V.identity_program_of(vk, list(plan), 7)      # compiled once per (key, plan)


def test_the_prover_programs_are_the_bytes_of_the_parent_commit():
    assert hashlib.sha256(E.export_prover_programs(7, 3, 2)).hexdigest() == "c9270be301a873f101c68962977a681117bcb96e5b436454b79d25c6ba8b653e"


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_calls():
    assert AH.params("zkhip_fr_domain_points_device") == ["uint32_t k", "uint32_t usable_rows", "const uint64_t omega[4]", "const void *d_x", "size_t n_points",
                                                          "void *d_out", "void *stream"]
    assert AH.params("zkhip_verify_identity_device") == ["const zkhip_vm_program *prog", "const void *d_evals", "uint32_t n_evals", "const void *d_challenges", "uint32_t k",
                                                         "uint32_t usable_rows", "const uint64_t omega[4]", "size_t n_proofs", "void *d_status", "void *d_report", "void *stream"]
    for name in ("zkhip_fr_domain_points_device", "zkhip_verify_identity_device"):
        assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported() and name in AH.rust_functions()
        assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    section = text[text.index("---- the quotient identity at x"):text.index("---- parity hooks")]
    for words in ("columns n_evals + 0 .. 4 are theta, beta, gamma, y, x", "columns n_evals + 5 .. 8 are x^n, l_0(x), l_last(x), l_active(x)"):
        assert words in " ".join(section.replace(" * ", " ").split()), words


def _program(mutate=None, n_evals=None):
    """(marshalled identity program of the (1, 1) shape, keep-alive, n_evals); mutate(RowProgram) edits it first"""
    cs = E.halo2_lib_shape(1, 1)
    plan = plan_of(cs, 1, 1, 7)
    prog = E.identity_program(cs, plan, 7)
    if mutate:
        mutate(prog)
    return prog._marshal(), len(plan) if n_evals is None else n_evals


def _verify(lib, marshalled, n_evals, k=7, u=122, omega=None, proofs=3, evals=FAKE, challenges=FAKE + (1 << 24), status=FAKE + (2 << 24), report=FAKE + (3 << 24), prog_null=False,
            omega_null=False):
    (prog, keep), w = marshalled, F.fr_encode([F.omega_for(k) if omega is None else omega])[0]
    return lib.zkhip_verify_identity_device(None if prog_null else C.byref(prog), evals, n_evals, challenges, k, u, None if omega_null else w.ctypes.data, proofs, status,
                                            report, None)


def test_verify_identity_refusals(lib):
    good, n = _program()
    assert _verify(lib, good, n, prog_null=True) == EINVAL and _verify(lib, good, n, omega_null=True) == EINVAL
    assert _verify(lib, good, n, proofs=0, report=None) == EINVAL                     # an empty batch still names its report
    assert _verify(lib, good, n - 1) == EINVAL                                        # the program names column n_evals + 8 of the longer record
    assert _verify(lib, good, 0) == EINVAL
    assert _verify(lib, good, 65536 - 8) == EINVAL                                    # n_evals + 9 > 65536
    for k, u in ((29, 5), (7, 0), (7, 128), (7, 63), (13, 1)):                        # k > 28; u < 1; u >= n; n - u > 64 twice
        assert _verify(lib, good, n, k=k, u=u, omega=F.omega_for(min(k, 28))) == EINVAL, (k, u)
    assert _verify(lib, good, n, proofs=(1 << 24) + 1) == EINVAL
    for arg in ("evals", "challenges", "status", "report"):
        assert _verify(lib, good, n, **{arg: None}) == EINVAL, arg
    assert _verify(lib, good, n, evals=FAKE + 8) == EINVAL and _verify(lib, good, n, challenges=FAKE + 8) == EINVAL
    assert _verify(lib, good, n, status=FAKE + 2) == EINVAL and _verify(lib, good, n, report=FAKE + 4) == EINVAL

    def rotate(p):
        p.rotations[0] = 1
    def unused_rotation(p):
        p.rotations.append(-1)                                                        # in the table, named by no instruction: still sizes the halos
    def prev(p):
        p.emit(E.OP_ADD, p.result_reg, E.RowProgram.reg(p.result_reg), E.RowProgram.PREV)
    def rowpow(p):
        p.omega = F.omega_for(7)
        p.emit(E.OP_MUL, p.result_reg, E.RowProgram.reg(p.result_reg), E.RowProgram.ROWPOW)
    def far_column(p):
        p.emit(E.OP_ADD, p.result_reg, E.RowProgram.reg(p.result_reg), (E.SRC_COLUMN, n + 9, 0))
    for mutate in (rotate, unused_rotation, prev, rowpow, far_column):
        bad, _ = _program(mutate)
        assert _verify(lib, bad, n) == EINVAL, mutate.__name__
        assert b"verify_identity" in lib.zkhip_last_error() or b"eval_rows" in lib.zkhip_last_error()


def test_domain_points_refusals(lib):
    w = F.fr_encode([F.omega_for(7)])[0].ctypes.data
    call = lambda k=7, u=122, omega=w, x=FAKE, points=4, out=FAKE + (1 << 24): lib.zkhip_fr_domain_points_device(k, u, omega, x, points, out, None)
    assert call(k=29) == EINVAL and call(u=0) == EINVAL and call(u=128) == EINVAL and call(u=63) == EINVAL and call(k=13, u=1) == EINVAL
    assert call(points=0) == EINVAL and call(points=(1 << 30) + 1) == EINVAL
    assert call(omega=None) == EINVAL and call(x=None) == EINVAL and call(out=None) == EINVAL
    assert call(x=FAKE + 8) == EINVAL and call(out=FAKE + 4) == EINVAL
    import numpy as np
    big = np.array([0x43e1f593f0000001, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029], dtype=np.uint64)      # r itself: not canonical
    assert call(omega=big.ctypes.data) == EINVAL


def test_the_refusals_need_no_device():
    """a fresh process in which HIP sees no device: the refusals are decided before it would be asked"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_identity_host as T\n"
            "lib = T._lib.load()\n"
            "good, n = T._program()\n"
            "assert T._verify(lib, good, n - 1) == -1 and T._verify(lib, good, n, u=63) == -1 and T._verify(lib, good, n, report=None) == -1\n"
            "w = T.F.fr_encode([T.F.omega_for(7)])[0].ctypes.data\n"
            "assert lib.zkhip_fr_domain_points_device(7, 63, w, T.FAKE, 4, T.FAKE + 4096, None) == -1\n"
            "print('refused without a device')\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0 and "refused without a device" in done.stdout, done.stdout + done.stderr

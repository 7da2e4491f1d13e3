"""CPU (`-m "not gpu"`): instance columns (public inputs) in the verifier, everything of them that needs no device.

  csrc/instance_evals.hpp compiled for the host under ASan + UBSan (tests/cpp/instance_evals_host_check.cpp), the lane groups of the kernel
      emulated lane by lane for G in {1, 4, 16}, against instance_reference.evaluation (the defining sum on Python integers): k in {1, 3, 7, 28},
      len in {0, 1, G - 1, G, G + 1, 2 G + 1} and 2^k at k = 3, 7, rotations {0, 1, n - 1, n - 3}, values all 0, all 1, all r - 1 and random,
      points of the domain give zero
  evaluation.instance_queries / identity_program(..., instance_queries=...), run by test_identity_host's interpreter, against
      instance_reference.identity_value: a gate reading Instance(0, 1), an instance permutation column, a missing query, None
  the refusals of the two C calls: ZKHIP_EINVAL, decided on the host in a process that never initialises HIP"""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import abi_header as AH
import identity_reference as IR
import instance_reference as NR
from test_identity_host import EINVAL, FAKE, ROOT, SAN, _run, interpret, plan_of
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F

R = F.R_MOD
mont = lambda v: f"{(v << 256) % R:x}"             # the external word of v: what the device loads


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("instance") / "instance_evals_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "instance_evals_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return str(out)


def group_cases():
    """(G, k, rot, x, values): the issue's grid; every (k, len, rot) once per value pattern off the domain and once on it"""
    rng = random.Random("instance-evals")
    cases = []
    for k in (1, 3, 7, 28):
        n, w = 1 << k, F.omega_for(k)
        for G in (1, 4, 16):
            lens = {0, 1, G - 1, G, G + 1, 2 * G + 1} | ({n} if k in (3, 7) else set())
            for length in sorted(l for l in lens if l <= n):
                for rot in sorted({0, 1 % n, n - 1, (n - 3) % n}):
                    for values in ([0] * length, [1] * length, [R - 1] * length, [rng.randrange(R) for _ in range(length)]):
                        cases.append((G, k, rot, rng.choice([2, R - 1, rng.randrange(R), rng.randrange(R)]), values))
                    cases.append((G, k, rot, pow(w, rng.randrange(n), R), [rng.randrange(R) for _ in range(length)]))
                    cases.append((G, k, rot, 0, [rng.randrange(R) for _ in range(length)]))
    return cases


def test_lane_groups_of_the_header_agree_with_the_defining_sum(exe):
    cases = group_cases()
    assert {(G, k) for G, k, *_ in cases} == {(G, k) for G in (1, 4, 16) for k in (1, 3, 7, 28)}
    assert {len(v) for G, k, _, _, v in cases if G == 16 and k == 7} == {0, 1, 15, 16, 17, 33, 128}
    lines = []
    for G, k, rot, x, values in cases:
        w = F.omega_for(k)
        lines.append(" ".join([str(G), str(k), str(rot), str(len(values)), mont(w), mont(pow(w, G, R)), mont(pow(1 << k, R - 2, R)), mont(x)] + [mont(v) for v in values]))
    run = _run([exe], input="\n".join(lines) + "\n")
    assert run.returncode == 0 and f"instance host check done: {len(cases)} cases" in run.stdout, run.stdout[-2000:]
    memo, in_domain, wrapped = {}, 0, 0
    for (G, k, rot, x, values), line in zip(cases, run.stdout.splitlines()):
        key = (k, rot, x, tuple(values))
        if key not in memo:
            memo[key] = NR.device_evaluation(values, rot, x, k)
        assert int(line, 16) == memo[key], (G, k, rot, len(values), hex(x))
        in_domain += pow(x, 1 << k, R) == 1
        wrapped += bool(values) and rot > 0 and memo[key] != 0
    assert in_domain >= 100 and wrapped >= 300                    # the zeros of the domain and the indices that wrap below zero were both exercised


def test_the_reference_evaluation_is_the_polynomial_through_the_values():
    """the defining sum against interpolation: e(rot) = p(x omega^rot) for the p of degree < n with p(omega^i) = v_i, zeros behind the values"""
    k, n, w, rng = 3, 8, F.omega_for(3), random.Random(8)
    coeffs = [rng.randrange(R) for _ in range(n)]
    p = lambda t: sum(c * pow(t, i, R) for i, c in enumerate(coeffs)) % R
    values = [p(pow(w, i, R)) for i in range(n)]
    for x in (2, R - 1, rng.randrange(R)):
        for rot in (0, 1, n - 1, n - 3):
            assert NR.evaluation(values, rot, x, k) == p(x * pow(w, rot, R) % R)
    assert NR.evaluation([], 1, 5, k) == 0 and NR.device_evaluation(values, 0, w, k) == 0 and NR.evaluation(values, 0, w, k) == values[1]


# ---- the program -------------------------------------------------------------------------------------------------------------------------------
def _instance_systems():
    """a halo2-lib shape with one public column tied in by the permutation, and the same with a gate that reads Instance(0, 1) and Instance(1)"""
    perm_only = E.halo2_lib_shape(2, 1, instances=1)
    gated = E.halo2_lib_shape(2, 1, instances=2)
    gated.gates = gated.gates + [[E.Fixed(0) * (E.Advice(0) - E.Instance(0, 1)) + E.Instance(1) * E.Advice(1, 1)]]
    return perm_only, gated


def test_halo2_lib_shape_appends_the_instance_columns_behind_the_constants():
    assert E.halo2_lib_shape(3, 2).permutation_columns == E.halo2_lib_shape(3, 2, instances=0).permutation_columns and E.halo2_lib_shape(3, 2).num_instance == 0
    cs = E.halo2_lib_shape(3, 2, instances=2)
    assert cs.num_instance == 2 and cs.permutation_columns[-3:] == [("fixed", 3), ("instance", 0), ("instance", 1)]
    assert cs.permutation_columns[:-2] == E.halo2_lib_shape(3, 2).permutation_columns


def test_instance_queries_are_the_expressions_reads_then_the_permutation_columns():
    perm_only, gated = _instance_systems()
    assert E.instance_queries(E.halo2_lib_shape(2, 1)) == []
    assert E.instance_queries(perm_only) == [(0, 0)]
    assert E.instance_queries(gated) == [(0, 1), (1, 0), (0, 0)]                     # (1, 0) is named by the gate first and by the permutation again: once


@pytest.mark.parametrize("which", ["permutation", "gate"])
def test_identity_program_with_instance_queries_computes_what_the_reference_computes(which):
    k, rng = 7, random.Random(which)
    cs = _instance_systems()[which == "gate"]
    plan = plan_of(cs, 2, 1, k)
    queries = E.instance_queries(cs)
    prog = E.identity_program(cs, plan, k, instance_queries=queries)
    assert prog.n_columns == len(plan) + 9 + len(queries) and prog.rotations == [0]
    columns = {o[1] for ins in prog.insns for o in ins[2:5] if o[0] == E.SRC_COLUMN}
    assert {len(plan) + 9 + q for q in range(len(queries))} <= columns and max(columns) < prog.n_columns
    for _ in range(3):
        evals, challenges = [rng.randrange(R) for _ in plan], tuple(rng.randrange(R) for _ in range(5))
        instances = [[rng.randrange(R) for _ in range(rng.choice([1, 5, 30]))] for _ in range(cs.num_instance)]
        derived = list(IR.device_domain_values(challenges[4], k, (1 << k) - 6))
        row = lambda ev, inst: ev + list(challenges) + derived + [NR.evaluation(inst[c], rot, challenges[4], k) for c, rot in queries]
        assert interpret(prog, row(evals, instances)) == NR.identity_value(cs, plan, k, evals, challenges, instances) != 0
        solved = NR.solve_h0(cs, plan, k, evals, challenges, instances)
        assert interpret(prog, row(solved, instances)) == 0 and NR.status(cs, plan, k, solved, challenges, instances) == 0
        changed = [list(col) for col in instances]
        changed[0][0] = (changed[0][0] + 1) % R                                      # one public value: the identity no longer holds
        assert interpret(prog, row(solved, changed)) == NR.identity_value(cs, plan, k, solved, challenges, changed) != 0


def test_identity_program_reads_a_query_list_in_any_order_and_by_rotation_mod_n():
    k, rng = 7, random.Random("order")
    cs = _instance_systems()[1]
    plan = plan_of(cs, 2, 1, k)
    queries = [(1, 0), (0, 0), (0, 1 - (1 << k)), (1, 5)]                           # another order, rotation 1 as 1 - n, one query nobody reads
    prog = E.identity_program(cs, plan, k, instance_queries=queries)
    assert prog.n_columns == len(plan) + 9 + 4
    evals, challenges = [rng.randrange(R) for _ in plan], tuple(rng.randrange(R) for _ in range(5))
    instances = [[rng.randrange(R) for _ in range(4)] for _ in range(2)]
    derived = list(IR.device_domain_values(challenges[4], k, (1 << k) - 6))
    row = evals + list(challenges) + derived + [NR.evaluation(instances[c], rot, challenges[4], k) for c, rot in queries]
    assert interpret(prog, row) == NR.identity_value(cs, plan, k, evals, challenges, instances)


def test_identity_program_names_a_missing_query_and_still_refuses_none():
    k = 7
    perm_only, gated = _instance_systems()
    plan = plan_of(gated, 2, 1, k)
    with pytest.raises(ValueError, match="instance 0 at rotation 1"):
        E.identity_program(gated, plan, k, instance_queries=[(0, 0), (1, 0)])
    with pytest.raises(ValueError, match="instance 1 at rotation 0"):
        E.identity_program(gated, plan, k, instance_queries=[(0, 0), (0, 1)])
    with pytest.raises(ValueError, match="instance 0 at rotation 0"):
        E.identity_program(perm_only, plan_of(perm_only, 2, 1, k), k, instance_queries=[])
    for cs in (perm_only, gated):
        with pytest.raises(ValueError, match="instance columns"):
            E.identity_program(cs, plan_of(cs, 2, 1, k), k)
    plain = E.halo2_lib_shape(2, 1)                                                 # without instance columns a list changes nothing but the column count
    a, b = E.identity_program(plain, plan_of(plain, 2, 1, k), k), E.identity_program(plain, plan_of(plain, 2, 1, k), k, instance_queries=[])
    assert a.insns == b.insns and a.constants == b.constants and a.n_columns == b.n_columns


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_instance_calls():
    assert AH.params("zkhip_fr_instance_evals_device") == ["uint32_t k", "const uint64_t omega[4]", "const void *d_x", "const void *d_instances", "const uint32_t *column_lens",
                                                           "uint32_t n_columns", "const uint32_t *query_columns", "const uint32_t *query_rotations", "uint32_t n_queries",
                                                           "size_t n_proofs", "void *d_out", "void *stream"]
    assert AH.params("zkhip_verify_identity_instances_device") == [
        "const zkhip_vm_program *prog", "const void *d_evals", "uint32_t n_evals", "const void *d_challenges", "uint32_t k", "uint32_t usable_rows", "const uint64_t omega[4]",
        "const void *d_instances", "const uint32_t *column_lens", "uint32_t n_columns", "const uint32_t *query_columns", "const uint32_t *query_rotations", "uint32_t n_queries",
        "size_t n_proofs", "void *d_status", "void *d_report", "void *stream"]
    for name in ("zkhip_fr_instance_evals_device", "zkhip_verify_identity_instances_device"):
        assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported() and name in AH.rust_functions()
        assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    section = " ".join(text[text.index("---- the quotient identity at x"):text.index("---- parity hooks")].replace(" * ", " ").split())
    assert "column n_evals + 9 + q is query q" in section and "Not built: instance columns" not in section


def u32s(values):
    return (C.c_uint32 * max(len(values), 1))(*values)


NOT_CANONICAL = (C.c_uint64 * 4)(0x43e1f593f0000001, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029)      # r itself


def _evals_call(lib, k=7, omega=None, omega_null=False, x=FAKE, instances=FAKE + (1 << 24), lens=(5, 3), queries=((0, 0), (1, 127)), proofs=3, out=FAKE + (2 << 24),
                n_columns=None, n_queries=None):
    w = F.fr_encode([F.omega_for(max(1, min(k, 28)))])[0]
    return lib.zkhip_fr_instance_evals_device(k, None if omega_null else (w.ctypes.data if omega is None else C.addressof(omega)), x, instances, u32s(lens), len(lens) if n_columns is None else n_columns,
                                              u32s([c for c, _ in queries]), u32s([r for _, r in queries]), len(queries) if n_queries is None else n_queries, proofs, out, None)


def test_instance_evals_refusals(lib):
    call = lambda **kw: _evals_call(lib, **kw)
    assert call(k=29) == EINVAL and call(k=0, queries=((0, 0),), lens=(1,)) == EINVAL and call(omega_null=True) == EINVAL and call(omega=NOT_CANONICAL) == EINVAL
    assert call(lens=(1,) * 65) == EINVAL and call(queries=((0, 0),) * 65) == EINVAL                 # more than 64 columns; more than 64 queries
    assert call(n_columns=65) == EINVAL and call(n_queries=65) == EINVAL
    assert call(queries=((2, 0),)) == EINVAL                                                         # a query column >= n_columns
    assert call(queries=((0, 128),)) == EINVAL and call(k=3, lens=(5, 3), queries=((0, 8),)) == EINVAL      # a rotation >= 2^k
    assert call(lens=(129, 3)) == EINVAL and call(k=3, lens=(5, 9), queries=((0, 0),)) == EINVAL     # len_c > 2^k
    assert call(proofs=(1 << 24) + 1) == EINVAL
    for arg in ("x", "instances", "out"):
        assert call(**{arg: None}) == EINVAL and call(**{arg: FAKE + 8}) == EINVAL, arg
    assert b"fr_instance_evals" in lib.zkhip_last_error()
    # nothing to write: no pointer is named, nothing is enqueued, the device is never asked
    assert call(proofs=0, x=None, instances=None, out=None) == 0 and call(queries=(), lens=(), x=None, instances=None, out=None) == 0


def _identity_call(lib, marshalled, n_evals, k=7, u=122, proofs=3, evals=FAKE, challenges=FAKE + (1 << 24), status=FAKE + (2 << 24), report=FAKE + (3 << 24),
                   instances=FAKE + (4 << 24), lens=(5,), queries=((0, 0),), n_columns=None, n_queries=None):
    (prog, keep), w = marshalled, F.fr_encode([F.omega_for(min(k, 28))])[0]
    return lib.zkhip_verify_identity_instances_device(C.byref(prog), evals, n_evals, challenges, k, u, w.ctypes.data, instances, u32s(lens), len(lens) if n_columns is None else n_columns,
                                                      u32s([c for c, _ in queries]), u32s([r for _, r in queries]), len(queries) if n_queries is None else n_queries, proofs,
                                                      status, report, None)


def _instance_program():
    cs = E.halo2_lib_shape(1, 1, instances=1)
    plan = plan_of(cs, 1, 1, 7)
    return E.identity_program(cs, plan, 7, instance_queries=[(0, 0)])._marshal(), len(plan)


def test_verify_identity_instances_refusals(lib):
    good, n = _instance_program()
    call = lambda **kw: _identity_call(lib, good, n, **kw)
    assert call(lens=(1,) * 65) == EINVAL and call(queries=((0, 0),) * 65) == EINVAL and call(n_columns=65) == EINVAL and call(n_queries=65) == EINVAL
    assert call(queries=((1, 0),)) == EINVAL                                                         # a query column >= n_columns
    assert call(queries=((0, 128),)) == EINVAL                                                       # a rotation >= 2^k
    assert call(lens=(123,)) == EINVAL and b"usable_rows" in lib.zkhip_last_error()                  # len_c > usable_rows: halo2's InstanceTooLarge
    assert call(instances=None) == EINVAL and call(instances=FAKE + 8) == EINVAL
    assert call(queries=()) == EINVAL                                                                # the program names column n_evals + 9: one query short
    # the existing conditions
    assert _identity_call(lib, good, n - 1) == EINVAL and _identity_call(lib, good, 0) == EINVAL and call(proofs=(1 << 24) + 1) == EINVAL
    for k, u in ((29, 5), (7, 0), (7, 128), (7, 63)):
        assert call(k=k, u=u) == EINVAL, (k, u)
    for arg in ("evals", "challenges", "status", "report"):
        assert call(**{arg: None}) == EINVAL, arg
    assert call(evals=FAKE + 8) == EINVAL and call(status=FAKE + 2) == EINVAL and call(report=FAKE + 4) == EINVAL and call(proofs=0, report=None) == EINVAL
    assert b"verify_identity_instances" in lib.zkhip_last_error()


def test_the_instance_refusals_need_no_device():
    """a fresh process in which HIP sees no device: the refusals are decided before it would be asked"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_instance_host as T\n"
            "lib = T._lib.load()\n"
            "T.test_instance_evals_refusals(lib)\n"
            "T.test_verify_identity_instances_refusals(lib)\n"
            "print('refused without a device')\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0 and "refused without a device" in done.stdout, done.stdout + done.stderr

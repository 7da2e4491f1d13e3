"""CPU (`-m "not gpu"`): the batch verifier's scalar side, everything of it that needs no device.

  csrc/gwc_fold.hpp compiled for the host under ASan + UBSan (tests/cpp/gwc_fold_host_check.cpp), a workgroup emulated lane by lane with every
      input unpacked lazily (the kernel's magnitudes): the GWC rows of the three shapes (the voter's 1996 queries included) and both plan orders
      against multiopen.gwc_accumulate, x, v, u also from {1, r - 1} and v = 0, 64 and 256 lanes; the fold lanes and the second level's joins at
      the counts where a lane gains a row, values from {0, 1, r - 1, random}, both signs
  multiopen.gwc_plan against construct_intermediate_sets
  the ZKHIP_EINVAL refusals of the two C calls, decided on the host in a process that never initialises HIP
  the header's declarations and the ctypes mirror of the plan struct"""
import ctypes as C
import os
import random
import subprocess

import pytest

import abi_header as AH
import gwc_reference as GR
from test_identity_host import EINVAL, FAKE, ROOT, SAN, _run
from zksnap_circuits_halo2_amd import _lib, fields as F, multiopen as MO

R = F.R_MOD
mont = lambda v: f"{(v << 256) % R:x}"             # the external word of v: what the device loads
unmont = lambda line: int(line, 16) * pow(1 << 256, R - 2, R) % R


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("gwc_fold") / "gwc_fold_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "gwc_fold_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return str(out)


def _run_cases(exe, lines, n_cases):
    run = _run([exe], input="\n".join(lines) + "\n")
    assert run.returncode == 0 and f"gwc fold host check done: {n_cases} cases" in run.stdout, run.stdout[-2000:]
    return run.stdout.splitlines()[:-1]


def gwc_cases():
    """(triples, plan, k, T, evals, x, v, u)"""
    rng = random.Random("gwc-scalars")
    cases = []
    for gate_cols, lookups, k in GR.SHAPES:
        for order in ("halo2", "seeded"):
            triples = GR.plan_for(gate_cols, lookups, k, order)
            gp = MO.gwc_plan(triples)
            points = [tuple(rng.randrange(1, R) for _ in range(3))]
            if (gate_cols, order) != (256, "seeded"):                    # the long plan once per special point is enough: the lanes do not depend on the order
                points += [(1, 1, 1), (R - 1, R - 1, R - 1), (rng.randrange(1, R), 0, rng.randrange(R)), (1, rng.randrange(R), R - 1)]
            for x, v, u in points:
                for T in ((64, 256) if gate_cols == 1 else (256,)):
                    cases.append((triples, gp, k, T, GR.pick(rng, len(triples)), x, v, u))
    return cases


def test_gwc_lanes_of_the_header_agree_with_gwc_accumulate(exe):
    cases = gwc_cases()
    assert max(len(c[0]) for c in cases) == 1996 and {c[3] for c in cases} == {64, 256}
    lines = []
    for triples, gp, k, T, evals, x, v, u in cases:
        w = F.omega_for(k)
        lines.append(" ".join(["gwc", str(T), str(gp.n_sets), str(gp.n_slots), str(gp.n_evals), mont(x), mont(v), mont(u)] + [mont(pow(w, rot % (1 << k), R)) for rot in gp.set_rotation]))
        lines += [f"{s} {pos} {slot} {mont(e)}" for s, pos, slot, e in zip(gp.query_set, gp.query_pos, gp.query_slot, evals)]
    out = _run_cases(exe, lines, len(cases))
    at = 0
    for triples, gp, k, T, evals, x, v, u in cases:
        row_a, row_c = GR.gwc_rows(triples, gp, k, evals, x, v, u)
        n = len(row_a) + len(row_c)
        assert [int(line, 16) for line in out[at:at + n]] == row_a + row_c, (len(triples), T, hex(x), hex(v), hex(u))
        at += n
    assert at == len(out)


def fold_cases():
    rng = random.Random("fold-rows")
    cases = []
    for count in (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 4095, 4096):
        for negate in (0, 1):
            for T in ((64, 256) if count <= 257 else (256,)):
                cases.append((T, count, negate, GR.pick(rng, count), GR.pick(rng, count)))
    cases.append((256, 300, 0, [R - 1] * 300, [R - 1] * 300))
    cases.append((256, 300, 1, [0] * 300, GR.pick(rng, 300)))
    return cases


def test_fold_lanes_and_joins_of_the_header_agree_with_the_plain_sum(exe):
    cases, lines = fold_cases(), []
    for T, count, negate, r, a in cases:
        lines.append(f"fold {T} {count} {negate} " + " ".join(f"{mont(ri)} {mont(ai)}" for ri, ai in zip(r, a)))
    joins = [(T, count, negate, GR.pick(random.Random(count), count)) for count in (0, 1, 16, 255, 257, 4096) for negate in (0, 1) for T in (256,)]
    for T, count, negate, a in joins:
        lines.append(f"join {T} {count} {negate} " + " ".join(mont(ai) for ai in a))
    scales = [(negate, r, a) for negate in (0, 1) for r in (0, 1, R - 1, 12345) for a in (0, 1, R - 1, R - 2)]
    lines += [f"scale {negate} {mont(r)} {mont(a)}" for negate, r, a in scales]
    out = _run_cases(exe, lines, len(cases) + len(joins) + len(scales))
    want = [(-1) ** negate * sum(ri * ai for ri, ai in zip(r, a)) % R for T, count, negate, r, a in cases]
    want += [(-1) ** negate * sum(a) % R for T, count, negate, a in joins]
    want += [(-1) ** negate * r * a % R for negate, r, a in scales]
    assert [unmont(line) for line in out] == want


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GR.SHAPES)
@pytest.mark.parametrize("order", ["halo2", "seeded"])
def test_gwc_plan_is_construct_intermediate_sets_grouped_by_rotation(shape, order):
    gate_cols, lookups, k = shape
    triples = GR.plan_for(gate_cols, lookups, k, order)
    gp = MO.gwc_plan(triples)
    x, w = random.Random(str(shape)).randrange(1, R), F.omega_for(k)
    queries = GR.queries_of(triples, list(range(len(triples))), x, k)
    sets = MO.construct_intermediate_sets(queries)
    assert not gp.repeated and gp.n_evals == len(triples) and gp.n_sets == len(sets)
    assert [x * pow(w, rot, R) % R for rot in gp.set_rotation] == [point for point, _ in sets]
    for q, query in enumerate(queries):
        assert sets[gp.query_set[q]][1][gp.query_pos[q]] is query
    keys = gp.own_keys + gp.shared_keys
    assert [keys[s] for s in gp.query_slot] == [(kind, idx) for kind, idx, _ in triples] and len(set(keys)) == len(keys) == gp.n_slots
    assert all(kind not in ("fixed", "sigma") for kind, _ in gp.own_keys) and all(kind in ("fixed", "sigma") for kind, _ in gp.shared_keys)
    firsts = [next(i for i, t in enumerate(triples) if t[:2] == key) for key in gp.own_keys]
    assert firsts == sorted(firsts)                                                    # slots in order of first appearance
    struct, keep = gp.marshal(k)
    assert (struct.n_evals, struct.n_sets, struct.n_slots) == (gp.n_evals, gp.n_sets, gp.n_slots) and max(keep[0]) < 1 << k
    if gate_cols == 256:
        assert gp.n_evals == 1996


def test_gwc_plan_flags_a_repeated_triple_and_refuses_rotations_equal_mod_n():
    triples = GR.plan_for(1, 1, 7)
    assert MO.gwc_plan(triples + [triples[3]]).repeated and not MO.gwc_plan(triples).repeated
    colliding = MO.gwc_plan([("advice", 0, 1), ("advice", 1, 1 - 128)])
    with pytest.raises(ValueError, match="equal mod"):
        colliding.marshal(7)
    # both kinds of plan take the verifier's one-by-one path; at k = 8 the two rotations are two sets again
    assert not colliding.foldable(7) and colliding.foldable(8) and MO.gwc_plan(triples).foldable(7) and not MO.gwc_plan(triples + [triples[3]]).foldable(7)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_both_calls_and_the_plan_struct(tmp_path):
    assert AH.params("zkhip_gwc_scalars_device") == ["const zkhip_gwc_plan *plan", "const void *d_evals", "const void *d_points", "uint32_t k", "const uint64_t omega[4]",
                                                     "size_t n_proofs", "void *d_rows_a", "void *d_rows_c", "void *stream"]
    assert AH.params("zkhip_fr_fold_rows_device") == ["const void *d_rows", "uint32_t n_cols", "uint32_t n_own", "const void *d_r", "int negate", "size_t n_rows",
                                                      "void *d_out_own", "void *d_out_shared", "void *stream"]
    for name in ("zkhip_gwc_scalars_device", "zkhip_fr_fold_rows_device"):
        assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported()
        assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"
    assert "zkhip_fr_fold_rows_device" in AH.rust_functions()
    # the plan struct: the C compiler's layout against the ctypes mirror, field by field
    fields = [name for name, _ in _lib.GwcPlan._fields_]
    assert fields == ["n_evals", "n_sets", "n_slots", "reserved", "set_rotation", "query_set", "query_pos", "query_slot"]
    body = "".join(f'printf("%zu %zu\\n", offsetof(zkhip_gwc_plan, {f}), sizeof(((zkhip_gwc_plan *)0)->{f}));' for f in fields)
    src, out = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zkhip.h"\nint main(void) { printf("%zu\\n", sizeof(zkhip_gwc_plan));' + body + " return 0; }\n")
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(out)], check=True)
    lines = subprocess.run([str(out)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0]) == C.sizeof(_lib.GwcPlan) == 48
    for f, line in zip(fields, lines[1:]):
        assert [int(v) for v in line.split()] == [getattr(_lib.GwcPlan, f).offset, getattr(_lib.GwcPlan, f).size], f
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    section = " ".join(text[text.index("---- the batch verifier"):].replace(" * ", " ").split())          # the header's last section
    for words in ("column i < n_sets (witness W_i): u^i x omega^set_rotation[i]", "column n_cols - 1 (G):", "d_rows_c is [n_proofs][n_sets], column j = u^j",
                  "out_own[i][j] = +- r_i rows[i][j]", "with n_rows == 0 the shared part is written as zeros"):
        assert words in section, words
    for doc in ("README.md", "DESIGN.md", os.path.join("zksnap_circuits_halo2_amd", "prover.py"), os.path.join("include", "zkhip.h")):
        assert "BatchVerifier), committed" not in open(os.path.join(ROOT, doc)).read() and "pairing checks into one, as halo2" not in open(os.path.join(ROOT, doc)).read(), doc


def u32s(values):
    return (C.c_uint32 * max(len(values), 1))(*values)


NOT_CANONICAL = (C.c_uint64 * 4)(0x43e1f593f0000001, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029)      # r itself


def _gwc_call(lib, k=7, rot=(0, 1, 127), sets=(0, 1, 2, 0), pos=(0, 0, 0, 1), slots=(0, 1, 2, 0), n_slots=3, n_evals=None, n_sets=None, omega=None, omega_null=False,
              plan_null=False, null_array=None, proofs=3, evals=FAKE, points=FAKE + (1 << 24), rows_a=FAKE + (2 << 24), rows_c=FAKE + (3 << 24)):
    arrays = {"set_rotation": u32s(rot), "query_set": u32s(sets), "query_pos": u32s(pos), "query_slot": u32s(slots)}
    ptr = {name: None if name == null_array else C.cast(a, C.POINTER(C.c_uint32)) for name, a in arrays.items()}
    plan = _lib.GwcPlan(len(sets) if n_evals is None else n_evals, len(rot) if n_sets is None else n_sets, n_slots, 0, ptr["set_rotation"], ptr["query_set"], ptr["query_pos"],
                        ptr["query_slot"])
    w = F.fr_encode([F.omega_for(max(1, min(k, 28)))])[0]
    return lib.zkhip_gwc_scalars_device(None if plan_null else C.byref(plan), evals, points, k, None if omega_null else (w.ctypes.data if omega is None else C.addressof(omega)),
                                        proofs, rows_a, rows_c, None)


def test_gwc_scalars_refusals(lib):
    call = lambda **kw: _gwc_call(lib, **kw)
    assert call(plan_null=True) == EINVAL and call(omega_null=True) == EINVAL and call(omega=NOT_CANONICAL) == EINVAL and call(k=29) == EINVAL
    for name in ("set_rotation", "query_set", "query_pos", "query_slot"):
        assert call(null_array=name) == EINVAL, name
    assert call(n_sets=0) == EINVAL and call(n_sets=65) == EINVAL and call(rot=tuple(range(65)), k=8) == EINVAL          # n_sets outside 1 .. 64
    assert call(n_evals=0) == EINVAL and call(n_evals=65528) == EINVAL                                                   # n_evals outside 1 .. 65527
    assert call(n_slots=0) == EINVAL and call(n_slots=65537) == EINVAL
    assert call(rot=(0, 1, 128)) == EINVAL and call(k=3, rot=(0, 1, 8)) == EINVAL                                        # a rotation >= 2^k
    assert call(sets=(0, 1, 3, 0)) == EINVAL and call(pos=(0, 0, 0, 4)) == EINVAL and call(slots=(0, 1, 3, 0)) == EINVAL  # a query outside its tables
    assert call(proofs=(1 << 24) + 1) == EINVAL
    for arg in ("evals", "points", "rows_a", "rows_c"):
        assert call(**{arg: None}) == EINVAL and call(**{arg: FAKE + 8}) == EINVAL, arg
    assert b"gwc_scalars" in lib.zkhip_last_error()
    # an empty batch names no array, enqueues nothing and never asks the device; a wrong plan is refused all the same
    assert call(proofs=0, evals=None, points=None, rows_a=None, rows_c=None) == 0 and call(proofs=0, n_sets=65) == EINVAL


def _fold_call(lib, n_cols=7, n_own=3, negate=0, n_rows=5, rows=FAKE, r=FAKE + (1 << 24), out_own=FAKE + (2 << 24), out_shared=FAKE + (3 << 24)):
    return lib.zkhip_fr_fold_rows_device(rows, n_cols, n_own, r, negate, n_rows, out_own, out_shared, None)


def test_fold_rows_refusals(lib):
    call = lambda **kw: _fold_call(lib, **kw)
    assert call(n_cols=0, n_own=0) == EINVAL and call(n_cols=65537) == EINVAL and call(n_own=8) == EINVAL
    assert call(negate=2) == EINVAL and call(negate=-1) == EINVAL
    assert call(n_rows=(1 << 24) + 1) == EINVAL and call(n_rows=1 << 24, n_cols=257, n_own=257) == EINVAL                # more than 2^32 elements
    for arg in ("rows", "r", "out_own", "out_shared"):
        assert call(**{arg: None}) == EINVAL and call(**{arg: FAKE + 8}) == EINVAL, arg
    assert call(n_rows=0, out_shared=None) == EINVAL and call(n_rows=0, out_shared=FAKE + 8) == EINVAL                   # the zeros have to go somewhere
    assert b"fr_fold_rows" in lib.zkhip_last_error()
    # pointers that are neither read nor written may be null: no own column, no shared column, no row and no shared column
    assert call(n_own=0, out_own=None, n_rows=(1 << 24) + 1) == EINVAL                                                   # (still refused for its size, not for the pointer)
    assert call(n_cols=3, n_own=3, n_rows=0, rows=None, r=None, out_own=None, out_shared=None) == 0

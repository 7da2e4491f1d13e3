"""CPU (`-m "not gpu"`): the SHPLONK accumulation scalars of the batch verifier, everything of them that needs no device.

  csrc/shplonk_fold.hpp compiled for the host under ASan + UBSan (tests/cpp/shplonk_fold_host_check.cpp), a workgroup emulated lane by lane with
      every input unpacked lazily (the kernel's magnitudes): the rows of the three shapes (the voter's 1996 queries included) and both plan orders
      against multiopen.shplonk_accumulate (tests/shplonk_reference.py), x, y, v, u also from {1, r - 1}, y = 0 and v = 0, 64 and 256 lanes; hand-made
      plans (one set only, sets of one point each, a set of three polynomials); the degenerate proofs: x = 0 and u on a point outside set 0 are
      status 1 with zero rows, u on a point of set 0 is status 0 with the host's rows and an exact zero in the H column
  the closed form the header states, restated in Python integers, against multiopen.shplonk_accumulate
  multiopen.shplonk_plan against construct_rotation_sets, its flags, its slots against gwc_plan's
  the ZKHIP_EINVAL refusals of the C call, decided on the host in a process that never initialises HIP
  the header's declaration and the ctypes mirror of the plan struct"""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import abi_header as AH
import gwc_reference as GR
import shplonk_reference as SR
from test_identity_host import EINVAL, FAKE, ROOT, SAN, _run
from zksnap_circuits_halo2_amd import _lib, fields as F, multiopen as MO

R = F.R_MOD
mont = lambda v: f"{(v << 256) % R:x}"             # the external word of v: what the device loads

HAND_MADE = {
    "one set only": [("advice", 0, 0), ("advice", 0, 1), ("advice", 1, 0), ("advice", 1, 1), ("fixed", 0, 1), ("fixed", 0, 0)],
    "sets of one point each": [("advice", 0, 0), ("advice", 1, 1), ("fixed", 0, -1), ("advice", 2, 5)],
    "a set of three polynomials": [("advice", 0, 0), ("advice", 1, 0), ("advice", 1, 1), ("advice", 2, 0), ("fixed", 0, 0), ("advice", 3, 0), ("advice", 3, 1),
                                   ("advice", 4, 1), ("advice", 4, 0), ("sigma", 0, 0)],
}


def special_points(rng):
    """(x, y, v, u): x, y, v, u each from {1, r - 1}, y = 0, v = 0.  None has u = x omega^rot for a rotation of these plans (u = x is avoided:
    rotation 0 is in every plan), so every one is status 0"""
    rnd = lambda: rng.randrange(2, R - 1)
    return [(1, R - 1, 1, R - 1), (R - 1, 1, R - 1, 1), (rnd(), 0, rnd(), rnd()), (rnd(), rnd(), 0, rnd()), (1, 1, R - 1, rnd()), (rnd(), R - 1, 1, 1),
            (R - 1, rnd(), rnd(), R - 2), (rnd(), 0, 0, R - 1)]


def degenerate_points(rng, sp, k):
    """[(x, y, v, u, status)]: x = 0; u on a point outside set 0 (where the plan has one); u on a point of set 0"""
    w, rnd = F.omega_for(k), lambda: rng.randrange(2, R - 1)
    out = [(0, rnd(), rnd(), rnd(), 1)]
    outside = [t for t in range(sp.n_points) if t not in sp.set_points[0]]
    x = rnd()
    if outside:
        out.append((x, rnd(), rnd(), x * pow(w, sp.point_rotation[outside[-1]] % (1 << k), R) % R, 1))
    out.append((x, rnd(), rnd(), x * pow(w, sp.point_rotation[sp.set_points[0][-1]] % (1 << k), R) % R, 0))
    return out


def closed_form(sp, k, evals, x, y, v, u):
    """the row of A as include/zkhip.h and csrc/shplonk_fold.hpp state it, in Python integers; None where x Z_0 = 0"""
    w = F.omega_for(k)
    wr = [pow(w, rot % (1 << k), R) for rot in sp.point_rotation]
    d = [(u - x * wt) % R for wt in wr]
    prod = lambda values: 1 if not values else values[0] * prod(values[1:]) % R
    z = [prod([d[t] for t in range(sp.n_points) if t not in pts]) for pts in sp.set_points]
    if x * z[0] % R == 0:
        return None
    inv = pow(x * z[0], -1, R)
    norm, xinv = inv * x % R, inv * z[0] % R
    wset = [pow(v, i, R) * z[i] * norm % R for i in range(sp.n_sets)]
    lag = {}
    for i, pts in enumerate(sp.set_points):
        for a in pts:
            c = pow(prod([(wr[a] - wr[b]) % R for b in pts if b != a]), -1, R)
            lag[(i, a)] = wset[i] * prod([d[b] for b in pts if b != a]) * pow(xinv, len(pts) - 1, R) * c % R
    g = -sum(lag[(sp.slot_set[s], t)] * pow(y, sp.slot_pos[s], R) * e for s, t, e in zip(sp.query_slot, sp.query_point, evals)) % R
    return [u % R, -prod(d) * norm % R] + [wset[i] * pow(y, pos, R) % R for i, pos in zip(sp.slot_set, sp.slot_pos)] + [g]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("shplonk_fold") / "shplonk_fold_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "shplonk_fold_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return str(out)


def shplonk_cases():
    """(triples, plan, k, T, evals, x, y, v, u, status)"""
    rng = random.Random("shplonk-scalars")
    cases = []
    for gate_cols, lookups, k in GR.SHAPES:
        for order in ("halo2", "seeded"):
            triples = GR.plan_for(gate_cols, lookups, k, order)
            sp = MO.shplonk_plan(triples)
            points = [tuple(rng.randrange(1, R) for _ in range(4)) + (0,)]
            if gate_cols != 256:                                             # the long plan: the random point in both orders, the degenerate ones in one
                points += [p + (0,) for p in special_points(rng)]
            if (gate_cols, order) != (256, "seeded"):
                points += degenerate_points(rng, sp, k)
            for x, y, v, u, status in points:
                for T in ((64, 256) if gate_cols == 1 else (256,)):
                    cases.append((triples, sp, k, T, GR.pick(rng, len(triples)), x, y, v, u, status))
                    assert status == (closed_form(sp, k, cases[-1][4], x, y, v, u) is None)       # status 1 is x Z_0 = 0, by definition
    for name, triples in HAND_MADE.items():
        sp = MO.shplonk_plan(triples)
        for x, y, v, u, status in [tuple(rng.randrange(1, R) for _ in range(4)) + (0,)] + [p + (0,) for p in special_points(rng)[:4]] + degenerate_points(rng, sp, 7):
            for T in (64, 256):
                cases.append((triples, sp, 7, T, GR.pick(rng, len(triples)), x, y, v, u, status))
                assert status == (closed_form(sp, 7, cases[-1][4], x, y, v, u) is None)
    return cases


def test_the_hand_made_plans_are_what_their_names_say():
    one, singles, three = (MO.shplonk_plan(HAND_MADE[name]) for name in ("one set only", "sets of one point each", "a set of three polynomials"))
    assert one.n_sets == 1 and sorted(one.set_points[0]) == list(range(one.n_points)) == [0, 1]
    assert singles.n_sets == singles.n_points == 4 and all(len(pts) == 1 for pts in singles.set_points)
    assert max(three.slot_pos) >= 2 and three.n_sets == 2 and three.set_points == [[0], [0, 1]]


def test_shplonk_lanes_of_the_header_agree_with_shplonk_accumulate(exe):
    cases = shplonk_cases()
    assert max(len(c[0]) for c in cases) == 1996 and {c[3] for c in cases} == {64, 256} and {c[9] for c in cases} == {0, 1}
    lines = []
    for triples, sp, k, T, evals, x, y, v, u, status in cases:
        w = F.omega_for(k)
        struct, (rot, starts, flat, slot_set, slot_pos, query_slot, query_point) = sp.marshal(k)
        lines.append(" ".join(["shplonk", str(T), str(sp.n_points), str(sp.n_sets), str(sp.n_slots), str(sp.n_evals), mont(x), mont(y), mont(v), mont(u)]
                              + [mont(pow(w, int(r), R)) for r in rot] + [str(s) for s in starts] + [str(t) for t in flat]))
        lines += [f"{s} {pos}" for s, pos in zip(slot_set, slot_pos)]
        lines += [f"{s} {t} {mont(e)}" for s, t, e in zip(query_slot, query_point, evals)]
    run = _run([exe], input="\n".join(lines) + "\n")
    assert run.returncode == 0 and f"shplonk fold host check done: {len(cases)} cases" in run.stdout, run.stdout[-2000:]
    out = run.stdout.splitlines()[:-1]
    at = 0
    for triples, sp, k, T, evals, x, y, v, u, status in cases:
        n = 1 + (2 + sp.n_slots + 1) + 1
        got = [int(line, 16) for line in out[at:at + n]]
        at += n
        where = (len(triples), T, hex(x), hex(y), hex(v), hex(u))
        if status:
            assert got == [1] + [0] * (n - 1), where
            continue
        row_a, row_c = SR.shplonk_rows(triples, sp, k, evals, x, y, v, u)
        assert got == [0] + row_a + row_c, where
        if (u - x * pow(F.omega_for(k), sp.point_rotation[sp.set_points[0][-1]] % (1 << k), R)) % R == 0:
            assert got[2] == 0                                               # u on a point of set 0: Z_T = 0, the H column is an exact zero
    assert at == len(out)


@pytest.mark.parametrize("shape", GR.SHAPES)
@pytest.mark.parametrize("order", ["halo2", "seeded"])
def test_the_closed_form_is_shplonk_accumulate(shape, order):
    k = shape[2]
    triples = GR.plan_for(*shape, order=order)
    sp = MO.shplonk_plan(triples)
    rng = random.Random(f"closed-{shape}-{order}")
    points = [tuple(rng.randrange(1, R) for _ in range(4))] + (special_points(rng)[:4] if shape[0] != 256 else [])
    for x, y, v, u in points:
        evals = GR.pick(rng, len(triples))
        assert closed_form(sp, k, evals, x, y, v, u) == SR.shplonk_rows(triples, sp, k, evals, x, y, v, u)[0], (hex(x), hex(y), hex(v), hex(u))
    assert closed_form(sp, k, GR.pick(rng, len(triples)), 0, 5, 6, 7) is None


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GR.SHAPES)
@pytest.mark.parametrize("order", ["halo2", "seeded"])
def test_shplonk_plan_is_construct_rotation_sets_grouped_by_rotation(shape, order):
    gate_cols, lookups, k = shape
    triples = GR.plan_for(gate_cols, lookups, k, order)
    sp, gp = MO.shplonk_plan(triples), MO.gwc_plan(triples)
    x, w = random.Random(str(shape)).randrange(1, R), F.omega_for(k)
    sets, super_points = MO.construct_rotation_sets(GR.queries_of(triples, list(range(len(triples))), x, k))          # evaluation q = q: a query is known by it
    point = [x * pow(w, rot % (1 << k), R) % R for rot in sp.point_rotation]
    assert not sp.repeated and sp.n_evals == len(triples) and sp.n_sets == len(sets) and sorted(point) == super_points and len(set(point)) == sp.n_points
    assert [sorted(point[t] for t in pts) for pts in sp.set_points] == [rs.points for rs in sets]
    assert (sp.own_keys, sp.shared_keys, sp.query_slot) == (gp.own_keys, gp.shared_keys, gp.query_slot)               # gwc_plan's keys and slots
    keys = sp.own_keys + sp.shared_keys
    for i, rs in enumerate(sets):                                                      # the polynomials of a set, in its order
        members = sorted((sp.slot_pos[s], keys[s]) for s in range(sp.n_slots) if sp.slot_set[s] == i)
        assert [pos for pos, _ in members] == list(range(len(rs.polys))) and [key for _, key in members] == rs.polys
    for q, (s, t) in enumerate(zip(sp.query_slot, sp.query_point)):                    # query q is the evaluation of its polynomial at its point
        rs = sets[sp.slot_set[s]]
        assert t in sp.set_points[sp.slot_set[s]] and rs.evals[sp.slot_pos[s]][rs.points.index(point[t])] == q
    assert sp.n_evals == sum(len(sp.set_points[i]) for i in sp.slot_set)
    struct, keep = sp.marshal(k)
    assert (struct.n_evals, struct.n_sets, struct.n_slots, struct.n_points) == (sp.n_evals, sp.n_sets, sp.n_slots, sp.n_points) and max(keep[0]) < 1 << k
    assert list(keep[1]) == [sum(len(pts) for pts in sp.set_points[:i]) for i in range(sp.n_sets + 1)]
    if order == "seeded":
        assert len(sp.set_points[0]) == 1
    elif gate_cols != 256:
        assert len(sp.set_points[0]) == 4
    if gate_cols == 256:
        assert sp.n_evals == 1996 and sp.n_slots == 947


def test_shplonk_plan_flags_a_repeated_triple_and_refuses_rotations_equal_mod_n():
    triples = GR.plan_for(1, 1, 7)
    assert MO.shplonk_plan(triples + [triples[3]]).repeated and not MO.shplonk_plan(triples).repeated
    colliding = MO.shplonk_plan([("advice", 0, 1), ("advice", 1, 1 - 128)])
    assert colliding.n_points == 2 and colliding.n_sets == 2
    with pytest.raises(ValueError, match="equal mod"):
        colliding.marshal(7)
    # both kinds of plan take the verifier's one-by-one path; at k = 8 the two rotations are two points again
    assert not colliding.foldable(7) and colliding.foldable(8) and MO.shplonk_plan(triples).foldable(7) and not MO.shplonk_plan(triples + [triples[3]]).foldable(7)
    for shape in GR.SHAPES:
        for order in ("halo2", "seeded"):
            t = GR.plan_for(*shape, order=order)
            assert MO.shplonk_plan(t).foldable(shape[2]) == MO.gwc_plan(t).foldable(shape[2]) is True


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_call_and_the_plan_struct(tmp_path):
    name = "zkhip_shplonk_scalars_device"
    assert AH.params(name) == ["const zkhip_shplonk_plan *plan", "const void *d_evals", "const void *d_points", "uint32_t k", "const uint64_t omega[4]", "size_t n_proofs",
                               "void *d_rows_a", "void *d_rows_c", "void *d_status", "void *stream"]
    assert AH.functions()[name][0] == "int" and name in _lib._SIGS and name in AH.exported()
    assert AH.hpp_call_arities(name) == [len(AH.params(name))], f"include/zkhip.hpp mirrors {name} once"
    # the plan struct: the C compiler's layout against the ctypes mirror, field by field
    fields = [field for field, _ in _lib.ShplonkPlan._fields_]
    assert fields == ["n_evals", "n_sets", "n_slots", "n_points", "point_rotation", "set_start", "set_point", "slot_set", "slot_pos", "query_slot", "query_point"]
    body = "".join(f'printf("%zu %zu\\n", offsetof(zkhip_shplonk_plan, {f}), sizeof(((zkhip_shplonk_plan *)0)->{f}));' for f in fields)
    src, out = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zkhip.h"\nint main(void) { printf("%zu\\n", sizeof(zkhip_shplonk_plan));' + body + " return 0; }\n")
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(out)], check=True)
    lines = subprocess.run([str(out)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0]) == C.sizeof(_lib.ShplonkPlan) == 72
    for f, line in zip(fields, lines[1:]):
        assert [int(v) for v in line.split()] == [getattr(_lib.ShplonkPlan, f).offset, getattr(_lib.ShplonkPlan, f).size], f
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    section = " ".join(text[text.index("---- the batch verifier"):].replace(" * ", " ").split())          # the header's last section
    for words in ("column 0 (H'): u", "column 1 (H): - Z_T / Z_0", "column 2 + p (polynomial slot p): w_slot_set[p] y^slot_pos[p]", "column n_cols - 1 (G): - sum_q L_(",
                  "d_rows_c is [n_proofs][1]", "status 1: x Z_0 = 0"):
        assert words in section, words
    for doc in ("README.md", "DESIGN.md", os.path.join("zksnap_circuits_halo2_amd", "prover.py"), os.path.join("include", "zkhip.h")):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        for m in re.finditer(r"Not built|They leave out", text):                   # what follows such words, a few lines of it, no longer names the call
            assert "SHPLONK scalars" not in text[m.start():m.start() + 400], f"{doc} still lists the call as not built"


def u32s(values):
    return (C.c_uint32 * max(len(values), 1))(*values)


NOT_CANONICAL = (C.c_uint64 * 4)(0x43e1f593f0000001, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029)      # r itself
ARRAYS = ("point_rotation", "set_start", "set_point", "slot_set", "slot_pos", "query_slot", "query_point")


def _shplonk_call(lib, k=7, rot=(0, 1, 127), starts=(0, 1, 4), set_point=(0, 0, 1, 2), slot_set=(0, 1, 0), slot_pos=(0, 0, 1), q_slot=(0, 1, 1, 1, 2), q_point=(0, 0, 1, 2, 0),
                  n_evals=None, n_sets=None, n_slots=None, n_points=None, omega=None, omega_null=False, plan_null=False, null_array=None, proofs=3, evals=FAKE,
                  points=FAKE + (1 << 24), rows_a=FAKE + (2 << 24), rows_c=FAKE + (3 << 24), status=FAKE + (4 << 24)):
    """the call over a plan of three points, set 0 = {0} with slots 0 and 2, set 1 = {0, 1, 2} with slot 1, five queries; every argument can be bent"""
    arrays = dict(zip(ARRAYS, (u32s(a) for a in (rot, starts, set_point, slot_set, slot_pos, q_slot, q_point))))
    ptr = [None if name == null_array else C.cast(arrays[name], C.POINTER(C.c_uint32)) for name in ARRAYS]
    plan = _lib.ShplonkPlan(len(q_slot) if n_evals is None else n_evals, len(starts) - 1 if n_sets is None else n_sets, len(slot_set) if n_slots is None else n_slots,
                            len(rot) if n_points is None else n_points, *ptr)
    w = F.fr_encode([F.omega_for(max(1, min(k, 28)))])[0]
    return lib.zkhip_shplonk_scalars_device(None if plan_null else C.byref(plan), evals, points, k, None if omega_null else (w.ctypes.data if omega is None else C.addressof(omega)),
                                            proofs, rows_a, rows_c, status, None)


REFUSED_PLANS = {
    "n_sets = 0": dict(n_sets=0), "n_sets = 65": dict(n_sets=65), "n_points = 0": dict(n_points=0), "n_points = 65": dict(n_points=65),
    "n_evals = 0": dict(n_evals=0), "n_evals = 65528": dict(n_evals=65528), "n_slots = 0": dict(n_slots=0), "n_slots = 65537": dict(n_slots=65537),
    "more than 256 pairs": dict(k=8, rot=tuple(range(64)), starts=(0, 64, 128, 192, 256, 320)),
    "set_start[0] != 0": dict(starts=(1, 2, 4)), "a set without a point": dict(starts=(0, 0, 4)), "set_start falls": dict(starts=(0, 4, 1)),
    "k = 29": dict(k=29), "a rotation = 2^k": dict(rot=(0, 1, 128)), "a rotation >= 2^k at k = 3": dict(k=3, rot=(0, 1, 8)), "a rotation twice": dict(rot=(0, 1, 1)),
    "set_point out of range": dict(set_point=(0, 0, 1, 3)), "a point twice in a set": dict(set_point=(0, 0, 1, 1)),
    "slot_set out of range": dict(slot_set=(0, 2, 0)), "slot_pos = 2^16": dict(slot_pos=(0, 0, 1 << 16)),
    "query_slot out of range": dict(q_slot=(0, 1, 1, 1, 3)), "query_point out of range": dict(q_point=(0, 0, 1, 3, 0)),
    "a point outside the slot's set": dict(q_point=(1, 0, 1, 2, 0)), "a pair queried twice": dict(q_point=(0, 0, 1, 1, 0)),
    "a pair not queried": dict(q_slot=(0, 1, 1, 1), q_point=(0, 0, 1, 2)), "a query too many": dict(q_slot=(0, 1, 1, 1, 2, 2), q_point=(0, 0, 1, 2, 0, 0)),
}


def test_shplonk_scalars_refusals(lib):
    call = lambda **kw: _shplonk_call(lib, **kw)
    assert call(plan_null=True) == EINVAL and call(omega_null=True) == EINVAL and call(omega=NOT_CANONICAL) == EINVAL
    for name in ARRAYS:
        assert call(null_array=name) == EINVAL, name
    for name, bent in REFUSED_PLANS.items():
        assert call(**bent) == EINVAL, name
        assert b"shplonk_scalars" in lib.zkhip_last_error(), name
    assert call(proofs=(1 << 24) + 1) == EINVAL
    for arg in ("evals", "points", "rows_a", "rows_c", "status"):
        assert call(**{arg: None}) == EINVAL and call(**{arg: FAKE + 8}) == EINVAL, arg
    assert b"shplonk_scalars" in lib.zkhip_last_error()
    # an empty batch names no array, enqueues nothing and never asks the device; a wrong plan is refused all the same
    assert call(proofs=0, evals=None, points=None, rows_a=None, rows_c=None, status=None) == 0 and call(proofs=0, n_sets=65) == EINVAL
    assert call(proofs=0, k=8, rot=tuple(range(64)), starts=(0, 64, 128, 192, 256), set_point=tuple(range(64)) * 4, slot_set=(0, 1, 2, 3), slot_pos=(0, 0, 0, 0),
                q_slot=tuple(s for s in range(4) for _ in range(64)), q_point=tuple(range(64)) * 4) == 0                        # exactly 256 pairs are accepted

"""GPU (-m gpu): SURVEY.md section 8(f) rows 1-3 -- row programs (`zkhip_fr_eval_rows`: the quotient numerator of
[DEP] plonk/evaluation.rs, multiopen linear combinations) and the grand products, bit-exact against the oracle's big-int
restatements (oracle/bn254.py: `row_program_run`, `evaluate_h_direct`, `grand_product`)."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F

pytestmark = pytest.mark.gpu
R = O.R_MOD


def enc(col):
    return F.fr_encode(col)


def run_host(prog, cols, log_rows, prev=None):
    out = None
    if prev is not None:
        out = enc(prev)
    res = prog.run([enc(c) for c in cols], log_rows, out=out, accumulate=prev is not None)
    return F.fr_decode(res)


def oracle_run(prog, cols, log_rows, prev=None, only_rows=None):
    return O.row_program_run(prog.insns, prog.constants, prog.rotations, prog.rot_scale, prog.result_reg, cols, log_rows,
                             omega=prog.omega, prev=prev, only_rows=only_rows)


def random_program(rng, n_cols, n_insns, rot_scale, omega, use_prev, n_regs=_lib.VM_REGS):
    """straight-line program over every opcode / operand kind; registers are read only after they were written"""
    p = E.RowProgram(rot_scale=rot_scale, omega=omega)
    written = []
    edge = [0, 1, R - 1, R - 2, (R - 1) // 2, 2, 1 << 253]

    def operand():
        kinds = ["const", "col"] + (["reg"] if written else []) + (["prev"] if use_prev else []) + (["rowpow"] if omega else [])
        k = rng.choice(kinds)
        if k == "const": return p.constant(rng.choice(edge) if rng.random() < 0.5 else rng.randrange(R))
        if k == "col": return p.column(rng.randrange(n_cols), rng.choice([0, 0, 1, -1, 2, 3, -3, 7]))
        if k == "reg": return E.RowProgram.reg(rng.choice(written))
        if k == "prev": return E.RowProgram.PREV
        return E.RowProgram.ROWPOW

    for _ in range(n_insns):
        op = rng.randrange(8)
        dst = rng.randrange(n_regs)
        p.emit(op, dst, operand(), operand(), operand())
        if dst not in written:
            written.append(dst)
    p.result_reg = written[-1]
    return p


@pytest.mark.parametrize("log_rows,seed", [(0, 1), (1, 2), (5, 3), (8, 4), (8, 5), (9, 6), (13, 7), (7, 8), (6, 9), (10, 10), (9, 11)])
def test_row_program_random_vs_interpreter(lib, log_rows, seed):
    rng = random.Random(seed)
    rows = 1 << log_rows
    n_cols = 5
    cols = [[rng.randrange(R) for _ in range(rows)] for _ in range(n_cols)]
    # edge values: 0 and r-1 runs stress the conditional subtractions
    for i in range(min(rows, 16)):
        cols[0][i] = [0, R - 1, 1, R - 2][i % 4]
        cols[1][i] = [R - 1, R - 1, 0, 1][i % 4]
    omega = O.omega_for(log_rows) if log_rows >= 1 and seed % 2 == 0 else (O.omega_for(max(log_rows, 1)) if seed == 7 else None)
    use_prev = seed % 3 == 0
    prev = [rng.randrange(R) for _ in range(rows)] if use_prev else None
    n_insns = 200 if log_rows < 13 else 60
    # the library runs a kernel variant sized for the highest register named: cover the 6 / 8 / 12 / 16 register variants
    n_regs = [6, 8, 12, 16][seed % 4]
    prog = random_program(rng, n_cols, n_insns, rot_scale=rng.choice([1, 2, 4]), omega=omega, use_prev=use_prev, n_regs=n_regs)
    only = None if log_rows <= 9 else sorted({i for i in rng.sample(range(rows), 200) + [0, 1, rows - 1, 4095, 4096, 4097] if i < rows})
    got = run_host(prog, cols, log_rows, prev)
    exp = oracle_run(prog, cols, log_rows, prev, only)
    if only is None:
        assert got == exp
    else:
        assert [got[i] for i in only] == exp


def test_row_program_long_add_sub_chains_at_the_bounds(lib):
    """chains of add / sub / dbl / neg on 0, 1, r-1: every intermediate must stay a correct residue (values < 2r inside)"""
    p = E.RowProgram()
    a, b = p.column(0), p.column(1)
    p.emit(E.OP_ADD, 0, a, b)
    for i in range(40):
        p.emit(E.OP_DBL, 1, E.RowProgram.reg(0))
        p.emit(E.OP_SUB, 2, E.RowProgram.reg(1), b)
        p.emit(E.OP_NEG, 3, E.RowProgram.reg(2))
        p.emit(E.OP_ADD, 0, E.RowProgram.reg(3), E.RowProgram.reg(1))
        p.emit(E.OP_SUB, 0, E.RowProgram.reg(0), p.constant(R - 1))
        p.emit(E.OP_MAD, 0, E.RowProgram.reg(0), p.constant(R - 1), E.RowProgram.reg(2))
    p.result_reg = 0
    vals = [0, 1, R - 1, R - 2, 2, (R + 1) // 2, (R - 1) // 2, 12345]
    cols = [[vals[i % 8] for i in range(64)], [vals[(i // 8) % 8] for i in range(64)]]
    assert run_host(p, cols, 6) == oracle_run(p, cols, 6)


def halo2_lib_like_cs(n_gate_cols=3):
    """a constraint system of the shape halo2-lib's BaseCircuitBuilder configures (the wrapper / state-transition circuits,
    /root/reference/aggregator/src/wrapper.rs:792-797): per advice column one vertical gate q (a + b c - d) over rotations 0..3,
    a range-check lookup, a two-expression lookup (exercises theta), a permutation over advice + fixed + instance columns."""
    A = n_gate_cols
    gates = [[E.Fixed(i) * (E.Advice(i, 0) + E.Advice(i, 1) * E.Advice(i, 2) - E.Advice(i, 3))] for i in range(A)]
    lookups = [E.Lookup([E.Advice(A)], [E.Fixed(A)]),
               E.Lookup([E.Advice(0) * E.Fixed(A + 1), E.Advice(1, -1) + E.Constant(5)], [E.Fixed(A), E.Fixed(A + 1) * 3])]
    perm = [("advice", i) for i in range(A)] + [("fixed", A + 1), ("instance", 0)]
    return E.ConstraintSystem(num_fixed=A + 2, num_advice=A + 1, num_instance=1, gates=gates, lookups=lookups,
                              permutation_columns=perm, blinding_factors=5, degree=4)


@pytest.mark.parametrize("k,extended_k,gate_cols", [(3, 5, 1), (5, 7, 3), (6, 8, 4)])
def test_evaluate_h_matches_reference_formulas(lib, k, extended_k, gate_cols):
    rng = random.Random(100 + k)
    cs = halo2_lib_like_cs(gate_cols)
    qc = E.quotient_columns(cs)
    rows = 1 << extended_k
    cols = [[rng.randrange(R) for _ in range(rows)] for _ in range(qc.total)]
    beta, gamma, theta, y = (rng.randrange(R) for _ in range(4))
    prog = E.evaluate_h_program(cs, k, extended_k, beta, gamma, theta, y)
    got = run_host(prog, cols, extended_k)
    sets = cs.num_permutation_sets
    exp = O.evaluate_h_direct(
        cs, k, extended_k, cols[qc.fixed:qc.fixed + cs.num_fixed], cols[qc.advice:qc.advice + cs.num_advice],
        cols[qc.instance:qc.instance + cs.num_instance], cols[qc.l0], cols[qc.l_last], cols[qc.l_active_row],
        cols[qc.sigma:qc.sigma + len(cs.permutation_columns)], cols[qc.perm_product:qc.perm_product + sets],
        [tuple(cols[qc.lookup + 3 * i + j] for j in range(3)) for i in range(len(cs.lookups))], beta, gamma, theta, y)
    assert got == exp


def halo2_lib_wide_cs(gate_cols, lookups):
    """the same shape at the width the reference's small circuits really have (`calculate_params(Some(20))`:
    /root/reference/voter/benches/voter_circuit.rs:49-51, /root/reference/aggregator/benches/state_transition_circuit.rs:48-50): `gate_cols`
    vertical gates, `lookups` range lookups on columns of their own, every advice column and a fixed column in the permutation"""
    A, Lk = gate_cols, lookups
    gates = [[E.Fixed(i) * (E.Advice(i, 0) + E.Advice(i, 1) * E.Advice(i, 2) - E.Advice(i, 3))] for i in range(A)]
    lks = [E.Lookup([E.Advice(A + j)], [E.Fixed(A)]) for j in range(Lk)]
    perm = [("advice", i) for i in range(A + Lk)] + [("fixed", A + 1), ("instance", 0)]
    return E.ConstraintSystem(num_fixed=A + 2, num_advice=A + Lk, num_instance=1, gates=gates, lookups=lks,
                              permutation_columns=perm, blinding_factors=5, degree=4)


@pytest.mark.parametrize("k,extended_k,gate_cols,lookups", [(5, 7, 64, 8), (6, 8, 256, 8), (7, 9, 64, 8)])
def test_evaluate_h_wide_matches_reference_formulas(lib, k, extended_k, gate_cols, lookups):
    """`evaluate_h` of a WIDE constraint system (64 / 256 gate columns, 8 lookups: hundreds of columns, thousands of instructions, the
    register allocator and the column-pointer table at their real load) against the oracle's direct restatement of the formulas, row for row"""
    rng = random.Random(200 + k + gate_cols)
    cs = halo2_lib_wide_cs(gate_cols, lookups)
    qc = E.quotient_columns(cs)
    assert qc.total > 4 * gate_cols // 2 + 3 * lookups
    rows = 1 << extended_k
    cols = [[rng.randrange(R) for _ in range(rows)] for _ in range(qc.total)]
    beta, gamma, theta, y = (rng.randrange(R) for _ in range(4))
    prog = E.evaluate_h_program(cs, k, extended_k, beta, gamma, theta, y)
    assert len(prog.insns) > 4 * gate_cols and prog.n_columns == qc.total
    got = run_host(prog, cols, extended_k)
    sets = cs.num_permutation_sets
    exp = O.evaluate_h_direct(
        cs, k, extended_k, cols[qc.fixed:qc.fixed + cs.num_fixed], cols[qc.advice:qc.advice + cs.num_advice],
        cols[qc.instance:qc.instance + cs.num_instance], cols[qc.l0], cols[qc.l_last], cols[qc.l_active_row],
        cols[qc.sigma:qc.sigma + len(cs.permutation_columns)], cols[qc.perm_product:qc.perm_product + sets],
        [tuple(cols[qc.lookup + 3 * i + j] for j in range(3)) for i in range(len(cs.lookups))], beta, gamma, theta, y)
    assert got == exp


def test_evaluate_h_device_resident_large_spot_check(lib):
    """k = 14 / extended 16 on device-resident columns; 150 rows (incl. the wrap-around rows) against the interpreter"""
    import torch

    k, ek = 14, 16
    rows = 1 << ek
    cs = halo2_lib_like_cs(3)
    qc = E.quotient_columns(cs)
    g = np.random.default_rng(5)
    host_cols = []
    for _ in range(qc.total):
        a = g.integers(0, 1 << 64, size=(rows, 4), dtype=np.uint64)
        a[:, 3] = g.integers(0, 0x30644E72E131A029, size=rows, dtype=np.uint64)     # canonical: top limb below the modulus'
        host_cols.append(a)
    d_cols = [torch.from_numpy(a.view(np.int64)).cuda() for a in host_cols]
    d_out = torch.zeros(rows * 4, dtype=torch.int64, device="cuda")
    rng = random.Random(9)
    beta, gamma, theta, y = (rng.randrange(R) for _ in range(4))
    prog = E.evaluate_h_program(cs, k, ek, beta, gamma, theta, y)
    prog.run_device([t.data_ptr() for t in d_cols], ek, d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint64).reshape(rows, 4)
    only = sorted(set(rng.sample(range(rows), 140) + [0, 1, 2, 3, rows - 1, rows - 2, rows - 24, 4095, 4096, 8191]))
    # the interpreter needs column values at rotated rows only: decode the rows it touches
    need = set()
    for r in only:
        for rot in prog.rotations:
            need.add((r + rot * prog.rot_scale) % rows)
    need = sorted(need)
    sparse = [dict(zip(need, F.fr_decode(a[need]))) for a in host_cols]
    exp = O.row_program_run(prog.insns, prog.constants, prog.rotations, prog.rot_scale, prog.result_reg, sparse, ek,
                            omega=prog.omega, only_rows=only)
    assert F.fr_decode(got[only]) == exp


def test_linear_combination_and_accumulate(lib):
    rng = random.Random(31)
    log_rows, n = 10, 7
    rows = 1 << log_rows
    cols = [[rng.randrange(R) for _ in range(rows)] for _ in range(n)]
    coeffs = [rng.randrange(R) for _ in range(n)]
    prog = E.linear_combination_program(coeffs)
    exp = [sum(c * col[i] for c, col in zip(coeffs, cols)) % R for i in range(rows)]
    assert run_host(prog, cols, log_rows) == exp
    # accumulate: out = out * x + column (the multiopen Horner over polynomials)
    x = rng.randrange(R)
    p = E.RowProgram()
    p.emit(E.OP_MAD, 0, E.RowProgram.PREV, p.constant(x), p.column(0))
    prev = [rng.randrange(R) for _ in range(rows)]
    assert run_host(p, cols[:1], log_rows, prev) == [(a * x + b) % R for a, b in zip(prev, cols[0])]


@pytest.mark.parametrize("n", [1, 2, 33, 1000, 4097, 1 << 16, 17, 257, 65537])
def test_grand_product_vs_reference_algorithm(lib, cref, n):
    num = cref.gen_scalars(900 + n, n, 0)
    den = cref.gen_scalars(901 + n, n, 0)
    if n > 40:
        den[17] = 0            # a zero denominator counts as zero (BatchInvert), so every later z is zero
    z = np.zeros_like(num)
    _lib.check(lib.zkhip_fr_grand_product(num.ctypes.data, den.ctypes.data, n, z.ctypes.data))
    inv = den.copy()
    cref.batch_invert(inv)
    ratio = cref.field_op(1, 0, num, inv)
    assert np.array_equal(z, cref.prefix_product(ratio))
    if n <= 1000:
        assert F.fr_decode(z) == O.grand_product(F.fr_decode(num), F.fr_decode(den))


def test_row_program_rejects_malformed_programs(lib):
    col = enc([1, 2, 3, 4])
    out = np.zeros((4, 4), dtype=np.uint64)
    ptrs = (C.c_void_p * 1)(col.ctypes.data)

    def rc_of(p, n_cols=1):
        prog, keep = p._marshal()
        return lib.zkhip_fr_eval_rows(C.byref(prog), ptrs, n_cols, 2, 0, out.ctypes.data)

    good = E.RowProgram()
    good.emit(E.OP_MOV, 0, good.column(0))
    assert rc_of(good) == 0 and F.fr_decode(out) == [1, 2, 3, 4]
    bad = E.RowProgram(); bad.emit(E.OP_MOV, _lib.VM_REGS, bad.column(0))
    assert rc_of(bad) == -1 and b"register" in lib.zkhip_last_error()
    bad = E.RowProgram(); bad.emit(9, 0, bad.column(0))
    assert rc_of(bad) == -1
    bad = E.RowProgram(); bad.emit(E.OP_MOV, 0, bad.column(3))
    assert rc_of(bad) == -1
    bad = E.RowProgram(); bad.emit(E.OP_MOV, 0, E.RowProgram.ROWPOW)          # no omega given
    assert rc_of(bad) == -1
    bad = E.RowProgram(); bad.emit(E.OP_MOV, 0, (E.SRC_CONST, 5, 0))
    assert rc_of(bad) == -1
    bad = E.RowProgram(); bad.constants.append(R); bad.emit(E.OP_MOV, 0, (E.SRC_CONST, 0, 0))
    prog, keep = bad._marshal()
    raw = np.array([O.limbs4(R)], dtype=np.uint64)                              # a non-canonical constant
    prog.constants = raw.ctypes.data
    assert lib.zkhip_fr_eval_rows(C.byref(prog), ptrs, 1, 2, 0, out.ctypes.data) == -1
    empty = E.RowProgram()
    prog, keep = empty._marshal()
    assert lib.zkhip_fr_eval_rows(C.byref(prog), ptrs, 1, 2, 0, out.ctypes.data) == -1


def test_grand_product_inputs_of_permutation_and_lookup_arguments(lib):
    """numerator / denominator programs + zkhip_fr_grand_product == the permutation / lookup product columns written out
    directly ([DEP] plonk/permutation/prover.rs, plonk/lookup/prover.rs)"""
    rng = random.Random(77)
    k = 8
    n = 1 << k
    beta, gamma, theta = (rng.randrange(R) for _ in range(3))
    omega = O.omega_for(k)
    # permutation: a chunk of 2 columns starting at permutation column 3
    vals = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    sig = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    num = run_host(E.permutation_numerator_program(2, 3, beta, gamma, k), vals, k)
    den = run_host(E.permutation_denominator_program(2, beta, gamma), vals + sig, k)
    exp_num, exp_den = [], []
    for i in range(n):
        a = b = 1
        for j in range(2):
            a = a * (vals[j][i] + pow(O.FR_DELTA, 3 + j, R) * beta % R * pow(omega, i, R) + gamma) % R
            b = b * (vals[j][i] + beta * sig[j][i] + gamma) % R
        exp_num.append(a); exp_den.append(b)
    assert num == exp_num and den == exp_den
    z = np.zeros((n, 4), dtype=np.uint64)
    N, D = enc(num), enc(den)
    _lib.check(lib.zkhip_fr_grand_product(N.ctypes.data, D.ctypes.data, n, z.ctypes.data))
    assert F.fr_decode(z) == O.grand_product(exp_num, exp_den)
    # lookup: two input / table expressions compressed with theta
    ins = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    tabs = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    perm = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    pn, pd = E.lookup_product_programs(2, 2, beta, gamma, theta)
    assert run_host(pn, ins + tabs, k) == [((ins[0][i] * theta + ins[1][i] + beta) * (tabs[0][i] * theta + tabs[1][i] + gamma)) % R for i in range(n)]
    assert run_host(pd, perm, k) == [(perm[0][i] + beta) * (perm[1][i] + gamma) % R for i in range(n)]


@pytest.mark.parametrize("n,bits,seed", [(1, 3, 1), (2, 1, 2), (64, 3, 3), (1000, 6, 4), (5000, 10, 5), (1 << 14, 12, 6), (3000, 250, 7)])
def test_lookup_permute_expression_pair_vs_reference_algorithm(lib, n, bits, seed):
    """range-check shaped lookups (inputs below 2^bits, table = the range, padded) and full-width values; the usable rows exclude
    the blinding rows as in the reference"""
    rng = random.Random(seed)
    usable = max(1, n - 6) if n > 8 else n
    if bits < 200:
        table = [i % (1 << bits) for i in range(n)]
        if n < (1 << bits):                                         # small table: inputs must come from what the table holds
            inputs = [rng.choice(table[:usable]) for _ in range(n)]
        else:
            inputs = [rng.randrange(1 << bits) for _ in range(n)]
    else:
        table = [rng.randrange(R) for _ in range(n)]
        inputs = [rng.choice(table[:usable]) for _ in range(n)]
    head = table[:usable]
    rng.shuffle(head)
    table[:usable] = head
    exp_in, exp_tab = O.permute_expression_pair(inputs, table, usable)
    got_in, got_tab = E.permute_expression_pair(enc(inputs), enc(table), usable)
    assert F.fr_decode(got_in) == exp_in
    assert F.fr_decode(got_tab) == exp_tab
    # the defining property of the permuted pair
    for i in range(usable):
        assert exp_tab[i] == exp_in[i] or (i > 0 and exp_in[i] == exp_in[i - 1])


def test_lookup_permute_reports_missing_table_value(lib):
    inputs, table = [1, 2, 3, 9], [1, 2, 3, 4]
    with pytest.raises(_lib.ZkhipError, match="missing from the table"):
        E.permute_expression_pair(enc(inputs), enc(table), 4)
    with pytest.raises(ValueError):
        O.permute_expression_pair(inputs, table, 4)
    # all inputs equal: one first row, the rest take the leftovers in descending row order
    got_in, got_tab = E.permute_expression_pair(enc([5] * 6), enc([5, 1, 2, 3, 4, 0]), 6)
    assert F.fr_decode(got_in) == [5] * 6 and F.fr_decode(got_tab) == [5, 4, 3, 2, 1, 0]


@pytest.mark.parametrize("n,count", [(1, 3), (31, 2), (32, 1), (33, 5), (1025, 7), (70001, 3), (1 << 16, 40)])
def test_eval_polynomial_batch_vs_single(lib, cref, n, count):
    """multiopen: many polynomials at one point, one launch per recursion level; each result equals the single-polynomial path
    and (small cases) the oracle"""
    import torch

    polys = [cref.gen_scalars(5000 + n + i, n, i % 2) for i in range(count)]
    x = cref.gen_scalars(77 + n, 1, 0)[0]
    d = [torch.from_numpy(p.view(np.int64)).cuda() for p in polys]
    out = torch.zeros(count * 4, dtype=torch.int64, device="cuda")
    ptrs = (C.c_void_p * count)(*[t.data_ptr() for t in d])
    _lib.check(lib.zkhip_fr_eval_polynomial_batch_device(ptrs, count, n, x.ctypes.data, out.data_ptr(), None))
    _lib.check(lib.zkhip_sync())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64).reshape(count, 4)
    for i in range(count):
        assert np.array_equal(got[i], cref.eval_polynomial(polys[i], x)), i
    if n <= 1025:
        xv = F.fr_decode(x)[0]
        assert F.fr_decode(got[0]) == [O.eval_polynomial(F.fr_decode(polys[0]), xv)]


def test_golden_prover_steps(lib):
    """the committed fixtures of the 8(f) steps (tests/golden/prover_steps.json, generated from the oracle) through the C ABI"""
    import json
    import os

    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "prover_steps.json")))
    words = lambda hs: np.array([[int(h[16 * i:16 * i + 16], 16) for i in range(4)] for h in hs], dtype=np.uint64)
    val = lambda h: F.fr_decode(words([h]))[0]
    rp = gold["row_program"]
    p = E.RowProgram(rot_scale=rp["rot_scale"], omega=val(rp["omega"]))
    p.constants = [val(h) for h in rp["constants"]]
    p.rotations = list(rp["rotations"])
    p.insns = [(r[0], r[1], tuple(r[2:5]), tuple(r[5:8]), tuple(r[8:11])) for r in rp["insns"]]
    p.result_reg, p.n_columns = rp["result_reg"], len(rp["columns"])
    out = words(rp["prev"]).copy()
    p.run([words(c) for c in rp["columns"]], rp["log_rows"], out=out, accumulate=True)
    assert np.array_equal(out, words(rp["expected"]))
    eh = gold["evaluate_h"]
    cs = halo2_lib_like_cs(eh["gate_cols"])
    cs.blinding_factors = eh["blinding_factors"]
    prog = E.evaluate_h_program(cs, eh["k"], eh["extended_k"], *(val(eh[c]) for c in ("beta", "gamma", "theta", "y")))
    assert np.array_equal(prog.run([words(c) for c in eh["columns"]], eh["extended_k"]), words(eh["expected"]))
    lp = gold["lookup_permute"]
    pi, pt = E.permute_expression_pair(words(lp["input"]), words(lp["table"]), lp["usable_rows"])
    assert np.array_equal(pi, words(lp["permuted_input"])) and np.array_equal(pt, words(lp["permuted_table"]))
    gp = gold["grand_product"]
    num, den = words(gp["num"]), words(gp["den"])
    z = np.zeros_like(num)
    _lib.check(lib.zkhip_fr_grand_product(num.ctypes.data, den.ctypes.data, num.shape[0], z.ctypes.data))
    assert np.array_equal(z, words(gp["z"]))


def _permutation_products_expected(vals, sig, chunk, k, usable, beta, gamma):
    """[DEP] plonk/permutation/prover.rs written out with big integers: per set the running product of num / den over the rows below
    `usable`, the sets chained through z[usable]; rows after `usable` repeat z[usable] (the caller's blinding rows)"""
    n, omega = 1 << k, O.omega_for(k)
    out, last = [], 1
    for lo in range(0, len(vals), chunk):
        z = [last]
        for i in range(n - 1):
            if i < usable:
                a = b = 1
                for c in range(lo, min(lo + chunk, len(vals))):
                    a = a * (vals[c][i] + pow(O.FR_DELTA, c, R) * beta % R * pow(omega, i, R) + gamma) % R
                    b = b * (vals[c][i] + beta * sig[c][i] + gamma) % R
                z.append(z[-1] * a % R * pow(b, -1, R) % R if b else 0)
            else:
                z.append(z[-1])
        last = z[usable]
        out.append(z)
    return out


@pytest.mark.parametrize("k,nperm,chunk", [(6, 5, 2), (5, 1, 2), (7, 6, 3), (4, 9, 1), (9, 4, 4)])
def test_permutation_products_every_set_in_one_call(lib, k, nperm, chunk):
    """zkhip_permutation_products (host buffers) == the permutation argument's products written out; the device form on the same columns ==
    the host form"""
    import torch

    rng = random.Random(1000 * k + nperm)
    n, usable = 1 << k, (1 << k) - 6
    beta, gamma = rng.randrange(R), rng.randrange(R)
    vals = [[rng.randrange(R) for _ in range(n)] for _ in range(nperm)]
    sig = [[rng.randrange(R) for _ in range(n)] for _ in range(nperm)]
    nsets = -(-nperm // chunk)
    V, S = [enc(c) for c in vals], [enc(c) for c in sig]
    consts = [F.fr_encode([x])[0] for x in (beta, gamma, O.FR_DELTA, O.omega_for(k))]
    z = np.zeros((nsets * n, 4), dtype=np.uint64)
    vp, sp = (C.c_void_p * nperm)(*[a.ctypes.data for a in V]), (C.c_void_p * nperm)(*[a.ctypes.data for a in S])
    _lib.check(lib.zkhip_permutation_products(vp, sp, nperm, chunk, k, usable, *[c.ctypes.data for c in consts], z.ctypes.data))
    exp = _permutation_products_expected(vals, sig, chunk, k, usable, beta, gamma)
    got = F.fr_decode(z)
    for s in range(nsets):
        assert got[s * n:(s + 1) * n] == exp[s], f"set {s}"
    dev = torch.device("cuda", 0)
    dV = [torch.from_numpy(a.view(np.int64)).to(dev) for a in V]
    dS = [torch.from_numpy(a.view(np.int64)).to(dev) for a in S]
    dz = torch.zeros((nsets * n, 4), dtype=torch.int64, device=dev)
    vp, sp = (C.c_void_p * nperm)(*[t.data_ptr() for t in dV]), (C.c_void_p * nperm)(*[t.data_ptr() for t in dS])
    _lib.check(lib.zkhip_permutation_products_device(vp, sp, nperm, chunk, k, usable, *[c.ctypes.data for c in consts], dz.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(dz.cpu().numpy().view(np.uint64), z)


def test_permutation_products_equal_the_row_program_path_at_2p14(lib):
    """the one-call form against the composition it replaces (numerator / denominator row programs, zkhip_fr_grand_product, chaining by a
    scaling program) on 7 columns in sets of 2 at k = 14, with a zero denominator in the second set (every later value is zero, like BatchInvert)"""
    import torch

    k, nperm, chunk = 14, 7, 2
    n, usable = 1 << k, (1 << k) - 6
    dev = torch.device("cuda", 0)
    rng = random.Random(5)
    beta, gamma = rng.randrange(R), rng.randrange(R)
    g = torch.Generator(device="cpu"); g.manual_seed(11)

    def rand_cols(m):
        a = torch.randint(-(1 << 63), (1 << 63) - 1, (m, n, 4), dtype=torch.int64, generator=g)
        a[:, :, 3] = torch.randint(0, 1 << 61, (m, n), dtype=torch.int64, generator=g)
        return a

    V, S = rand_cols(nperm), rand_cols(nperm)
    # a zero denominator: v + beta sigma + gamma = 0 at row 100 of column 2 (set 1)
    v100 = F.fr_decode(V[2, 100:101].numpy().view(np.uint64))[0]
    sig100 = (-(v100 + gamma)) * pow(beta, -1, R) % R
    S[2, 100] = torch.from_numpy(F.fr_encode([sig100]).view(np.int64))[0]
    dV, dS = V.to(dev), S.to(dev)
    nsets = -(-nperm // chunk)
    consts = [F.fr_encode([x])[0] for x in (beta, gamma, O.FR_DELTA, O.omega_for(k))]
    dz = torch.zeros((nsets, n, 4), dtype=torch.int64, device=dev)
    vp, sp = (C.c_void_p * nperm)(*[dV[i].data_ptr() for i in range(nperm)]), (C.c_void_p * nperm)(*[dS[i].data_ptr() for i in range(nperm)])
    _lib.check(lib.zkhip_permutation_products_device(vp, sp, nperm, chunk, k, usable, *[c.ctypes.data for c in consts], dz.data_ptr(), None))
    torch.cuda.synchronize()
    last = 1
    for s in range(nsets):
        lo, hi = s * chunk, min((s + 1) * chunk, nperm)
        num = torch.empty((n, 4), dtype=torch.int64, device=dev)
        den = torch.empty((n, 4), dtype=torch.int64, device=dev)
        E.permutation_numerator_program(hi - lo, lo, beta, gamma, k).run_device([dV[c].data_ptr() for c in range(lo, hi)], k, num.data_ptr())
        E.permutation_denominator_program(hi - lo, beta, gamma).run_device([dV[c].data_ptr() for c in range(lo, hi)] + [dS[c].data_ptr() for c in range(lo, hi)], k, den.data_ptr())
        _lib.check(lib.zkhip_fr_grand_product_device(num.data_ptr(), den.data_ptr(), n, num.data_ptr(), None))
        torch.cuda.synchronize()
        zs = F.fr_decode(num[:usable + 1].cpu().numpy().view(np.uint64))
        got = F.fr_decode(dz[s, :usable + 1].cpu().numpy().view(np.uint64))
        assert got == [last * x % R for x in zs], f"set {s}"
        tail = F.fr_decode(dz[s, usable:].cpu().numpy().view(np.uint64))
        assert tail == [tail[0]] * len(tail)
        last = got[usable]
    assert last == 0


def test_permutation_products_reject_bad_arguments(lib):
    col = enc([1, 2, 3, 4])
    z = np.zeros((4, 4), dtype=np.uint64)
    one = F.fr_encode([1])[0]
    ptrs = (C.c_void_p * 1)(col.ctypes.data)
    null = (C.c_void_p * 1)(None)
    args = (one.ctypes.data,) * 4
    assert lib.zkhip_permutation_products(ptrs, ptrs, 1, 0, 2, 3, *args, z.ctypes.data) == -1          # chunk_len 0
    assert lib.zkhip_permutation_products(ptrs, ptrs, 1, 2, 2, 5, *args, z.ctypes.data) == -1          # usable_rows > n
    assert lib.zkhip_permutation_products(ptrs, null, 1, 2, 2, 3, *args, z.ctypes.data) == -1          # a null column
    assert lib.zkhip_permutation_products(ptrs, ptrs, 1, 2, 2, 3, *args, None) == -1
    assert lib.zkhip_permutation_products(ptrs, ptrs, 0, 2, 2, 3, *args, None) == 0                    # no columns: nothing to do


def _pinned_fr(values):
    """(len(values), 4) uint64 view of page-locked host memory holding the encoded values (and the tensor that owns it)"""
    import torch

    t = torch.empty((len(values), 4), dtype=torch.int64, pin_memory=True)
    a = t.numpy().view(np.uint64)
    a[:] = enc(values)
    return a, t


def test_permutation_products_null_last_column_then_a_correct_call(lib):
    """a null column -- the last one, behind columns an upload could already have started on -- is refused with nothing enqueued, and a correct
    call from the same thread right after it (same lane, pinned inputs) is bit-exact"""
    k, nperm, chunk = 6, 3, 2
    rng = random.Random(77)
    n, usable = 1 << k, (1 << k) - 6
    beta, gamma = rng.randrange(R), rng.randrange(R)
    vals = [[rng.randrange(R) for _ in range(n)] for _ in range(nperm)]
    sig = [[rng.randrange(R) for _ in range(n)] for _ in range(nperm)]
    V, S = [_pinned_fr(c) for c in vals], [_pinned_fr(c) for c in sig]
    consts = [F.fr_encode([x])[0] for x in (beta, gamma, O.FR_DELTA, O.omega_for(k))]
    args = [c.ctypes.data for c in consts]
    nsets = -(-nperm // chunk)
    z = np.zeros((nsets * n, 4), dtype=np.uint64)
    vp = (C.c_void_p * nperm)(*[a.ctypes.data for a, _ in V])
    sp = (C.c_void_p * nperm)(*[a.ctypes.data for a, _ in S])
    sp_null = (C.c_void_p * nperm)(*([a.ctypes.data for a, _ in S[:-1]] + [None]))
    assert lib.zkhip_permutation_products(vp, sp_null, nperm, chunk, k, usable, *args, z.ctypes.data) == -1
    assert lib.zkhip_last_error().decode() == f"permutation_products: column {nperm - 1} is null"
    assert not z.any()
    _lib.check(lib.zkhip_permutation_products(vp, sp, nperm, chunk, k, usable, *args, z.ctypes.data))
    exp = _permutation_products_expected(vals, sig, chunk, k, usable, beta, gamma)
    got = F.fr_decode(z)
    for s in range(nsets):
        assert got[s * n:(s + 1) * n] == exp[s], f"set {s}"


def test_eval_rows_null_last_column_then_a_correct_call(lib):
    """zkhip_fr_eval_rows checks every column before its first copy: a null LAST column is ZKHIP_EINVAL with the message it always had and nothing
    enqueued (the output is untouched), and a correct call from the same thread right after it (pinned inputs) equals the oracle"""
    log_rows, n_cols = 10, 3
    rows = 1 << log_rows
    rng = random.Random(78)
    cols = [[rng.randrange(R) for _ in range(rows)] for _ in range(n_cols)]
    p = E.RowProgram()
    p.emit(E.OP_MAD, 0, p.column(0, 1), p.column(1, -1), p.column(2, 0))
    p.emit(E.OP_ADD, 1, E.RowProgram.reg(0), p.constant(R - 1))
    p.result_reg = 1
    P = [_pinned_fr(c) for c in cols]
    out, _keep = _pinned_fr([0] * rows)
    prog, keep = p._marshal()
    ptrs = (C.c_void_p * n_cols)(*[a.ctypes.data for a, _ in P])
    ptrs_null = (C.c_void_p * n_cols)(*([a.ctypes.data for a, _ in P[:-1]] + [None]))
    assert lib.zkhip_fr_eval_rows(C.byref(prog), ptrs_null, n_cols, log_rows, 0, out.ctypes.data) == -1
    assert lib.zkhip_last_error().decode() == f"eval_rows: column {n_cols - 1} is null"
    assert not out.any()
    _lib.check(lib.zkhip_fr_eval_rows(C.byref(prog), ptrs, n_cols, log_rows, 0, out.ctypes.data))
    del keep
    assert F.fr_decode(out) == oracle_run(p, cols, log_rows)


@pytest.mark.parametrize("log_n,count", [(0, 1), (3, 2), (7, 33), (9, 70), (10, 1), (6, 0), (5, 2100)])
def test_linear_combination_of_many_columns(lib, log_n, count):
    """zkhip_fr_linear_combination_device == sum_j c_j col_j with big integers (one group, several groups, an odd column left over, more than
    64 groups, no column at all), also with the output aliasing a column"""
    import torch

    rng = random.Random(100 * log_n + count)
    n = 1 << log_n
    dev = torch.device("cuda", 0)
    base = [[rng.randrange(R) if rng.random() < 0.9 else rng.choice([0, 1, R - 1]) for _ in range(n)] for _ in range(min(count, 40))]
    cols = [base[j % len(base)] for j in range(count)] if count else []
    coeffs = [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(count)]
    d_base = [torch.from_numpy(enc(c).view(np.int64)).to(dev) for c in base]
    d_cols = [d_base[j % len(d_base)] for j in range(count)]
    cw = F.fr_encode(coeffs) if count else np.zeros((1, 4), dtype=np.uint64)
    out = torch.full((n, 4), -1, dtype=torch.int64, device=dev)
    ptrs = (C.c_void_p * max(count, 1))(*[t.data_ptr() for t in d_cols])
    _lib.check(lib.zkhip_fr_linear_combination_device(ptrs, cw.ctypes.data, count, n, out.data_ptr(), None))
    torch.cuda.synchronize()
    exp = [sum(c * col[i] for c, col in zip(coeffs, cols)) % R for i in range(n)]
    assert F.fr_decode(out.cpu().numpy().view(np.uint64)) == exp
    if count:                                  # in place: the output is the first column
        first = d_cols[0].clone()
        ptrs = (C.c_void_p * count)(*([first.data_ptr()] + [t.data_ptr() if t is not d_cols[0] else first.data_ptr() for t in d_cols[1:]]))
        _lib.check(lib.zkhip_fr_linear_combination_device(ptrs, cw.ctypes.data, count, n, first.data_ptr(), None))
        torch.cuda.synchronize()
        assert F.fr_decode(first.cpu().numpy().view(np.uint64)) == exp


@pytest.mark.parametrize("parts", [1, 2, 7, 64])
def test_quotient_numerator_as_a_sum_of_programs(lib, parts):
    """evaluate_h_parts + zkhip_fr_eval_rows_sum_device == evaluate_h_program (one fold over all terms) on random columns of a halo2-lib
    shaped constraint system (6 gate columns, 2 lookups: 25 terms); `parts` beyond the number of terms is clamped"""
    import torch

    k, ek = 6, 8
    rows = 1 << ek
    cs = E.halo2_lib_shape(6, 2)
    qc = E.quotient_columns(cs)
    rng = random.Random(parts)
    beta, gamma, theta, y = (rng.randrange(1, R) for _ in range(4))
    dev = torch.device("cuda", 0)
    cols = torch.randint(-(1 << 63), (1 << 63) - 1, (qc.total, rows, 4), dtype=torch.int64, device=dev)
    cols[:, :, 3] = torch.randint(0, 1 << 61, (qc.total, rows), dtype=torch.int64, device=dev)
    ptrs = [cols[i].data_ptr() for i in range(qc.total)]
    whole = torch.empty((rows, 4), dtype=torch.int64, device=dev)
    E.evaluate_h_program(cs, k, ek, beta, gamma, theta, y).run_device(ptrs, ek, whole.data_ptr())
    progs, weights = E.evaluate_h_parts(cs, k, ek, beta, gamma, theta, y, parts)
    assert 1 <= len(progs) <= parts and weights[-1] == 1
    summed = torch.full((rows, 4), -1, dtype=torch.int64, device=dev)
    E.run_programs_sum_device(progs, weights, ptrs, ek, summed.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(summed, whole)


def test_eval_rows_sum_rejects_bad_arguments(lib):
    import torch

    p = E.RowProgram(); p.emit(E.OP_MOV, 0, p.column(0))
    prog, keep = p._marshal()
    arr = (_lib.VmProgram * 1)(prog)
    col = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    out = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    w = F.fr_encode([1])
    ptrs = (C.c_void_p * 1)(col.data_ptr())
    assert lib.zkhip_fr_eval_rows_sum_device(arr, w.ctypes.data, 1, ptrs, 1, 2, out.data_ptr(), None) == 0
    assert lib.zkhip_fr_eval_rows_sum_device(arr, w.ctypes.data, 0, ptrs, 1, 2, out.data_ptr(), None) == -1
    assert lib.zkhip_fr_eval_rows_sum_device(arr, None, 1, ptrs, 1, 2, out.data_ptr(), None) == -1
    assert lib.zkhip_fr_eval_rows_sum_device(arr, w.ctypes.data, 1, ptrs, 0, 2, out.data_ptr(), None) == -1        # the program names column 0
    torch.cuda.synchronize()

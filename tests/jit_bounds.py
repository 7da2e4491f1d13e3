"""Shared by tests/test_vm_jit_bounds_host.py (CPU) and tests/test_gpu_vm_jit_bounds.py (-m gpu): row programs that put a register AT the
magnitude thresholds of the run-time compiler (csrc/rowvm_jit.hip), a worst-case replay of the text it generates, and the jobs a child
process runs through the compiled executor.

The generator keeps additions lazy and tracks, per register, an upper bound in units of r; it emits a reduction only where a threshold is
crossed (2 / 4: condsub2 against fe_reduce_soft; 2.3: SQR; 5.29: a product's operands and the times32 repack; 15: the subtrahend of SUB / NEG,
which picks one of P2_S1 .. P16_S1; 30: DBL; 40: the minuend of SUB; 60: ADD and the addend of MAD; 3: the final fe_canon_lt3p).  `DIRECTED`
has one program just under and one just over each of them, each with the reductions and `Fr::PK_S1` constants the generator must emit.

`check_magnitudes` does not trust those bounds: it walks the generated text with exact integers -- for every name the largest value that can
occur -- and raises where the precondition of an operation (csrc/fp29.hpp, the prelude of rowvm_jit.hip) can fail."""
import json
import random
import re
import sys
from collections import namedtuple

from zksnap_circuits_halo2_amd import evaluation as E, fields as F

R = F.R_MOD
REG = E.RowProgram.reg
GRID = [0, 1, R - 1, R - 2, 2, (R + 1) // 2, (R - 1) // 2, random.Random(20).randrange(R)]


def grid_columns(log_rows=6):
    """two columns on the 8 x 8 grid of GRID (repeating past 64 rows): some rows have both columns 0, some both r-1, so a register that grows
    by additions sits at m (r-1) on some rows and at an exact multiple of r on others"""
    n = 1 << log_rows
    return [[GRID[i % 8] for i in range(n)], [GRID[(i // 8) % 8] for i in range(n)]]


def prev_column(log_rows=6):
    rng = random.Random(21)
    edge = [0, R - 1, 1, R - 2]
    return [edge[i % 4] if i < 16 else rng.randrange(R) for i in range(1 << log_rows)]


def grow(p, reg, m, col=0):
    """MOV reg, col then m-1 x ADD reg, reg, col: generator bound m, value m * col"""
    p.emit(E.OP_MOV, reg, p.column(col))
    for _ in range(m - 1):
        p.emit(E.OP_ADD, reg, REG(reg), p.column(col))


# ---- the directed programs ------------------------------------------------------------------------------------------------------------------
# condsub2 / soft: the names reduced, in the order of the text; pk: the K of every Fr::PK_S1, in order; contains: text that must appear
Directed = namedtuple("Directed", "name prog condsub2 soft pk contains")
DIRECTED = []


def _final(bound, reg):
    """the reduction of the result register: none strictly below 3 (fe_canon_lt3p needs a value < 3r), condsub2 up to 4, soft above"""
    return ([], []) if bound < 3 else ([reg], []) if bound <= 4 else ([], [reg])


def _add(name, build, condsub2=(), soft=(), pk=(), contains=(), result_bound=None, omega=None):
    p = E.RowProgram(omega=omega)
    p.result_reg = build(p)
    c, s = list(condsub2), list(soft)
    if result_bound is not None:
        fc, fs = _final(result_bound, "r%d" % p.result_reg)
        c, s = c + fc, s + fs
    DIRECTED.append(Directed(name, p, c, s, list(pk), tuple(contains)))


def _build_directed():
    a, b = (lambda p: p.column(0)), (lambda p: p.column(1))
    OMEGA = F.omega_for(6)

    # a product's first factor: a register of bound m times a memory operand (which takes the free scaling): 5 <= 5.29 < 6
    def first_factor(m):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_MUL, 1, REG(0), b(p))
            return 1
        return build
    _add("mul_first_factor_5", first_factor(5), contains=["fe_mul<Fr, false>(r0, t"])
    _add("mul_first_factor_6", first_factor(6), soft=["r0"])

    # its second factor: register x register, the other one a MOV of a column: times32 repacks 5 (r-1) < 2^256 = 5.29 r
    def second_factor(m):
        def build(p):
            p.emit(E.OP_MOV, 1, b(p))
            grow(p, 0, m)
            p.emit(E.OP_MUL, 2, REG(1), REG(0))
            return 2
        return build
    _add("mul_second_factor_5", second_factor(5), contains=["fe_mul<Fr, false>(r1, times32(r0))"])
    _add("mul_second_factor_6", second_factor(6), soft=["r0"], contains=["fe_mul<Fr, false>(r1, times32(r0))"])

    # bounds 3 x 2 = 6 > 5.29: the larger one takes a conditional subtraction, whichever side it is on
    def three_by_two(swap):
        def build(p):
            grow(p, 0, 3)
            grow(p, 1, 2, col=1)
            p.emit(E.OP_MUL, 2, *((REG(1), REG(0)) if swap else (REG(0), REG(1))))
            return 2
        return build
    _add("mul_3_by_2", three_by_two(False), condsub2=["r0"])
    _add("mul_2_by_3", three_by_two(True), condsub2=["r0"])

    def sqr(m):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_SQR, 1, REG(0))
            return 1
        return build
    _add("sqr_2", sqr(2))
    _add("sqr_3", sqr(3), condsub2=["r0"])
    _add("sqr_5", sqr(5), soft=["r0"])

    # the subtrahend of SUB and the operand of NEG: K r with K - 1 the first of 1, 2, 3, 5, 7, 9, 11, 15 at or above the bound
    ladder = [(1, 2), (2, 3), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (15, 16)]

    def sub(m):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_SUB, 1, b(p), REG(0))
            return 1
        return build

    def neg(m):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_NEG, 1, REG(0))
            return 1
        return build
    for m, k in ladder:
        _add("sub_subtrahend_%d" % m, sub(m), pk=[k], result_bound=1 + k)
        _add("neg_%d" % m, neg(m), pk=[k], result_bound=k)
    _add("sub_subtrahend_16", sub(16), soft=["r0"], pk=[4], result_bound=5)          # reduced (< 2r + 2^233), then 4r - b
    _add("neg_16", neg(16), soft=["r0"], pk=[4], result_bound=4)

    def minuend(m):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_SUB, 1, REG(0), b(p))
            return 1
        return build
    _add("sub_minuend_40", minuend(40), pk=[2], result_bound=42)
    _add("sub_minuend_41", minuend(41), soft=["r0"], pk=[2], result_bound=4.5)

    def dbl(m):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_DBL, 1, REG(0))
            return 1
        return build
    _add("dbl_30", dbl(30), result_bound=60)
    _add("dbl_31", dbl(31), soft=["r0"], result_bound=4.5)

    def add(m):
        def build(p):
            grow(p, 0, m)
            grow(p, 1, 30, col=1)
            p.emit(E.OP_ADD, 2, REG(0), REG(1))
            return 2
        return build
    _add("add_30_30", add(30), result_bound=60)
    _add("add_31_30", add(31), soft=["r0", "r1"], result_bound=4.5)

    # the addend of MAD at 60: the sum (bound about 61.2) then becomes a product's factor, the largest input fe_reduce_soft can see;
    # one more MAD on top finds its addend above 60
    def mad(over):
        def build(p):
            grow(p, 0, 30)
            grow(p, 1, 30, col=1)
            p.emit(E.OP_ADD, 2, REG(0), REG(1))
            p.emit(E.OP_MAD, 3, a(p), b(p), REG(2))
            if over:
                p.emit(E.OP_MAD, 4, a(p), b(p), REG(3))
            else:
                p.emit(E.OP_MUL, 4, REG(3), b(p))
            return 4
        return build
    _add("mad_addend_60", mad(False), soft=["r3"])
    _add("mad_addend_61", mad(True), soft=["r3"], result_bound=3.2)

    # the result register
    def result_sum(m):
        def build(p):
            grow(p, 0, m)
            return 0
        return build
    for m in (1, 2, 3, 4):
        _add("result_bound_%d" % m, result_sum(m), result_bound=m)

    def result_62(p):
        grow(p, 0, 30)
        grow(p, 1, 30, col=1)
        p.emit(E.OP_ADD, 2, REG(0), REG(1))
        p.emit(E.OP_MAD, 3, a(p), b(p), REG(2))
        return 3
    _add("result_bound_62", result_62, result_bound=61.2)

    # omega^row (generator bound 1.76) and the previous value (bound 1) as a product's factor against a register of bound 3 and 4
    def special(operand, m, first):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_MUL, 1, *((operand, REG(0)) if first else (REG(0), operand)))
            return 1
        return build
    _add("rowpow_by_3", special(E.RowProgram.ROWPOW, 3, True), omega=OMEGA, contains=["fe_mul<Fr, false>(vpow, times32(r0))"])
    _add("rowpow_by_4", special(E.RowProgram.ROWPOW, 4, True), omega=OMEGA, condsub2=["r0"])
    _add("3_by_rowpow", special(E.RowProgram.ROWPOW, 3, False), omega=OMEGA, contains=["fe_mul<Fr, false>(r0, times32(vpow))"])
    _add("4_by_rowpow", special(E.RowProgram.ROWPOW, 4, False), omega=OMEGA, condsub2=["r0"])
    _add("prev_by_3", special(E.RowProgram.PREV, 3, True), contains=["fe_mul<Fr, false>(vprev, times32(r0))"])
    _add("prev_by_4", special(E.RowProgram.PREV, 4, True), contains=["fe_mul<Fr, false>(vprev, times32(r0))"])
    _add("4_by_prev", special(E.RowProgram.PREV, 4, False), contains=["fe_mul<Fr, false>(r0, times32(vprev))"])

    # a register read before it is written: include/zkhip.h, "registers start at 0 for every row"
    def unwritten(p):
        p.emit(E.OP_ADD, 0, REG(5), a(p))
        p.emit(E.OP_MUL, 1, REG(0), REG(6))
        p.emit(E.OP_SUB, 2, REG(1), REG(7))
        p.emit(E.OP_MAD, 3, REG(2), b(p), REG(0))
        return 3
    _add("register_read_before_written", unwritten, pk=[2], contains=["r5 = fe_zero()", "r6 = fe_zero()", "r7 = fe_zero()"])

    def unwritten_result(p):
        p.emit(E.OP_MOV, 0, a(p))
        return 9
    _add("unwritten_result_register", unwritten_result, contains=["r9 = fe_zero()"])

    # results that are an exact multiple of r on some rows: K r - 0
    def neg_product(mov):
        def build(p):
            p.emit(E.OP_MUL, 0, a(p), b(p))
            p.emit(E.OP_NEG, 1, REG(0))
            if mov:
                p.emit(E.OP_MOV, 2, REG(1))
            return 2 if mov else 1
        return build

    def neg_sum(mov):
        def build(p):
            p.emit(E.OP_ADD, 0, a(p), b(p))
            p.emit(E.OP_NEG, 1, REG(0))
            if mov:
                p.emit(E.OP_MOV, 2, REG(1))
            return 2 if mov else 1
        return build
    _add("neg_of_product", neg_product(False), pk=[3], result_bound=3)
    _add("neg_of_sum", neg_sum(False), pk=[3], result_bound=3)
    _add("mov_of_neg_of_product", neg_product(True), pk=[3], result_bound=3)
    _add("mov_of_neg_of_sum", neg_sum(True), pk=[3], result_bound=3)

    def x_minus_x(m):
        def build(p):
            grow(p, 0, m)
            p.emit(E.OP_SUB, 1, REG(0), REG(0))
            return 1
        return build
    for m, k in ((1, 2), (2, 3), (5, 6)):
        _add("x_minus_x_%d" % m, x_minus_x(m), pk=[k], result_bound=m + k)


_build_directed()
DIRECTED_BY_NAME = {d.name: d for d in DIRECTED}
assert len(DIRECTED_BY_NAME) == len(DIRECTED)


# ---- the generated text ---------------------------------------------------------------------------------------------------------------------
def source_of(lib, prog, n_columns, log_rows):
    """zkhip_vm_jit_source: the whole translation unit the generator writes for `prog`"""
    import ctypes as C

    from zksnap_circuits_halo2_amd import _lib

    P, keep = prog._marshal()
    n = C.c_size_t(0)
    buf = C.create_string_buffer(1 << 18)
    _lib.check(lib.zkhip_vm_jit_source(C.byref(P), n_columns, log_rows, buf, len(buf), C.byref(n)))
    if n.value > len(buf):                              # *len: the bytes needed, NUL included
        buf = C.create_string_buffer(n.value)
        _lib.check(lib.zkhip_vm_jit_source(C.byref(P), n_columns, log_rows, buf, n.value, None))
    del keep
    return buf.value.decode()


def kernel_body(source):
    return source[source.index('extern "C" __global__'):]


def reductions_of(source):
    """(names given to condsub2, names given to fe_reduce_soft, the K of every Fr::PK_S1), each in the order of the text"""
    body = kernel_body(source)
    return (re.findall(r"= condsub2\((\w+)\);", body), re.findall(r"= fe_reduce_soft<Fr>\((\w+)\);", body),
            [int(k) for k in re.findall(r"Fr::P(\d+)_S1", body)])


class MagnitudeError(AssertionError):
    pass


def _split_args(s):
    args, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    args.append(cur.strip())
    return args


_NAME = re.compile(r"^(r\d+|t\d+|vprev|vpow)$")
_CALL = re.compile(r"^(\w+)(<[^()]*>)?\((.*)\)$", re.S)


def check_magnitudes(source):
    """Replays the kernel of `source` on worst-case magnitudes.  A value is (largest integer it can be, scale): scale 5 marks x 2^5, the form
    fe_mul takes as its second factor.  The rules are those of csrc/fp29.hpp and of the prelude of csrc/rowvm_jit.hip:
      ldx<SH>            (r-1) 2^SH (a canonical element of memory)          vprev  r-1
      fe_mul(x, y)       floor(x y / 2^261) + r; x plain with a top limb (x >> 232) below 2^31, y scaled and below 2^261
      times32(x)         32 x, needs x < 2^256
      fe_add / fe_dbl    the sum / twice                                     fe_norm  the value
      fe_sub_red(a, b, PK)  a + K r, needs b <= (K-1) r                      fe_neg_red(b, PK)  K r (attained: b = 0), needs b <= (K-1) r
      condsub2(x)        x below 2r, else max(2r - 1, x - 2r); needs x <= 4r
      fe_reduce_soft(x)  min(x, 2r + 2^233 - 1); needs x < 2^261
      every value < 2^264 (the top limb is 32 bits); the result strictly below 3r (fe_canon_lt3p).
    Returns the largest value of the result.  Raises MagnitudeError where a precondition can fail, ValueError on text it does not know."""
    env = {}
    stored = None

    def need(cond, what, stmt):
        if not cond:
            raise MagnitudeError("%s in `%s`" % (what, stmt.strip()))

    def ev(x, stmt):
        x = x.strip()
        if _NAME.match(x):
            if x not in env:
                raise ValueError("`%s` is read before it is declared in `%s`" % (x, stmt.strip()))
            return env[x]
        if "?" in x:                                                       # A.accumulate ? ldx<0>(A.out, row) : fe_zero()
            cond, rest = x.split("?", 1)
            yes, no = rest.rsplit(":", 1)
            (va, sa), (vb, sb) = ev(yes, stmt), ev(no, stmt)
            return max(va, vb), max(sa, sb)
        m = _CALL.match(x)
        if not m:
            raise ValueError("unknown expression `%s` in `%s`" % (x, stmt.strip()))
        fn, targ, args = m.group(1), m.group(2), _split_args(m.group(3))
        if fn == "fe_zero":
            return 0, 0
        if fn == "ldx":
            sh = int(targ[1:-1])
            if sh not in (0, 5):
                raise ValueError("ldx shift in `%s`" % stmt.strip())
            return (R - 1) << sh, sh
        if fn == "fe_mul":
            (va, sa), (vb, sb) = ev(args[0], stmt), ev(args[1], stmt)
            need(sa == 0 and sb == 5, "fe_mul takes a plain first and a scaled second factor", stmt)
            # fp29.hpp: max(a_i) max(b_j) < 2^60.6; the second factor's limbs are below 2^29 (fe_unpack), the first one's top limb is a >> 232
            need(va >> 232 < 1 << 31 and vb < 1 << 261, "fe_mul: a 64-bit product column can overflow", stmt)
            return (va * vb >> 261) + R, 0
        if fn == "times32":
            v, s = ev(args[0], stmt)
            need(s == 0, "times32 of a scaled value", stmt)
            need(v < 1 << 256, "times32 of a value that can reach 2^256 (%.3f r)" % (v / R), stmt)
            return 32 * v, 5
        if fn == "fe_norm":
            return ev(args[0], stmt)
        if fn in ("fe_add", "fe_dbl"):
            vals = [ev(arg, stmt) for arg in args] * (2 if fn == "fe_dbl" else 1)
            need(all(s == 0 for _, s in vals), fn + " of a scaled value", stmt)
            return sum(v for v, _ in vals), 0
        if fn in ("fe_sub_red", "fe_neg_red"):
            km = re.match(r"^Fr::P(\d+)_S1$", args[-1])
            if not km:
                raise ValueError("unknown multiple of r in `%s`" % stmt.strip())
            k = int(km.group(1))
            vals = [ev(arg, stmt) for arg in args[:-1]]
            need(all(s == 0 for _, s in vals), fn + " of a scaled value", stmt)
            need(vals[-1][0] <= (k - 1) * R, "%d r minus a value that can reach %.3f r borrows" % (k, vals[-1][0] / R), stmt)
            return (vals[0][0] if fn == "fe_sub_red" else 0) + k * R, 0
        if fn == "condsub2":
            v, s = ev(args[0], stmt)
            need(s == 0, "condsub2 of a scaled value", stmt)
            need(v <= 4 * R, "condsub2 of a value that can reach %.3f r" % (v / R), stmt)
            return (v if v < 2 * R else max(2 * R - 1, v - 2 * R)), 0
        if fn == "fe_reduce_soft":
            v, s = ev(args[0], stmt)
            need(s == 0, "fe_reduce_soft of a scaled value", stmt)
            need(v < 1 << 261, "fe_reduce_soft of a value that can reach 2^261", stmt)
            return min(v, 2 * R + (1 << 233) - 1), 0
        raise ValueError("unknown function `%s` in `%s`" % (fn, stmt.strip()))

    def assign(name, expr, stmt):
        v = ev(expr, stmt)
        need(v[0] < 1 << 264, "`%s` can reach 2^264" % name, stmt)
        env[name] = v

    lines = kernel_body(source).replace("fe_mul<Fr, false>(", "fe_mul(").splitlines()      # (the one template list with a comma)
    for stmt in lines[1:]:
        s = stmt.strip()
        if not s or s.startswith("//") or s == "}" or s.startswith("const uint64_t row =") or s == "if (row >= A.rows) return;":
            continue
        if stored is not None:
            raise ValueError("text after the result: `%s`" % s)
        m = re.match(r"^fe (r\d+ = fe_zero\(\)(?:, r\d+ = fe_zero\(\))*);$", s)
        if m:
            for name in re.findall(r"(r\d+) =", m.group(1)):
                env[name] = (0, 0)
            continue
        m = re.match(r"^const fe (t\d+|vprev|vpow) = (.*);$", s)
        if m:
            if m.group(1) in env:
                raise ValueError("`%s` is declared twice" % m.group(1))
            assign(m.group(1), m.group(2), stmt)
            continue
        m = re.match(r"^(r\d+) = (.*);$", s)
        if m:
            if m.group(1) not in env:
                raise ValueError("`%s` is assigned but not declared" % m.group(1))
            assign(m.group(1), m.group(2), stmt)
            continue
        m = re.match(r"^\{ uint32_t w\[8\]; fe_pack\(fe_canon_lt3p<Fr>\((r\d+)\), w\); store_words\(A\.out \+ row \* 8, w\); \}$", s)
        if m:
            v, sc = ev(m.group(1), stmt)
            need(sc == 0, "the result is a scaled value", stmt)
            need(v < 3 * R, "fe_canon_lt3p of a value that can reach %s" % ("exactly 3 r" if v == 3 * R else "%.3f r" % (v / R)), stmt)
            stored = v
            continue
        raise ValueError("unknown statement `%s`" % s)
    if stored is None:
        raise ValueError("the kernel stores no result")
    return stored


# ---- seeded random programs whose bounds climb ------------------------------------------------------------------------------------------------
def random_program(seed):
    """up to 256 instructions over two columns and few registers, the opcodes skewed towards add / sub / neg / dbl so that the lazy bounds reach
    the thresholds; registers may be read before they are written (they start at 0); a third of the programs use omega^row, a third PREV"""
    rng = random.Random(seed)
    use_pow, use_prev = seed % 3 == 1, seed % 3 == 2 or seed % 7 == 1
    p = E.RowProgram(rot_scale=rng.choice([1, 2]), omega=F.omega_for(6) if use_pow else None)
    n_regs = rng.choice([2, 3, 4, 6, 16])
    ops = [E.OP_ADD] * 8 + [E.OP_SUB] * 5 + [E.OP_NEG] * 3 + [E.OP_DBL] * 3 + [E.OP_MOV, E.OP_MUL, E.OP_MUL, E.OP_SQR, E.OP_MAD, E.OP_MAD]
    if seed % 5 == 0:
        ops = list(range(8))
    reg_weight = rng.choice([1, 3, 8])

    def operand():
        kinds = ["const", "col"] + ["reg"] * reg_weight + (["prev"] if use_prev else []) + (["rowpow"] if use_pow else [])
        k = rng.choice(kinds)
        if k == "const": return p.constant(rng.choice([0, 1, R - 1, rng.randrange(R)]))
        if k == "col": return p.column(rng.randrange(2), rng.choice([0, 0, 1, -1, 3]))
        if k == "reg": return REG(rng.randrange(n_regs))
        return E.RowProgram.PREV if k == "prev" else E.RowProgram.ROWPOW

    for _ in range(rng.choice([rng.randrange(1, 24), rng.randrange(24, 257), 256])):
        p.emit(rng.choice(ops), rng.randrange(n_regs), operand(), operand(), operand())
    p.result_reg = rng.randrange(n_regs)
    return p


# ---- jobs for the compiled executor -------------------------------------------------------------------------------------------------------------
# One job is one zkhip_fr_eval_rows call; `compiled`: whether it must go through a compiled kernel under ZKHIP_VM_JIT=2.
Job = namedtuple("Job", "label prog cols log_rows prev compiled")
GROUP = 8
N_GROUPS = (len(DIRECTED) + GROUP - 1) // GROUP


def _uses_prev(prog):
    return any(o[0] == E.SRC_PREV for insn in prog.insns for o in insn[2:2 + E._N_OPERANDS[insn[0]]])


def directed_job(d):
    return Job(d.name, d.prog, grid_columns(6), 6, prev_column(6) if _uses_prev(d.prog) else None, True)


def chain_program(n_insns, c=R - 1):
    """`n_insns` instructions of the add / sub / dbl / neg / mad chain of tests/test_gpu_rows.py (cut where the count is reached)"""
    p = E.RowProgram()
    a, b = p.column(0), p.column(1)
    p.emit(E.OP_ADD, 0, a, b)
    cycle = [lambda: p.emit(E.OP_DBL, 1, REG(0)),
             lambda: p.emit(E.OP_SUB, 2, REG(1), b),
             lambda: p.emit(E.OP_NEG, 3, REG(2)),
             lambda: p.emit(E.OP_ADD, 0, REG(3), REG(1)),
             lambda: p.emit(E.OP_SUB, 0, REG(0), p.constant(c)),
             lambda: p.emit(E.OP_MAD, 0, REG(0), p.constant(c), REG(2))]
    i = 0
    while len(p.insns) < n_insns:
        cycle[i % len(cycle)]()
        i += 1
    p.result_reg = 0
    return p


def wide_program(n_columns):
    """reads every one of `n_columns` columns: sums and differences, then a product with the last one"""
    p = E.RowProgram()
    p.emit(E.OP_MOV, 0, p.column(0))
    for i in range(1, n_columns):
        p.emit(E.OP_SUB if i % 3 == 0 else E.OP_ADD, 0, REG(0), p.column(i, (i % 3) - 1))
    p.emit(E.OP_MUL, 1, REG(0), p.column(n_columns - 1))
    p.result_reg = 1
    return p


def wide_columns(n_columns, log_rows=6):
    rng = random.Random(22)
    g = grid_columns(log_rows)
    return [g[i % 2] if i % 4 < 2 else [rng.randrange(R) for _ in range(1 << log_rows)] for i in range(n_columns)]


def constants_only_program():
    """no column at all: constants and omega^row"""
    p = E.RowProgram(omega=F.omega_for(6))
    p.emit(E.OP_MUL, 0, E.RowProgram.ROWPOW, p.constant(5))
    p.emit(E.OP_MAD, 1, REG(0), E.RowProgram.ROWPOW, p.constant(R - 1))
    p.emit(E.OP_SUB, 2, REG(1), E.RowProgram.ROWPOW)
    p.emit(E.OP_NEG, 3, REG(2))
    p.emit(E.OP_ADD, 3, REG(3), p.constant(0))
    p.result_reg = 3
    return p


def rotation_program(r0, r1, omega=None):
    p = E.RowProgram(rot_scale=2, omega=omega)
    p.emit(E.OP_MUL, 0, p.column(0, r0), p.column(1, r1))
    p.emit(E.OP_NEG, 1, REG(0))
    p.emit(E.OP_MAD, 2, REG(1), E.RowProgram.PREV, p.column(0, r1))
    p.emit(E.OP_SUB, 3, REG(2), E.RowProgram.PREV)
    if omega is not None:
        p.emit(E.OP_MUL, 3, REG(3), E.RowProgram.ROWPOW)
    p.result_reg = 3
    return p


def reuse_jobs():
    """what one cached kernel must serve, and what must not be served by it: in one process, in this order"""
    g6, g7 = grid_columns(6), grid_columns(7)
    rot = rotation_program(1, -1)
    return [
        Job("constants_first", chain_program(40, R - 1), g6, 6, None, True),
        Job("constants_other_values", chain_program(40, 12345), g6, 6, None, True),            # the same instructions: the constants are a table
        Job("accumulate_off", rot, g6, 6, None, True),
        Job("accumulate_on", rot, g6, 6, prev_column(6), True),                                # the same kernel, PREV = out
        Job("rotations_other_values", rotation_program(2, -3), g6, 6, prev_column(6), True),   # the same slots: the offsets are literals
        Job("rows_64", rotation_program(1, -1, F.omega_for(6)), g6, 6, prev_column(6), True),
        Job("rows_128", rotation_program(1, -1, F.omega_for(7)), g7, 7, prev_column(7), True),  # the row mask and omega change
        Job("rows_64_again", rotation_program(1, -1, F.omega_for(6)), g6, 6, None, True),
    ]


def limit_jobs():
    g6 = grid_columns(6)
    return [
        Job("insns_256", chain_program(256), g6, 6, None, True),
        Job("insns_257", chain_program(257), g6, 6, None, False),
        Job("columns_96", wide_program(96), wide_columns(96), 6, None, True),
        Job("columns_97", wide_program(97), wide_columns(97), 6, None, False),
        Job("no_column", constants_only_program(), [], 6, None, True),
    ]


def jobs_of(scenario):
    """`directed:<group>`, `reuse`, `limits`"""
    if scenario.startswith("directed:"):
        g = int(scenario.split(":")[1])
        return [directed_job(d) for d in DIRECTED[g * GROUP:(g + 1) * GROUP]]
    return {"reuse": reuse_jobs, "limits": limit_jobs}[scenario]()


def expected_bytes(job):
    """the oracle's interpreter (oracle/bn254.py) on the job, as the canonical bytes zkhip_fr_eval_rows writes"""
    from oracle import bn254 as O

    p = job.prog
    vals = O.row_program_run(p.insns, p.constants, p.rotations, p.rot_scale, p.result_reg, job.cols, job.log_rows, omega=p.omega, prev=job.prev)
    return F.fr_encode(vals).tobytes()


def run_job(lib, job):
    """(bytes written, how many launches went through a compiled kernel) of one zkhip_fr_eval_rows call"""
    out = F.fr_encode(job.prev) if job.prev is not None else None
    before = lib.zkhip_test_rows_compiled_count()
    res = job.prog.run([F.fr_encode(c) for c in job.cols], job.log_rows, out=out, accumulate=job.prev is not None)
    return res.tobytes(), lib.zkhip_test_rows_compiled_count() - before


def child_main(scenario):
    """runs in a fresh process (the executor switch $ZKHIP_VM_JIT is read once per process): one JSON line per job"""
    from zksnap_circuits_halo2_amd import _lib

    lib = _lib.load()
    for job in jobs_of(scenario):
        got, compiled = run_job(lib, job)
        print("JOB " + json.dumps({"label": job.label, "compiled": compiled, "out": got.hex()}), flush=True)


if __name__ == "__main__":
    child_main(sys.argv[1])

"""`halo2_proofs::dev::MockProver` over device-resident columns: does this witness satisfy its circuit, and if not, where.

The reference never calls `create_proof` on an unchecked witness: `gen_proof` runs `MockProver::run(k, &circuit, instances)
.assert_satisfied()` first (/root/reference/aggregator/src/wrapper.rs:117-123).  Here the three questions MockProver asks are three
read-only passes over the columns the prover needs in HBM anyway (include/zkhip.h, "witness checks"):

  gates     every polynomial of every gate is zero on rows [0, n - blinding_factors - 1)     zkhip_check_rows_device
  copies    every cell equals the cell the permutation maps it to, on all rows               zkhip_check_copies_device
  lookups   every compressed input value occurs among the compressed table values,
            both over the usable rows                                                        zkhip_check_lookups_device

Each pass reduces on the device to (number of failing items, lowest failing index); `MockProver.verify()` turns those records into a sorted
list of failures and `assert_satisfied()` raises with it.  `verify_host` is the same contract in plain Python integers, with no device.

Lookups are compressed with a caller-supplied theta, as the prover does.  For a lookup of ONE input and ONE table column -- the range
lookups of the halo2-lib shapes -- the compressed column is the column itself and the check is exact.  For several columns it is a
random-theta test: a tuple that is not in the table is reported unless theta happens to be a root of a non-zero polynomial of degree below
the number of columns (probability at most (columns - 1) / r for a uniform theta), and a caller who fixes theta gets what that theta gives.

Not covered (halo2's MockProver does more): its unassigned-cell (`Poison`) diagnostics -- every cell of a column in HBM has a value;
selector and region bookkeeping -- failures are located by gate, polynomial and row, not by region and offset; row-shard sets and devices
other than the one the stream belongs to -- the columns are whole columns on one device."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import evaluation as E
from . import fields as F
from .buffers import DeviceBuffer
from .tensors import fr_ints

NONE = (1 << 64) - 1          # `first` of a record without failures
DEFAULT_THETA = 0x2545F4914F6CDD1D_9E3779B97F4A7C15_BF58476D1CE4E5B9_94D049BB133111EB % F.R_MOD


# ---------------------------------------------------------------------------------------------------
# gates -> row programs
# ---------------------------------------------------------------------------------------------------
def gate_polynomials(cs: E.ConstraintSystem) -> List[Tuple[int, int, E.Expr]]:
    """(gate, polynomial within the gate, expression) in the order of `cs.gates`"""
    return [(gi, pi, poly) for gi, polys in enumerate(cs.gates) for pi, poly in enumerate(polys)]


def gate_programs(cs: E.ConstraintSystem, challenges: Sequence[int] = ()) -> List[E.RowProgram]:
    """Every polynomial of every gate as a row program of its own over the base domain (rot_scale = 1), in the order of `gate_polynomials`.
    Columns: fixed, advice, instance, as `evaluation.quotient_columns` numbers them."""
    qc = E.quotient_columns(cs)
    progs = []
    for _, _, poly in gate_polynomials(cs):
        g = E.Graph()
        progs.append(E.compile_graph(g, E._add_expression(g, cs, qc, poly, challenges), rot_scale=1))
    return progs


def _compressed_program(cs: E.ConstraintSystem, exprs: Sequence[E.Expr], theta: int, challenges: Sequence[int]) -> E.RowProgram:
    qc = E.quotient_columns(cs)
    g = E.Graph()
    parts = [E._add_expression(g, cs, qc, e, challenges) for e in exprs]
    return E.compile_graph(g, g.horner(g.const(0), parts, g.const(theta)), rot_scale=1)


def _plain_column(cs: E.ConstraintSystem, exprs: Sequence[E.Expr]) -> Optional[int]:
    """index (fixed, advice, instance numbering) of the column a one-expression list names at rotation 0, or None"""
    if len(exprs) != 1 or exprs[0].kind not in ("fixed", "advice", "instance") or (exprs[0].b or 0) != 0:
        return None
    qc = E.quotient_columns(cs)
    return {"fixed": qc.fixed, "advice": qc.advice, "instance": qc.instance}[exprs[0].kind] + exprs[0].a


# ---------------------------------------------------------------------------------------------------
# the three calls
# ---------------------------------------------------------------------------------------------------
def _addr(c) -> int:
    return c.data_ptr() if hasattr(c, "data_ptr") else (c.value if isinstance(c, C.c_void_p) else int(c))


def _pointers(cols):
    return (C.c_void_p * max(len(cols), 1))(*[_addr(c) for c in cols])


def enqueue_check_rows(progs: Sequence[E.RowProgram], d_columns, log_rows: int, row0: int, count: int, d_reports: int, stream=None) -> None:
    """zkhip_check_rows_device: d_reports receives len(progs) records; nothing is read back here"""
    marshalled = [p._marshal() for p in progs]
    arr = (_lib.VmProgram * max(len(progs), 1))(*[m[0] for m in marshalled])
    _lib.check(_lib.load().zkhip_check_rows_device(arr, len(progs), _pointers(d_columns), len(d_columns), log_rows, row0, count, C.c_void_p(d_reports),
                                                  C.c_void_p(stream)))


def enqueue_check_copies(d_columns, log_n: int, d_map_col: int, d_map_row: int, d_report: int, stream=None) -> None:
    """zkhip_check_copies_device: d_map_col / d_map_row are [columns][2^log_n] u32 on the device"""
    _lib.check(_lib.load().zkhip_check_copies_device(_pointers(d_columns), len(d_columns), log_n, C.c_void_p(d_map_col), C.c_void_p(d_map_row),
                                                    C.c_void_p(d_report), C.c_void_p(stream)))


def enqueue_check_lookups(d_inputs, d_tables, log_n: int, usable_rows: int, d_reports: int, stream=None) -> None:
    """zkhip_check_lookups_device: compressed input / table columns; equal table addresses are one table"""
    if len(d_inputs) != len(d_tables):
        raise ValueError("as many tables as inputs")
    _lib.check(_lib.load().zkhip_check_lookups_device(_pointers(d_inputs), _pointers(d_tables), len(d_inputs), log_n, usable_rows, C.c_void_p(d_reports),
                                                     C.c_void_p(stream)))


def read_reports(d_reports: int, count: int, stream=None) -> List[Tuple[int, int]]:
    """(failures, first) of `count` records, after the stream has finished"""
    lib = _lib.load()
    out = np.zeros((max(count, 1), 2), dtype=np.uint64)
    if count:
        _lib.check(lib.zkhip_stream_sync(C.c_void_p(stream)))
        _lib.check(lib.zkhip_download(out.ctypes.data, C.c_void_p(d_reports), count * 16))
    return [(int(out[i, 0]), int(out[i, 1])) for i in range(count)]


# ---------------------------------------------------------------------------------------------------
# MockProver
# ---------------------------------------------------------------------------------------------------
class MockProver:
    """MockProver(cs, k, fixed, advice, instance, assembly): `fixed` / `advice` / `instance` are the circuit's columns in HBM ((2^k, 4) int64
    device tensors, or device addresses), `assembly` the `keygen.Assembly` of its copy constraints (None: no permutation).  `verify()`
    returns the sorted list of
        ("gate", gate, polynomial, first failing row, failing rows)
        ("copy", permutation column, row, failing cells)          the failing cell with the lowest column 2^k + row
        ("lookup", lookup, first failing row, failing rows)
    and [] for a satisfied witness.  The columns are read where they lie; the object owns a few small device buffers (the records, the
    permutation's mapping, compressed lookup columns when an expression is not a plain column) until `close()`."""

    def __init__(self, cs: E.ConstraintSystem, k: int, fixed, advice, instance=(), assembly=None, theta: int = DEFAULT_THETA, challenges: Sequence[int] = (),
                 stream=None):
        if len(fixed) != cs.num_fixed or len(advice) != cs.num_advice or len(instance) != cs.num_instance:
            raise ValueError("columns do not match the constraint system")
        self.cs, self.k, self.n, self.stream = cs, k, 1 << k, stream
        self.usable = self.n - (cs.blinding_factors + 1)
        if self.usable <= 0:
            raise ValueError("no usable rows")
        self.columns = list(fixed) + list(advice) + list(instance)            # evaluation.quotient_columns order
        self.gates = gate_polynomials(cs)
        self.programs = gate_programs(cs, challenges)
        self._buffers = []

        def buffer(nbytes):
            b = DeviceBuffer(nbytes)
            self._buffers.append(b)
            return b

        try:
            self.n_perm = len(cs.permutation_columns) if assembly is not None else 0
            if self.n_perm:
                if assembly.n_columns != self.n_perm or assembly.n != self.n:
                    raise ValueError("the assembly does not match the constraint system")
                qc = E.quotient_columns(cs)
                base = {"fixed": qc.fixed, "advice": qc.advice, "instance": qc.instance}
                self.perm_columns = [self.columns[base[kind] + idx] for kind, idx in cs.permutation_columns]
                self._maps = buffer(2 * self.n_perm * self.n * 4)                 # [map_col | map_row], [column][row] u32 each
                self._maps.upload(np.ascontiguousarray(assembly.map_col, dtype=np.uint32))
                self._maps.upload(np.ascontiguousarray(assembly.map_row, dtype=np.uint32), self.n_perm * self.n * 4)
            # lookups: a plain column is its own compressed column; anything else is evaluated into a column of this object, once per
            # distinct expression list, so that a table shared by several lookups keeps one address (and is sorted once)
            self._compress, made = [], {}
            self.lookup_inputs, self.lookup_tables = [], []
            for lk in cs.lookups:
                pair = []
                for exprs in (lk.input_expressions, lk.table_expressions):
                    plain = _plain_column(cs, exprs)
                    if plain is not None:
                        pair.append(self.columns[plain])
                        continue
                    key = tuple(exprs)
                    if key not in made:
                        made[key] = buffer(self.n * 32)
                        self._compress.append((_compressed_program(cs, exprs, theta, challenges), made[key]))
                    pair.append(made[key].ptr.value)
                self.lookup_inputs.append(pair[0])
                self.lookup_tables.append(pair[1])
            self.n_records = len(self.programs) + (1 if self.n_perm else 0) + len(cs.lookups)
            self._reports = buffer(16 * max(self.n_records, 1))
        except Exception:
            self.close()
            raise

    def close(self) -> None:
        for b in self._buffers:
            b.free()
        self._buffers = []

    def __enter__(self) -> "MockProver":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def enqueue(self) -> None:
        """the three checks on the stream; the records stay on the device"""
        base, ptrs = self._reports.ptr.value, [_addr(c) for c in self.columns]
        for prog, out in self._compress:
            prog.run_device(ptrs, self.k, out.ptr.value, stream=self.stream or 0)
        if self.programs:
            enqueue_check_rows(self.programs, ptrs, self.k, 0, self.usable, base, self.stream)
        if self.n_perm:
            maps = self._maps.ptr.value
            enqueue_check_copies(self.perm_columns, self.k, maps, maps + self.n_perm * self.n * 4, base + 16 * len(self.programs), self.stream)
        if self.cs.lookups:
            enqueue_check_lookups(self.lookup_inputs, self.lookup_tables, self.k, self.usable, base + 16 * (len(self.programs) + (1 if self.n_perm else 0)), self.stream)

    def verify(self) -> list:
        self.enqueue()
        rec = read_reports(self._reports.ptr.value, self.n_records, self.stream)
        out = []
        for (gi, pi, _), (failures, first) in zip(self.gates, rec):
            if failures:
                out.append(("gate", gi, pi, first, failures))
        at = len(self.programs)
        if self.n_perm:
            failures, first = rec[at]
            if failures:
                out.append(("copy", first >> self.k, first & (self.n - 1), failures))
            at += 1
        for li in range(len(self.cs.lookups)):
            failures, first = rec[at + li]
            if failures:
                out.append(("lookup", li, first, failures))
        return sorted(out)

    def assert_satisfied(self) -> None:
        failures = self.verify()
        if failures:
            raise AssertionError(f"the witness does not satisfy the circuit: {failures}")


# ---------------------------------------------------------------------------------------------------
# the same contract in plain Python integers
# ---------------------------------------------------------------------------------------------------
def _ints(col) -> List[int]:
    return fr_ints(col) if isinstance(col, np.ndarray) else [int(v) % F.R_MOD for v in col]


def _evaluate(e: E.Expr, cols, row: int, n: int, challenges: Sequence[int]) -> int:
    k = e.kind
    if k == "constant": return e.a
    if k in ("fixed", "advice", "instance"): return cols[k][e.a][(row + (e.b or 0)) % n]
    if k == "challenge": return challenges[e.a] % F.R_MOD
    if k == "neg": return -_evaluate(e.a, cols, row, n, challenges) % F.R_MOD
    if k == "sum": return (_evaluate(e.a, cols, row, n, challenges) + _evaluate(e.b, cols, row, n, challenges)) % F.R_MOD
    if k == "product": return _evaluate(e.a, cols, row, n, challenges) * _evaluate(e.b, cols, row, n, challenges) % F.R_MOD
    if k == "scaled": return _evaluate(e.a, cols, row, n, challenges) * e.b % F.R_MOD
    raise ValueError(k)


def verify_host(cs: E.ConstraintSystem, k: int, fixed, advice, instance=(), assembly=None, theta: int = DEFAULT_THETA, challenges: Sequence[int] = ()) -> list:
    """What `MockProver(...).verify()` returns, computed from host columns ((2^k, 4) uint64 word arrays or lists of integers) in Python
    integers: no device, no library call."""
    n = 1 << k
    usable = n - (cs.blinding_factors + 1)
    cols = {"fixed": [_ints(c) for c in fixed], "advice": [_ints(c) for c in advice], "instance": [_ints(c) for c in instance]}
    out = []
    for gi, pi, poly in gate_polynomials(cs):
        bad = [r for r in range(usable) if _evaluate(poly, cols, r, n, challenges) != 0]
        if bad:
            out.append(("gate", gi, pi, bad[0], len(bad)))
    if assembly is not None and cs.permutation_columns:
        perm = [cols[kind][idx] for kind, idx in cs.permutation_columns]
        npc = len(perm)
        mc, mr = np.asarray(assembly.map_col).astype(np.int64) % npc, np.asarray(assembly.map_row).astype(np.int64) % n
        moved = np.nonzero((mc != np.arange(npc)[:, None]) | (mr != np.arange(n)[None, :]))          # a cell that maps to itself cannot fail
        bad = [(int(c), int(r)) for c, r in zip(*moved) if perm[c][r] != perm[mc[c, r]][mr[c, r]]]
        if bad:
            out.append(("copy", bad[0][0], bad[0][1], len(bad)))                                     # np.nonzero walks the [column][row] array in order: the lowest column 2^k + row first
    for li, lk in enumerate(cs.lookups):
        def compressed(exprs, r):
            v = 0
            for e in exprs:
                v = (v * theta + _evaluate(e, cols, r, n, challenges)) % F.R_MOD
            return v
        table = {compressed(lk.table_expressions, r) for r in range(usable)}
        bad = [r for r in range(usable) if compressed(lk.input_expressions, r) not in table]
        if bad:
            out.append(("lookup", li, bad[0], len(bad)))
    return sorted(out)

"""A `create_proof` for circuits of the halo2-lib shape (evaluation.halo2_lib_shape), device-resident from the witness columns to the
multi-open -- the steps of [DEP] halo2-axiom plonk/prover.rs, each a method of `Prover`:

  halo2_lib_witness   fixed and advice columns, lookup inputs, the table, the copy cycles, the Assembly and the ConstraintSystem
  Prover              one proof: advice commitments, permutation products, the lookup argument (every lookup in one call, or one at a time),
                      the vanishing argument's random polynomial, Lagrange -> coefficients, the extended coset, the quotient (one program, a sum
                      of parts, or row-sharded), the h commitments, the evaluations, the SHPLONK multi-open
  TorchBlinding / DeviceBlinding          where blinding rows come from
  SeededChallenges / TranscriptChallenges where challenges come from; each has its own order of steps (Prover._seeded, Prover._transcript)
  opening_plan        the opened (kind, index, rotation) triples; the prover and both verifiers turn them into queries through one
                      (kind, index) map each
The verifier of the proofs written here is verifier.py; it is handed the plan.

`lap` is a callable handed a name at every phase boundary (tools/prove_flow.py times the phases with it); None: no laps, so no synchronisation
is added for timing (the phases that read a value back -- whether a product closes, the evaluations as integers -- still wait for it)."""
import ctypes as C
import functools
import io
import random
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, evaluation as E, fields as F, keygen as KG, multiopen as MO, tensors as T
from .domain import EvaluationDomain
from .transcript import transcript_classes, vk_transcript_repr
from .verifier import key_commitments, verifier_queries

R = F.R_MOD
BLIND = 5
DEV = torch.device("cuda", 0)

_SIDE_STREAM = None


def side_stream():
    """the high-priority stream commits alternate onto: one per process, kept between proofs like the scratch set the library keys by it"""
    global _SIDE_STREAM
    if _SIDE_STREAM is None:
        _SIDE_STREAM = torch.cuda.Stream(priority=-1)
    return _SIDE_STREAM


empty = functools.partial(T.fr_empty, device=DEV)
rand_fr = functools.partial(T.fr_random, device=DEV)
words = functools.partial(T.fr_words, device=DEV)      # python ints -> device tensor of Montgomery words
small_ints = T.fr_from_small                           # int64 tensor of 2^k small non-negative integers on DEV -> Montgomery words


def run_prog(prog, cols, log_rows, out=None):
    if out is None:
        out = empty(1 << log_rows)
    prog.run_device([c.data_ptr() for c in cols], log_rows, out.data_ptr())
    return out


def affine(jac):
    return F.g1_decode_jacobian(jac.cpu().numpy().view(np.uint64))


# ---- where blinding rows come from ------------------------------------------------------------------------------------------------------------
# A phase makes the same calls whatever the source; each source draws in the calls of its own order, the others do nothing:
#                  column(n)                  made(col, row0)        ahead(count)                 step(cols, row0)
#   TorchBlinding  draws all n rows           draws rows row0 ..     draws `count` rows, returned nothing
#   DeviceBlinding allocates, draws nothing   nothing                nothing (None)               draws rows row0 .. of all cols, one call
# random_polynomial: None where the source has none (the seeded flow with torch never committed one), else n -> coefficients.
class TorchBlinding:
    """torch's generator (the caller seeds it): one draw per column, at the moment the column is made"""

    def column(self, n, out=None):       # a new column, random in every row: what is computed into it leaves the blinding rows as drawn
        r = rand_fr(n)
        return r if out is None else out.copy_(r)

    def made(self, col, row0):           # a column has just been computed
        col[row0:] = rand_fr(col.shape[0] - row0)

    def ahead(self, count):              # the tail of a column that does not exist yet
        return rand_fr(count)

    def step(self, cols, row0): pass     # all columns of a step exist: theirs are drawn already

    random_polynomial = None


class DeviceBlinding:
    """the library's random stream (E.blind_rows_device): the tails of all columns of a step in one call, every stream index used once"""

    def __init__(self, seed: bytes):
        self.seed, self.first = seed, 0

    def column(self, n, out=None):
        return empty(n) if out is None else out

    def made(self, col, row0): pass
    def ahead(self, count): return None

    def step(self, cols, row0):
        count = cols[0].shape[0] - row0
        E.blind_rows_device(cols, row0, count, self.seed, first=self.first)
        self.first += len(cols) * count

    def random_polynomial(self, n):      # the vanishing argument's: n coefficients of stream 1, drawn where they are committed and opened
        return E.random_fr_device(self.seed, n, stream_id=1)


# ---- where challenges come from --------------------------------------------------------------------------------------------------------------
class SeededChallenges:
    """every challenge drawn up front from random.Random(seed), in the order beta, gamma, theta, y, x, the trapdoor `s` of a test SRS, and the
    multi-open's y, v, u; the commitments handed in are ignored"""
    transcript = None

    def __init__(self, seed):
        rng = random.Random(seed)
        self._beta, self._gamma, self._theta, self._y, self._x, self.s = (rng.randrange(1, R) for _ in range(6))
        self.multiopen_challenges = tuple(rng.randrange(1, R) for _ in range(3))

    def instances(self, values): pass
    def theta(self, points=()): return self._theta
    def beta_gamma(self, points=()): return self._beta, self._gamma
    def y(self, points=()): return self._y
    def x(self, points=()): return self._x

    def multiopen(self, prover, queries):
        return prover.create_proof(queries, *self.multiopen_challenges)      # raises if L(u) != 0: an evaluation that does not belong to its polynomial

    def finish(self):
        return None


class TranscriptChallenges:
    """Fiat-Shamir: a transcript opened with the verifying key; each challenge is squeezed after the commitments handed in (Jacobian
    points on the device) have been written.  `finish()` returns the proof bytes.  hash: "blake2b" (the benches' `gen_proof`) or "poseidon"
    (`gen_snark`'s `PoseidonTranscript`): the same calls and the same proof layout, other challenges."""

    def __init__(self, vk, hash="blake2b"):
        vk_io = io.BytesIO()
        vk.write(vk_io, KG.RAW_BYTES)
        self.transcript = transcript_classes(hash)[0]()
        self.transcript.common_scalar(vk_transcript_repr(vk_io.getvalue()))      # a stand-in for halo2's vk.transcript_repr (transcript.py)

    def instances(self, values):
        """the public inputs, absorbed (never written) between the key and the advice commitments: every value of every instance column, as
        halo2's `create_proof` and `verify_proof` both do.  No instance column: nothing is absorbed."""
        for column in values:
            for v_ in column:
                self.transcript.common_scalar(v_)

    def _after(self, points):
        if len(points):
            self.transcript.write_points(torch.stack(list(points)).contiguous())
        return self.transcript.squeeze_challenge()

    theta = y = x = _after

    def beta_gamma(self, points=()):
        return self._after(points), self.transcript.squeeze_challenge()

    def write_scalars(self, scalars):
        self.transcript.write_scalars(scalars)

    def multiopen(self, prover, queries):                                        # y, v and u are squeezed, H and H' written
        return prover.create_proof_transcript(queries, self.transcript)

    def finish(self):
        proof = self.transcript.finalize()
        self.transcript.close()
        return proof


# ---- the opening plan ------------------------------------------------------------------------------------------------------------------------------
def opening_plan(cs, gate_cols, lookups, usable_rows, random_poly=False, order="halo2"):
    """The opened (kind, index, rotation) triples of the halo2-lib shape.  order "halo2": the order halo2 writes its evaluations in -- advice;
    fixed; the random polynomial; sigma; per permutation set z(x), z(omega x) and, for all but the last set, z(omega^last x); per lookup
    product, product-next, permuted input, permuted input at omega^-1 x, permuted table -- and then the three quotient pieces (this prover opens
    them one by one; halo2 opens their combination, whose value its verifier computes).  order "seeded": the same triples with the fixed columns
    first, as the seeded flow has always opened them."""
    G, NL, sets = gate_cols, lookups, cs.num_permutation_sets
    advice = [("advice", i, r) for i in range(G) for r in range(4)] + [("advice", G + j, 0) for j in range(NL)]      # the vertical gate reads rows 0 .. 3
    fixed = [("fixed", i, 0) for i in range(cs.num_fixed)]
    random_ = [("random", 0, 0)] if random_poly else []
    rest = [("sigma", i, 0) for i in range(len(cs.permutation_columns))]
    rest += [("perm", si, r) for si in range(sets) for r in (0, 1) + ((usable_rows,) if si + 1 < sets else ())]      # the last usable row chains the sets
    rest += [(kind, j, r) for j in range(NL) for kind, r in (("lookup_z", 0), ("lookup_z", 1), ("lookup_pa", 0), ("lookup_pa", -1), ("lookup_ps", 0))]
    rest += [("h", i, 0) for i in range(3)]
    if order == "halo2":
        return advice + fixed + random_ + rest
    if order == "seeded":
        return fixed + advice + random_ + rest
    raise ValueError("opening_plan: order is \"halo2\" or \"seeded\"")


# ---- the witness -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Witness:
    """a circuit of the halo2-lib shape and an assignment to it: Lagrange-basis columns on the device"""
    k: int
    gate_cols: int
    lookups: int
    cs: E.ConstraintSystem
    fixed: list                           # q_0 .., the constants column, the table
    advice: list                          # the gate columns, then the lookup inputs
    assembly: KG.Assembly
    instance: list = field(default_factory=list)           # the public inputs: values in the first rows, zeros behind them, NO blinding rows (halo2 pads with zeros)
    instance_values: list = field(default_factory=list)    # ... and as integers, a list per column: what a verifier is handed

    @property
    def lookup_inputs(self): return self.advice[self.gate_cols:]
    @property
    def table(self): return self.fixed[self.gate_cols + 1]

    def permutation_column(self, c):      # every advice column, then the constants column, then the instance columns
        if c < len(self.advice):
            return self.advice[c]
        return self.fixed[self.gate_cols] if c == len(self.advice) else self.instance[c - len(self.advice) - 1]


def halo2_lib_witness(k, gate_cols, lookups, blinding, lookup_bits=8, corrupt=None, instances=0, instance_len=4, public_inputs=None):
    """A satisfied circuit: `gate_cols` advice columns with the vertical gate q (a + b c - d) on rows 0, 4, 8, ..., `lookups` range-lookup
    columns against a 2^lookup_bits-entry table, copy constraints across advice and constants columns, BLIND blinding rows.
    instances: that many instance columns of `instance_len` public values each; public value t (counted through the columns) is tied by a
    copy constraint to the gate input in row 4 (t // gate_cols) + 2 of gate column t % gate_cols, whose value it takes -- or, with
    public_inputs (a list of `instance_len` integers per column), which is given that value first: proofs of one key over different inputs.
    corrupt: "gate" / "copy" break the witness; "lookup" puts a value outside the table into lookup column 1; "instance" gives the gate
    input behind the first public value another value (the gates stay satisfied, the copy constraint does not)."""
    G, NL = gate_cols, lookups
    n, u = 1 << k, (1 << k) - (BLIND + 1)
    lookup_bits = min(lookup_bits, k - 1)            # every table value must occur among the usable rows
    ONE = words([1])[0]
    rows = torch.arange(n, dtype=torch.int64, device=DEV)
    gate_rows = (rows % 4 == 0) & (rows + 3 < u)
    sel = torch.where(gate_rows[:, None], ONE[None, :], torch.zeros_like(ONE)[None, :]).contiguous()
    sel3 = torch.roll(sel, 3, 0).contiguous()                                  # 1 on the gates' output rows
    fixed = [sel.clone() for _ in range(G)] + [rand_fr(n), small_ints(rows % (1 << lookup_bits), k)]
    advice = [rand_fr(n) for _ in range(G)]
    for _ in range(NL):
        lk = small_ints(torch.randint(0, 1 << lookup_bits, (n,), dtype=torch.int64, device=DEV), k)
        blinding.made(lk, u)
        advice.append(lk)
    public_cells = [(t % G, 4 * (t // G) + 2) for t in range(instances * instance_len)] if instances else []
    if public_cells and (public_cells[-1][1] >= u or instance_len > u):
        raise ValueError(f"halo2_lib_witness: {instances} x {instance_len} public values do not fit the gate inputs of {G} columns over {u} usable rows")
    if corrupt == "instance" and not public_cells:
        raise ValueError("corrupt=\"instance\" needs an instance column with a value")
    w = Witness(k, G, NL, E.halo2_lib_shape(G, NL, BLIND, instances), fixed, advice, KG.Assembly(n, G + NL + 1 + instances))
    FC = G + NL                                                                # index of the constants column among the permutation columns
    cycles = [[(0, 1), (FC, 2)], [(G, 10), (G, 20)], [(0, 13), (G, 30)], [(0, 17), (0, 21), (FC, 5)]]
    cycles += [[(G + j, 40 + j), (G, 60 + j)] for j in range(1, NL)]           # lookup column j <-> lookup column 0
    if G > 1:
        cycles += [[(G - 1, 5), (FC, 7)], [(G // 2, 9), (G - 1, 25)]]          # the far gate columns take part in the permutation too
    for cyc in cycles:                    # equal values along every cycle (a cycle through a lookup column carries a table value)
        src = next(((c, r) for c, r in cyc if G <= c < FC), cyc[0])
        v = w.permutation_column(src[0])[src[1]].clone()
        for c, r in cyc:
            w.permutation_column(c)[r] = v
        for (c1, r1), (c2, r2) in zip(cyc, cyc[1:]):
            w.assembly.copy(c1, r1, c2, r2)
    if public_inputs is not None and [len(column) for column in public_inputs] != [instance_len] * instances:
        raise ValueError(f"public_inputs: {instances} lists of {instance_len} integers")
    for j in range(instances):            # the public inputs take the values of their cells (gate inputs: the gate program leaves them as they are)
        column = torch.zeros((n, 4), dtype=torch.int64, device=DEV)
        chosen = words([v_ % R for v_ in public_inputs[j]]) if public_inputs is not None and instance_len else None
        for i in range(instance_len):
            c, r = public_cells[j * instance_len + i]
            if chosen is not None:
                advice[c][r] = chosen[i]
            column[i] = advice[c][r]
            w.assembly.copy(c, r, FC + 1 + j, i)
        w.instance.append(column)
        w.instance_values.append(T.fr_ints(column[:instance_len]) if instance_len else [])
    if corrupt == "instance":
        c, r = public_cells[0]
        advice[c][r] = advice[c][r - 1].clone()                                # before the gate outputs are computed: every gate still holds
    gate = E.RowProgram()                 # out = a + sel3 * ((a[-3] + a[-2] a[-1]) - a): the gate outputs, everything else unchanged
    gate.emit(E.OP_MUL, 0, gate.column(0, -2), gate.column(0, -1))
    gate.emit(E.OP_ADD, 0, E.RowProgram.reg(0), gate.column(0, -3))
    gate.emit(E.OP_SUB, 0, E.RowProgram.reg(0), gate.column(0, 0))
    gate.emit(E.OP_MAD, 0, E.RowProgram.reg(0), gate.column(1, 0), gate.column(0, 0))
    for i in range(G):
        advice[i] = run_prog(gate, [advice[i], sel3], k)
    if corrupt == "gate":
        advice[0][7] = advice[0][8].clone()
    if corrupt == "copy":
        advice[0][21] = advice[0][22].clone()
    if corrupt == "lookup":
        advice[G + 1][3] = small_ints(torch.full((n,), 1 << lookup_bits, dtype=torch.int64, device=DEV), k)[3]      # one value outside the table
    blinding.step(advice, u)
    return w


# ---- the prover ------------------------------------------------------------------------------------------------------------------------------
def check_options(transcript, lookups, lookups_one_call, sharded_quotient, sharded_key):
    if sharded_key and not sharded_quotient:
        raise ValueError("sharded_key needs sharded_quotient")
    if transcript and lookups and not lookups_one_call:
        raise ValueError("transcript: the lookup argument is split at its challenges only in the one-call form")


class Prover:
    """One proof of one Witness.  `prove(dpk, challenges)` runs the phases in the order of the challenge source; `commit_advice()` may be called
    before the key exists.  Afterwards the object holds what the proof consists of (`commitments`, `plan`, `queries`, `multiopen_proof`, with a
    transcript `proof`) and what the prover's own invariants are read from (`*_closes`, `h_coeff`, `a0_coeff_commit`, `multiopen_ok`)."""

    def __init__(self, params, witness, blinding, batched=None, lap=None, multiopen="shplonk"):
        self.params, self.w, self.blinding = params, witness, blinding
        self.multiopen_name, self.multiopen_prover = multiopen, MO.multiopen_classes(multiopen)[0]
        self.cs, self.qc = witness.cs, E.quotient_columns(witness.cs)
        self.k, self.n, self.u = witness.k, 1 << witness.k, (1 << witness.k) - (BLIND + 1)
        self.dom = EvaluationDomain(4, self.k)
        self.batched = self.k <= 17 if batched is None else batched      # small MSMs are latency-bound one at a time: all columns of a phase in one launch set
        self.lap = lap or (lambda name: None)
        # the current stream and one high-priority stream: streams of different priority never share a hardware queue (two streams of one
        # priority may, and then run one after the other)
        self.streams = [torch.cuda.current_stream(), side_stream()]
        self.commitments = {}                                            # (kind, index) -> Jacobian point on the device
        self.random_poly = None

    # -- commitments
    def commit(self, lagrange, ptr):                                     # params.commit / commit_lagrange of 2^k device-resident values
        out = torch.zeros(12, dtype=torch.int64, device=DEV)
        self.params.commit_device(ptr, self.n, out.data_ptr(), lagrange=lagrange)
        return out

    def commit_all(self, lagrange, cols):
        """independent commits alternate between two streams: one MSM's latency-bound reduction tail runs under the next one's accumulation
        (tools/two_stream_msm.py: 5.31 -> 4.96 ms per 2^22 MSM); each stream has its own scratch set inside the library.
        batched (small k): the columns are gathered into one array and committed by one call"""
        n = self.n
        if self.batched and len(cols) > 1:
            stack = torch.stack(list(cols)).contiguous()
            outs_b = torch.zeros((len(cols), 12), dtype=torch.int64, device=DEV)
            self.params.commit_many_device(stack.data_ptr(), n, len(cols), n, outs_b.data_ptr(), lagrange=lagrange)
            return [outs_b[i] for i in range(len(cols))]
        outs = [torch.zeros(12, dtype=torch.int64, device=DEV) for _ in cols]
        cur = torch.cuda.current_stream()
        self.streams[1].wait_stream(cur)
        for i, col in enumerate(cols):
            self.params.commit_device(col.data_ptr(), n, outs[i].data_ptr(), lagrange=lagrange, stream=self.streams[i % 2].cuda_stream)
        cur.wait_stream(self.streams[1])
        return outs

    def commit_ptr(self, ptr):                                           # what the multi-open provers commit their quotients with
        return self.commit(False, ptr).cpu().numpy().view(np.uint64)

    def _committed(self, kinds, points):
        self.commitments.update(zip(kinds, points))
        return points

    def commit_advice(self):                                             # advice is committed in the Lagrange basis
        self.adv_commit = self._committed([("advice", i) for i in range(len(self.w.advice))], self.commit_all(True, self.w.advice))
        self.lap("commit_advice")

    # -- the order of steps
    def prove(self, dpk, challenges, lookups_one_call=True, sharded_quotient=False, sharded_key=False):
        NL, with_transcript = self.w.lookups, challenges.transcript is not None
        check_options(with_transcript, NL, lookups_one_call, sharded_quotient, sharded_key)
        if not with_transcript and self.multiopen_prover is not MO.ProverSHPLONK:      # SeededChallenges draws SHPLONK's y, v, u
            raise ValueError("multiopen=\"gwc\" writes its witnesses to a transcript: the seeded flow opens with SHPLONK")
        self.dpk, self.ch, self.sharded_quotient, self.sharded_key = dpk, challenges, sharded_quotient, sharded_key
        # a single lookup over 2^20 rows or more stays with the loop
        self.one_call = bool(lookups_one_call and NL and (with_transcript or not (NL == 1 and self.k >= 20)))
        self.lookup_cols, self.lookup_closes = [], True
        if not self.commitments:
            self.commit_advice()
        (self._transcript if with_transcript else self._seeded)()
        return self

    def _seeded(self):
        """permutation products first, then the lookups, then ONE commit of all the products' coefficients"""
        ch, qc = self.ch, self.qc
        self.theta, (self.beta, self.gamma), self.y = ch.theta(), ch.beta_gamma(), ch.y()
        self.load_sigma()
        self.permutation_products()
        if self.one_call:
            self.lookup_permute()
            self.lookup_products()
        else:
            self.lookup_one_at_a_time()
        self.lap("lookup_permute_and_product")
        self.random_polynomial()
        self.to_coefficients()
        commits = self.commit_all(False, [self.coeff[i] for i in range(qc.perm_product, qc.total)] + [self.coeff[qc.advice]])
        self.a0_coeff_commit = commits.pop()
        self._committed(self.product_kinds(), commits)
        self.lap("commit_products")
        self.quotient_pieces()
        self.x = ch.x()
        self.plan = opening_plan(self.cs, self.w.gate_cols, self.w.lookups, self.u, False, "seeded")      # the seeded flow has never opened the random polynomial
        self.evaluate_at_x()
        self.multiopen()

    def _transcript(self):
        """halo2 `create_proof`'s order: vk repr; advice commitments, theta; the lookups' permuted commitments, beta,
        gamma; permutation then lookup product commitments (Lagrange basis: the same group elements as the commitments to their coefficients), the
        random polynomial's commitment, y; the quotient pieces, x; the evaluations; the multi-open"""
        ch, lap, NL = self.ch, self.lap, self.w.lookups
        ch.instances(self.w.instance_values)            # between the key and the advice commitments; nothing for a circuit without instance columns
        self.theta = ch.theta(self.adv_commit)
        lap("transcript")
        self.load_sigma()
        if NL:
            self.lookup_permute()
            lap("lookup_permute_and_product")
            permuted = self._committed([(kind, j) for j in range(NL) for kind in ("lookup_pa", "lookup_ps")],
                                       self.commit_all(True, [c_ for j in range(NL) for c_ in (self.pa_all[j], self.ps_all[j])]))
            lap("commit_products")
            self.beta, self.gamma = ch.beta_gamma(permuted)
            lap("transcript")
            self.permutation_products()                 # only now can the products be formed
            self.lookup_products()
            lap("lookup_permute_and_product")
        else:                                           # no lookups: beta and gamma follow theta at once
            lap("lookup_permute_and_product")
            self.beta, self.gamma = ch.beta_gamma()
            self.permutation_products()
        self.random_polynomial()
        kinds = [kind for kind in self.product_kinds() if kind[0] in ("perm", "lookup_z")]
        products = self._committed(kinds, self.commit_all(True, self.z_sets + [self.lookup_cols[3 * j] for j in range(NL)]))
        lap("commit_products")
        self.y = ch.y(products + ([self.commitments[("random", 0)]] if self.random_poly is not None else []))
        lap("transcript")
        self.to_coefficients()
        self.a0_coeff_commit = self.commit(False, self.coeff[self.qc.advice].data_ptr())
        lap("commit_products")
        self.quotient_pieces()
        self.x = ch.x(self.h_commit)
        lap("transcript")
        self.plan = opening_plan(self.cs, self.w.gate_cols, NL, self.u, self.random_poly is not None, "halo2")
        self.evaluate_plan()
        lap("transcript")
        self.multiopen()
        lap("transcript")

    def quotient_pieces(self):
        self.extend()
        self.quotient()
        self.commit_h()

    # -- the phases
    def load_sigma(self):                                                # working copies of the key's permutation columns
        self.sigma = [empty(self.n) for _ in self.cs.permutation_columns]
        for i, sg in enumerate(self.sigma):
            KG._copy_device(sg.data_ptr(), self.dpk.permutation_values(i), self.k)

    def permutation_products(self):
        """every set's product column in ONE call (zkhip_permutation_products_device: the sets are chained on the device through z[u]); one
        read-back of the last set's z[u] says whether the argument closes"""
        cs, n, u, k = self.cs, self.n, self.u, self.k
        sets, npc = cs.num_permutation_sets, len(cs.permutation_columns)
        self.z_all = empty(sets, n)
        vptr = (C.c_void_p * npc)(*[self.w.permutation_column(c).data_ptr() for c in range(npc)])
        sptr = (C.c_void_p * npc)(*[sg.data_ptr() for sg in self.sigma])
        consts = [F.fr_encode([v_])[0] for v_ in (self.beta, self.gamma, E.DELTA, F.omega_for(k))]
        _lib.check(_lib.load().zkhip_permutation_products_device(vptr, sptr, npc, cs.chunk_len, k, u, *[c_.ctypes.data for c_ in consts], self.z_all.data_ptr(), None))
        self.z_sets = [self.z_all[si] for si in range(sets)]
        self.permutation_closes = T.fr_ints(self.z_all[sets - 1, u:u + 1])[0] == 1
        for z in self.z_sets:
            self.blinding.made(z, u + 1)
        self.blinding.step(self.z_sets, u + 1)
        self.lap("permutation_products")

    def lookup_permute(self):
        """every lookup's permuted input and table in one call; the blinding rows are drawn first, per lookup pa, ps and the product's tail"""
        NL, n, u, b = self.w.lookups, self.n, self.u, self.blinding
        self.pa_all, self.ps_all, self.lookup_tails = empty(NL, n), empty(NL, n), []
        for j in range(NL):
            b.column(n, self.pa_all[j]), b.column(n, self.ps_all[j])
            self.lookup_tails.append(b.ahead(n - u - 1))
        b.step([self.pa_all[j] for j in range(NL)] + [self.ps_all[j] for j in range(NL)], u)
        E.permute_expression_pairs_device(self.w.lookup_inputs, [self.w.table] * NL, u, self.k, self.pa_all, self.ps_all)

    def lookup_products(self):
        """every lookup's product column in one call"""
        NL, u = self.w.lookups, self.u
        z_lk = E.lookup_products_device(self.w.lookup_inputs, [self.w.table] * NL, self.pa_all, self.ps_all, u, self.k, self.beta, self.gamma)
        self.lookup_closes = all(v_ == 1 for v_ in T.fr_ints(z_lk[:, u]))
        for j, tail in enumerate(self.lookup_tails):
            if tail is not None:
                z_lk[j, u + 1:] = tail
        self.blinding.step([z_lk[j] for j in range(NL)], u + 1)
        self.lookup_cols = [c_ for j in range(NL) for c_ in (z_lk[j], self.pa_all[j], self.ps_all[j])]

    def lookup_one_at_a_time(self):
        """the single-lookup call, two row programs and a grand product per lookup"""
        lib, n, u, k, b, table = _lib.load(), self.n, self.u, self.k, self.blinding, self.w.table
        pn, pd = E.lookup_product_programs(1, 1, self.beta, self.gamma, self.theta)
        for lk in self.w.lookup_inputs:
            pa, ps = b.column(n), b.column(n)
            b.step([pa, ps], u)
            _lib.check(lib.zkhip_lookup_permute_device(lk.data_ptr(), table.data_ptr(), u, pa.data_ptr(), ps.data_ptr(), None))
            zl = run_prog(pn, [lk, table], k)
            den = run_prog(pd, [pa, ps], k)
            _lib.check(lib.zkhip_fr_grand_product_device(zl.data_ptr(), den.data_ptr(), n, zl.data_ptr(), None))
            self.lookup_closes = self.lookup_closes and T.fr_ints(zl[u])[0] == 1
            b.made(zl, u + 1)
            b.step([zl], u + 1)
            self.lookup_cols += [zl, pa, ps]

    def random_polynomial(self):
        """the vanishing argument's random polynomial, where the blinding source has one: drawn in the coefficient basis and committed"""
        if self.blinding.random_polynomial is not None:
            self.random_poly = self.blinding.random_polynomial(self.n)
            self._committed([("random", 0)], [self.commit(False, self.random_poly.data_ptr())])
            self.lap("vanishing_random_poly")

    def product_kinds(self):                                             # the prover's own polynomials in the order of their columns
        return [("perm", si) for si in range(self.cs.num_permutation_sets)] + [(kind, j) for j in range(self.w.lookups) for kind in ("lookup_z", "lookup_pa", "lookup_ps")]

    def to_coefficients(self):
        """Lagrange -> coefficients.  Columns of the proving key (fixed, l_0 / l_last / l_active, the permutation's sigma polynomials) are
        transformed once per circuit by keygen and their extended cosets are kept (pk.fixed_cosets, pk.permutation.cosets [DEP]); only the
        witness-dependent columns (advice, the permutation / lookup products, the permuted lookup pair) are transformed per proof.  The laps named
        "keygen_*" are not part of the proof."""
        lib, cs, qc, dpk, dom, n, u, k, w = _lib.load(), self.cs, self.qc, self.dpk, self.dom, self.n, self.u, self.k, self.w
        ONE = words([1])[0]
        l0 = torch.zeros((n, 4), dtype=torch.int64, device=DEV); l0[0] = ONE
        l_last = torch.zeros((n, 4), dtype=torch.int64, device=DEV); l_last[u] = ONE
        rows = torch.arange(n, dtype=torch.int64, device=DEV)
        l_active = torch.where((rows < u)[:, None], ONE[None, :], torch.zeros_like(ONE)[None, :]).contiguous()
        # the instance columns sit between the advice and l_0: transformed per proof with the advice, never committed, never opened
        lagrange = w.fixed + w.advice + w.instance + [l0, l_last, l_active] + self.sigma + self.z_sets + self.lookup_cols
        assert len(lagrange) == qc.total
        self.coeff = coeff = torch.stack(lagrange).contiguous()                     # [ncol][n][4]
        npc = len(cs.permutation_columns)
        key_polys = [dpk.fixed_poly(i) for i in range(cs.num_fixed)] + [None] * (qc.sigma - qc.advice) + [dpk.permutation_poly(i) for i in range(npc)]
        self.lap("stack_columns")
        self.key_ranges = [(qc.fixed, qc.advice), (qc.l0, qc.perm_product)]
        self.proof_ranges = [(qc.advice, qc.l0), (qc.perm_product, qc.total)]

        def ifft_range(lo, hi):
            if hi > lo:
                _lib.check(lib.zkhip_ifft_scaled_batch_device(coeff[lo].data_ptr(), dom.omega_inv.ctypes.data, k, dom.ifft_divisor.ctypes.data, hi - lo, n, None))

        for lo, hi in self.key_ranges:           # l0 / l_last / l_active_row have no stored coefficient form in the key: transformed here, outside the proof time
            for i in range(lo, hi):
                if key_polys[i] is not None:
                    KG._copy_device(coeff[i].data_ptr(), key_polys[i], k)
                else:
                    ifft_range(i, i + 1)
        self.lap("keygen_lagrange_to_coeff")
        for lo, hi in self.proof_ranges:
            ifft_range(lo, hi)
        self.lap("lagrange_to_coeff")

    def extend(self):
        """coefficients -> extended coset: the key's cosets are copied (or, with a sharded key, read where they lie), the proof's columns are
        transformed -- inside the sharded quotient's call where that is used"""
        lib, cs, qc, dpk, dom, n, k = _lib.load(), self.cs, self.qc, self.dpk, self.dom, self.n, self.k
        ek, en, ncol = dom.extended_k, dom.extended_len(), qc.total
        self.key_cosets = ([dpk.fixed_coset(i) for i in range(cs.num_fixed)] + [None] * (qc.l0 - qc.advice) + [dpk.l0(), dpk.l_last(), dpk.l_active_row()]
                           + [dpk.permutation_coset(i) for i in range(len(cs.permutation_columns))])
        self.ext = empty(ncol, en)
        for lo, hi in self.key_ranges:
            for i in range(lo, hi):
                if not self.sharded_key:
                    KG._copy_device(self.ext[i].data_ptr(), self.key_cosets[i], ek)
        self.lap("keygen_coeff_to_extended")
        if self.sharded_quotient and ncol > 96 and ek < 18:
            raise ValueError("sharded_quotient: the sum-of-programs quotient of the wide circuits is not sharded")
        for lo, hi in self.proof_ranges if not self.sharded_quotient else ():
            if hi > lo:
                _lib.check(lib.zkhip_coeff_to_extended_device(self.coeff[lo].data_ptr(), n, k, self.ext[lo].data_ptr(), en, ek, hi - lo, dom.extended_omega.ctypes.data,
                                                              dom.g_coset.ctypes.data, None))
        self.lap("coeff_to_extended")

    def quotient(self):
        """the quotient numerator over the extended coset, divided by X^n - 1, back to coefficients"""
        lib, dom, k, coeff, ext = _lib.load(), self.dom, self.k, self.coeff, self.ext
        ek, en, ncol = dom.extended_k, dom.extended_len(), self.qc.total
        challenges = (self.beta, self.gamma, self.theta, self.y)
        h_ext = empty(en)
        if ncol > 96 and ek < 18 and not self.sharded_quotient:
            # hundreds of columns over a few thousand rows: as one program a handful of wavefronts walk thousands of instructions; as a sum of
            # programs over runs of the y-fold's terms (evaluate_h_parts + zkhip_fr_eval_rows_sum_device) they run side by side in one launch
            progs, weights = E.evaluate_h_parts(self.cs, k, ek, *challenges, 16)
            E.run_programs_sum_device(progs, weights, [ext[i].data_ptr() for i in range(ncol)], ek, h_ext.data_ptr())
        else:
            progs = [E.evaluate_h_program(self.cs, k, ek, *challenges)]
            if self.sharded_quotient:
                # rows cut over the devices of zkhip_init; the key's cosets EXTENDED (or a row-shard set), the proof's columns COEFF
                key = {i for lo, hi in self.key_ranges for i in range(lo, hi)}
                key_form = (lambda i: (self.key_cosets[i], E.COL_ROW_SHARDS)) if self.sharded_key else (lambda i: (ext[i].data_ptr(), E.COL_EXTENDED))
                E.evaluate_rows_sharded_device(progs[0], [key_form(i) if i in key else (coeff[i].data_ptr(), E.COL_COEFF) for i in range(ncol)],
                                               k, ek, dom, h_ext.data_ptr())
            else:
                run_prog(progs[0], [ext[i] for i in range(ncol)], ek, out=h_ext)
        self.program_insns, self.program_registers = sum(len(p_.insns) for p_ in progs), max(p_.registers_used() for p_ in progs)
        tinv = torch.from_numpy(dom.t_evaluations.view(np.int64)).to(DEV)
        _lib.check(lib.zkhip_mul_periodic_device(h_ext.data_ptr(), en, tinv.data_ptr(), tinv.shape[0], None))
        self.lap("evaluate_h")
        self.h_coeff = empty(en)
        _lib.check(lib.zkhip_extended_to_coeff_device(h_ext.data_ptr(), en, ek, dom.extended_omega_inv.ctypes.data, dom.extended_ifft_divisor.ctypes.data,
                                                      dom.g_coset.ctypes.data, self.h_coeff.data_ptr(), en, en, 1, None))
        self.lap("extended_to_coeff")

    def commit_h(self):
        kinds = [("h", i) for i in range(3)]
        self.h_commit = self._committed(kinds, self.commit_all(False, [self.h_coeff[i * self.n:(i + 1) * self.n] for i in range(3)]))
        self.lap("commit_h")

    def polynomials(self):
        """the (kind, index) of every column and quotient piece (None: not a polynomial of the proof) and the device addresses of their
        coefficients, in the order of `evals`: the one map a plan becomes queries through"""
        qc, cs, n = self.qc, self.cs, self.n
        kinds = ([("fixed", i) for i in range(cs.num_fixed)] + [("advice", i) for i in range(cs.num_advice)] + [None] * (cs.num_instance + 3)
                 + [("sigma", i) for i in range(len(cs.permutation_columns))] + self.product_kinds() + [("h", i) for i in range(3)])
        return kinds, [self.coeff[i].data_ptr() for i in range(qc.total)] + [self.h_coeff[i * n:].data_ptr() for i in range(3)]

    def _queries(self):
        w_, polys = F.omega_for(self.k), dict(zip(*self.polynomials()))
        if self.random_poly is not None:
            polys[("random", 0)] = self.random_poly.data_ptr()
        self.queries = [MO.ProverQuery(self.x * pow(w_, r, R) % R, polys[(kind, idx)]) for kind, idx, r in self.plan]

    def evaluate_at_x(self):
        """every column and quotient piece at x in one batched call (the verifier's side reads them from `evals`); the rotated openings are
        left to the multi-open"""
        ptrs = self.polynomials()[1]
        self.evals = torch.zeros((len(ptrs), 4), dtype=torch.int64, device=DEV)
        _lib.check(_lib.load().zkhip_fr_eval_polynomial_batch_device((C.c_void_p * len(ptrs))(*ptrs), len(ptrs), self.n, F.fr_encode([self.x])[0].ctypes.data,
                                                                    self.evals.data_ptr(), None))
        self.lap("evaluations")
        self._queries()

    def evaluate_plan(self):
        """every opened (polynomial, rotation): one batched evaluation per rotation into one device buffer, put into the plan's order there, and
        written to the transcript from there"""
        self._queries()
        queries, w_ = self.queries, F.omega_for(self.k)
        by_rot = {}
        for qi, (_, _, r) in enumerate(self.plan):
            by_rot.setdefault(r, []).append(qi)
        grouped = torch.zeros((len(queries), 4), dtype=torch.int64, device=DEV)
        where, off = [0] * len(queries), 0
        for r, qis in by_rot.items():
            ptrs_r = (C.c_void_p * len(qis))(*[queries[qi].poly for qi in qis])
            point = F.fr_encode([self.x * pow(w_, r, R) % R])[0]
            _lib.check(_lib.load().zkhip_fr_eval_polynomial_batch_device(ptrs_r, len(qis), self.n, point.ctypes.data, grouped[off:].data_ptr(), None))
            for t_, qi in enumerate(qis):
                where[qi] = off + t_
            off += len(qis)
        evals_plan = grouped[torch.tensor(where, dtype=torch.int64, device=DEV)].contiguous()
        self.lap("evaluations")
        self.ch.write_scalars(evals_plan)
        for q_, e_ in zip(queries, T.fr_ints(evals_plan)):
            q_.eval = e_                                        # the multi-open's R_ij need them as integers

    def multiopen(self):
        """SHPLONK (the benches' `gen_proof` path; `gen_snark` opens with GWC: multiopen="gwc") over the plan's queries; with a transcript the
        proof bytes are complete after it"""
        self.multiopen_ok, self.multiopen_proof = True, None
        mo_prover = self.multiopen_prover(self.k, self.commit_ptr)
        try:
            self.multiopen_proof = self.ch.multiopen(mo_prover, self.queries)
        except ArithmeticError:
            self.multiopen_ok = False
        self.lap("multiopen_" + self.multiopen_name)
        mo_prover.close()
        self.proof = self.ch.finish()

    # -- the verifier's side of a seeded proof
    def verifier_queries(self):
        """what a verifier holds of a seeded proof: the commitments (advice, products, quotient pieces, the verifying key's fixed and sigma
        commitments) and the evaluations (`evals` at x, the rotated openings from the multi-open), as VerifierQuerys in the plan's order"""
        com = {kind: c_.cpu().numpy().view(np.uint64).reshape(12).copy() for kind, c_ in self.commitments.items()}
        com.update(key_commitments(self.dpk.vk))
        slot = {kind: i for i, kind in enumerate(self.polynomials()[0])}
        at_x = T.fr_ints(self.evals)
        evals = [at_x[slot[(kind, idx)]] if r == 0 else q.eval for (kind, idx, r), q in zip(self.plan, self.queries)]
        return verifier_queries(self.plan, com, evals, self.x, self.k)


def create_proof(params, dpk, witness, challenges, blinding, batched=None, lap=None, multiopen="shplonk", **how):
    """one proof, start to end, with no synchronisation added for timing when `lap` is None; `how`: lookups_one_call, sharded_quotient, sharded_key (Prover.prove).  Returns the Prover."""
    return Prover(params, witness, blinding, batched, lap, multiopen).prove(dpk, challenges, **how)

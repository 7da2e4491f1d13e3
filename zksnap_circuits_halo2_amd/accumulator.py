"""KZG accumulators: the value the reference's IVC carries from round to round (`RecursionCircuit::new`, aggregator/src/wrapper.rs).

An accumulator is a pair of G1 points (lhs, rhs) with e(lhs, g2) = e(rhs, [s]g2), here an int64 device tensor (..., 2, 8) of affine Montgomery
limbs.  lhs is the A point of the batch verifier's rows (multiopen.fold_check), rhs the C point; for GWC rhs = sum_i u^i W_i.
  succinct_verify_proofs   `PlonkSuccinctVerifier::verify` over a batch: everything of a verifier but the pairing -- each proof's accumulator
                           as a value, from the device rows of scalars through zkhip_g1_row_msm_device (B small MSMs in one launch set)
  accumulate               `KzgAs::create_proof` without blinding: the accumulators absorbed into a fresh transcript, r squeezed,
                           (sum r^i lhs_i, sum r^i rhs_i)
  to_limbs / from_limbs    an accumulator as 12 public inputs (3 limbs of 88 bits per coordinate, csrc/kzg_limbs.hpp) and back
  decide / decide_all      the pairing check, of one accumulator or of a random combination of many
Not built: blinded `KzgAs`, the in-circuit side, a batch sharded over devices.  Still unpinned against snark-verifier (not vendored): the order
new-then-old of the accumulators a round folds, Gwc19's set order against ours, the strictness of `fe_from_limbs`."""
import contextlib
import io
import os

import numpy as np
import torch

from . import _lib, fields as F, keygen as KG, multiopen as MO, verifier as V
from .tensors import stream_of
from .transcript import decoded, transcript_classes, vk_transcript_repr

R = F.R_MOD
Q = MO._Q_MOD
LIMBS, LIMB_BITS = 3, 88
DEV = V.DEV


def _device_tensor(name, t, shape):
    if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int64) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} is a contiguous int64 device tensor of shape {tuple(shape)}")


def row_msm_device(rows, own_points, shared_points, n_own=None, stream=None, out=None):
    """zkhip_g1_row_msm_device: rows (B, n_cols, 4) scalars; own_points (B, m, 8) affine or None, of which row i uses its first n_own (default:
    all m; a smaller n_own reads the head of every row of a wider array, stride m); shared_points (n_cols - n_own, 8) or None -> (B, 12) Jacobian
    points, out[i] = sum_j rows[i][j] * (own[i][j] if j < n_own else shared[j - n_own]).  Asynchronous on `stream`."""
    B, n_cols = rows.shape[0], rows.shape[1]
    m = 0 if own_points is None else own_points.shape[1]
    n_own = m if n_own is None else int(n_own)
    t = 0 if shared_points is None else shared_points.shape[0]
    if not 0 <= n_own <= m or n_own + t != n_cols:
        raise ValueError(f"row_msm_device: {n_cols} columns over {n_own} of {m} own points and {t} shared points")
    _device_tensor("row_msm_device: rows", rows, (B, n_cols, 4))
    if own_points is not None:
        _device_tensor("row_msm_device: own_points", own_points, (B, m, 8))
    if shared_points is not None:
        _device_tensor("row_msm_device: shared_points", shared_points, (t, 8))
    if out is None:
        out = torch.empty((B, 12), dtype=torch.int64, device=rows.device)
    _device_tensor("row_msm_device: out", out, (B, 12))
    _lib.check(_lib.load().zkhip_g1_row_msm_device(rows.data_ptr() if B else None, n_cols, own_points.data_ptr() if B and n_own else None, n_own, max(m, n_own),
                                                   shared_points.data_ptr() if t else None, B, out.data_ptr() if B else None, stream_of(stream)))
    return out


# ---- limbs -----------------------------------------------------------------------------------------------------------------------------------
def fe_to_limbs(x: int):
    """`fe_to_limbs::<_, _, 3, 88>`: the canonical integer of a coordinate cut little-endian into three 88-bit limbs"""
    if not 0 <= x < Q:
        raise ValueError("fe_to_limbs: a canonical coordinate, 0 <= x < q")
    return [(x >> (LIMB_BITS * i)) & ((1 << LIMB_BITS) - 1) for i in range(LIMBS)]


def fe_from_limbs(limbs) -> int:
    """the coordinate of three limbs, strictly: ValueError for a limb of 2^88 or more and for a value of q or more"""
    limbs = [int(v) for v in limbs]
    if len(limbs) != LIMBS or any(not 0 <= v < (1 << LIMB_BITS) for v in limbs):
        raise ValueError("fe_from_limbs: three limbs below 2^88")
    x = sum(v << (LIMB_BITS * i) for i, v in enumerate(limbs))
    if x >= Q:
        raise ValueError("fe_from_limbs: the value is not below q")
    return x


def to_limbs(acc, stream=None):
    """zkhip_kzg_limbs_encode_device: points (..., 8) -> (..., 6, 4) Fr words; so an accumulator (..., 2, 8) gives (..., 2, 6, 4), and
    `.reshape(..., 12, 4)` is lhs.x, lhs.y, rhs.x, rhs.y as the wrapper's public inputs hold them"""
    _device_tensor("to_limbs: the points", acc, acc.shape[:-1] + (8,))
    n = acc.numel() // 8
    out = torch.empty(acc.shape[:-1] + (2 * LIMBS, 4), dtype=torch.int64, device=acc.device)
    _lib.check(_lib.load().zkhip_kzg_limbs_encode_device(acc.data_ptr() if n else None, n, out.data_ptr() if n else None, stream_of(stream)))
    return out


def from_limbs(limbs, stream=None):
    """zkhip_kzg_limbs_decode_device: (..., 6, 4) Fr words -> (points (..., 8), status (...) int32): 0 accepted, 1 a limb >= 2^88, 2 a coordinate
    >= q, 3 not on the curve ((0, 0) included); a refused point is (0, 0)"""
    _device_tensor("from_limbs: the limbs", limbs, limbs.shape[:-2] + (2 * LIMBS, 4))
    n = limbs.numel() // (8 * LIMBS)
    points = torch.empty(limbs.shape[:-2] + (8,), dtype=torch.int64, device=limbs.device)
    status = torch.empty(limbs.shape[:-2], dtype=torch.int32, device=limbs.device)
    _lib.check(_lib.load().zkhip_kzg_limbs_decode_device(limbs.data_ptr() if n else None, n, points.data_ptr() if n else None, status.data_ptr() if n else None,
                                                         stream_of(stream)))
    return points, status


def default_accumulator(params):
    """(g[1], g[0]) = ([s]G, G): the accumulator the reference's round 0 carries"""
    return torch.from_numpy(np.stack([np.asarray(params.g[1], dtype=np.uint64).reshape(8), np.asarray(params.g[0], dtype=np.uint64).reshape(8)]).view(np.int64)).to(DEV)


# ---- the succinct verifier -------------------------------------------------------------------------------------------------------------------
class SuccinctResult:
    """status: (B,) int32 on the host -- 0 accepted, 1 the identity refused, 2 the bytes do not decode (or its evaluations contradict each
    other), 3 a carried accumulator is malformed; accumulators: (B, 1 + len(accumulator_indices), 2, 8) on the device, the proof's new
    accumulator first, the carried ones behind it; a proof with status 1 or 2 has zeros, a malformed carried accumulator is zeros"""

    def __init__(self, status, accumulators):
        self.status, self.accumulators = status, accumulators


def _normalize_device(xyz, out):
    """zkhip_g1_batch_normalize_device over every Jacobian point of `xyz` (..., 12) into `out` (..., 8)"""
    _lib.check(_lib.load().zkhip_g1_batch_normalize_device(xyz.data_ptr(), xyz.numel() // 12, out.data_ptr(), None))


def _fallback_points(scheme, params, queries, reader, part, n_points):
    """a proof's two points by the scheme's host path (Python-integer scalars): `part` is what the device path has read of the multi-open's
    part, None reads it from `reader`.  -> (lhs, rhs) affine limbs, or None: the part does not decode or the queries are inconsistent"""
    if part is None:
        part = decoded(scheme(params).read_proof, reader, n_points, device=False)
        if part is None:
            return None
    return scheme(params).accumulator_points_read(queries, *part)


def carried_accumulators(instances, accumulator_indices, proofs):
    """the accumulators a batch of proofs carries in its public inputs: for every (column, lo) of `accumulator_indices` the 12 limbs
    instances[i][column][lo : lo + 12] decoded -> (accumulators (B, n, 2, 8), status (B, n, 2) int32) on the device"""
    indices = [(int(c), int(lo)) for c, lo in accumulator_indices]
    if not indices or proofs == 0:
        return torch.zeros((proofs, len(indices), 2, 8), dtype=torch.int64, device=DEV), torch.zeros((proofs, len(indices), 2), dtype=torch.int32, device=DEV)
    if instances is None or len(instances) != proofs:
        raise ValueError("accumulator_indices: the proofs' public inputs (instances=) hold the carried accumulators")
    flat = []
    for per_proof in instances:
        for c, lo in indices:
            if c >= len(per_proof) or lo < 0 or lo + 4 * LIMBS > len(per_proof[c]):
                raise ValueError(f"accumulator_indices: instance column {c} has no 12 values from {lo}")
            flat += [int(v) % R for v in per_proof[c][lo:lo + 4 * LIMBS]]
    limbs = V.words(flat).reshape(proofs, len(indices), 2, 2 * LIMBS, 4)
    return from_limbs(limbs)


def succinct_verify_proofs(params, vk, k, proofs, shape, plan, hash="poseidon", multiopen="gwc", instances=None, accumulator_indices=()):
    """`PlonkSuccinctVerifier::verify` over a batch of proofs of one circuit: verifier.verify_transcript_proofs(fold=True) up to the rows -- the
    heads read, the identity of the whole batch in one call, the scheme's rows of scalars on the device --, then each proof's two points as
    values: two row_msm_device calls (A over [own | shared], C over the first c own points through the stride) and one
    zkhip_g1_batch_normalize_device.  No pairing is taken: `decide` does that.  A proof without a device row (x = 0 mod r, a SHPLONK status 1,
    a plan that is not foldable) gets its points from the scheme's host path.  accumulator_indices: (column, lo) pairs, the 12 limbs of an
    accumulator the proof carries in its public inputs (`with_accumulator_indices`).  -> SuccinctResult."""
    scheme = MO.multiopen_classes(multiopen)[1]
    reader = transcript_classes(hash)[1]
    V.identity_program_of(vk, plan, k)
    n_instance = vk.cs.num_instance
    if n_instance and instances is None:
        raise ValueError("succinct_verify_proofs: the key's circuit has instance columns: hand in the public inputs of every proof (instances=)")
    if n_instance:
        V._check_instances(vk.cs, k, instances, len(proofs))
    B, n_carried = len(proofs), len(tuple(accumulator_indices))
    status = np.full(B, 2, dtype=np.int32)
    accs = torch.zeros((B, 1 + n_carried, 2, 8), dtype=torch.int64, device=DEV)
    if B == 0:
        return SuccinctResult(status, accs)
    vk_io = io.BytesIO()
    vk.write(vk_io, KG.RAW_BYTES)
    vk_repr = vk_transcript_repr(vk_io.getvalue())
    fold_plan = V._kept_on(vk, "fold_plans", (scheme, tuple(plan)), lambda: scheme.fold_plan(plan))
    on_device = fold_plan.foldable(k)
    points, key_com = V.key_points(vk), {}
    with contextlib.ExitStack() as stack:
        heads = {}
        for i, proof in enumerate(proofs):
            r = stack.enter_context(reader(bytes(proof)))
            head = decoded(V._read_proof_head, r, vk_repr, shape, plan, instances[i] if n_instance else (), on_device=on_device)
            if head is not None:
                heads[i] = (r,) + head
        order = sorted(heads)
        if not order:
            return SuccinctResult(status, accs)
        d_evals = V.words([e_ for i in order for e_ in heads[i][3]]).reshape(len(order), len(plan), 4)
        identity = V.identity_statuses(vk, k, plan, [heads[i][3] for i in order], [heads[i][2] for i in order], [instances[i] for i in order] if n_instance else None,
                                       d_evals=d_evals)
        rows_of = {i: row for row, i in enumerate(order)}
        for i, s_ in zip(order, identity):
            status[i] = 0 if s_ == 0 else 1
        order = [i for i in order if status[i] == 0]

        def host_path(i, part=None):
            r, com, challenges, evals = heads[i]
            host = dict(zip(com, MO._points_xyz(com.values()))) if on_device else com
            if not key_com:
                key_com.update(zip(points, MO._points_xyz(points.values())))
            queries = V.verifier_queries(plan, {**host, **key_com}, evals, challenges[4], k)
            pair = _fallback_points(scheme, params, queries, r, part, len(MO.construct_intermediate_sets(queries)))
            if pair is None:
                status[i] = 2
            else:
                accs[i, 0] = torch.from_numpy(np.stack(pair).view(np.int64)).to(DEV)

        rowed, parts = [], []
        for i in order:
            if not on_device or heads[i][2][4] % R == 0:
                host_path(i)
                continue
            part = decoded(scheme(params).read_proof, heads[i][0], len(fold_plan.rotations), device=True)
            if part is None:
                status[i] = 2
            else:
                rowed.append(i)
                parts.append(part)
        if rowed:
            shared = np.stack([np.asarray(points[key_], dtype=np.uint64).reshape(8) for key_ in fold_plan.shared_keys] + [np.asarray(params.g[0], dtype=np.uint64).reshape(8)])
            d_shared = torch.from_numpy(shared.view(np.int64)).to(DEV)
            d_own = torch.stack([torch.stack(mine + [heads[i][1][key_] for key_ in fold_plan.own_keys]) for i, (mine, _) in zip(rowed, parts)]).contiguous()
            index = torch.tensor([rows_of[i] for i in rowed], dtype=torch.int64, device=DEV)
            d_points = V.words([c_ for i, (_, challenges) in zip(rowed, parts) for c_ in (heads[i][2][4],) + challenges]).reshape(len(rowed), -1, 4)
            d_rows_a, d_rows_c, d_status = scheme.fold_scalars(fold_plan, d_evals.index_select(0, index).contiguous(), d_points, k)
            refused = {j for j, s_ in enumerate(d_status.cpu().tolist()) if s_ != 0} if d_status is not None else set()
            for j in sorted(refused):                       # no row exists for such a proof
                host_path(rowed[j], parts[j])
            kept = [j for j in range(len(rowed)) if j not in refused]
            if kept:
                if refused:
                    keep = torch.tensor(kept, dtype=torch.int64, device=DEV)
                    d_own, d_rows_a, d_rows_c = (t_.index_select(0, keep).contiguous() for t_ in (d_own, d_rows_a, d_rows_c))
                n = len(kept)
                sums = torch.empty((2, n, 12), dtype=torch.int64, device=DEV)
                row_msm_device(d_rows_a, d_own, d_shared, out=sums[0])
                row_msm_device(d_rows_c, d_own, None, n_own=d_rows_c.shape[1], out=sums[1])
                pairs = torch.empty((2, n, 8), dtype=torch.int64, device=DEV)
                _normalize_device(sums, pairs)
                accs[torch.tensor([rowed[j] for j in kept], dtype=torch.int64, device=DEV), 0] = pairs.permute(1, 0, 2)
    if n_carried:
        carried, carried_status = carried_accumulators(instances, accumulator_indices, B)
        carried = carried * (carried_status == 0).all(dim=2)[:, :, None, None]       # a malformed accumulator is zeros, both points
        bad = (carried_status.reshape(B, -1) != 0).any(dim=1).cpu().numpy()
        for i in range(B):
            if status[i] == 0:
                accs[i, 1:] = carried[i]
                if bad[i]:
                    status[i] = 3
    return SuccinctResult(status, accs)


# ---- KzgAs ------------------------------------------------------------------------------------------------------------------------------------
def _accumulate(accumulators, tr):
    _device_tensor("accumulate: the accumulators", accumulators, (accumulators.shape[0], 2, 8))
    n = accumulators.shape[0]
    if n == 0:
        raise ValueError("accumulate: no accumulator")
    host = accumulators.cpu().numpy().view(np.uint64).reshape(n, 2, 8)
    if any(not host[i, j].any() for i in range(n) for j in range(2)):
        raise ValueError("accumulate: an accumulator holds the identity, which a transcript refuses")
    if n == 1:
        return accumulators[0], 1
    for i in range(n):
        tr.common_point(host[i, 0])
        tr.common_point(host[i, 1])
    r = tr.squeeze_challenge()
    scalars = V.words([pow(r, i, R) for i in range(n)])
    sums = torch.empty((2, 12), dtype=torch.int64, device=accumulators.device)
    out = torch.empty((2, 8), dtype=torch.int64, device=accumulators.device)
    lib = _lib.load()
    for side in range(2):
        bases = accumulators[:, side, :].contiguous()
        _lib.check(lib.zkhip_msm_g1_device(scalars.data_ptr(), bases.data_ptr(), n, sums[side].data_ptr(), None))
    _lib.check(lib.zkhip_g1_batch_normalize_device(sums.data_ptr(), 2, out.data_ptr(), None))
    return out, r


def accumulate(accumulators, hash="poseidon"):
    """`KzgAs::create_proof` without blinding (the reference's `Default::default()` keys have no zk): accumulators (n, 2, 8) -> (acc (2, 8),
    as_proof, r).  A fresh transcript absorbs lhs_0, rhs_0, lhs_1, ..., squeezes r, and acc = (sum r^i lhs_i, sum r^i rhs_i) by two
    zkhip_msm_g1_device calls and a normalise.  Nothing is written, so as_proof is b"".  n = 1 returns its input (r = 1, nothing absorbed).
    ValueError: an identity point, which the transcript refuses."""
    with transcript_classes(hash)[0]() as tr:
        acc, r = _accumulate(accumulators, tr)
        return acc, tr.finalize(), r


def accumulate_read(accumulators, as_proof, hash="poseidon"):
    """`KzgAs::verify`'s arithmetic: `accumulate` with a reader over `as_proof` -> (acc, r)"""
    with transcript_classes(hash)[1](bytes(as_proof)) as tr:
        return _accumulate(accumulators, tr)


# ---- deciders ---------------------------------------------------------------------------------------------------------------------------------
def _g2_pair(params, device):
    if params.g2 is None or params.s_g2 is None:
        raise ValueError("the decider needs g2 and s_g2")
    return torch.from_numpy(np.stack([np.asarray(params.g2, dtype=np.uint64).reshape(16), np.asarray(params.s_g2, dtype=np.uint64).reshape(16)]).view(np.int64)).to(device)


def decide(params, acc) -> bool:
    """e(lhs, g2) = e(rhs, [s]g2)?  One zkhip_pairing_check_device of the two pairs (lhs, g2), (-rhs, [s]g2).  acc: (2, 8)"""
    _device_tensor("decide: the accumulator", acc, (2, 8))
    host = acc.cpu().numpy().view(np.uint64)
    pair = torch.from_numpy(np.stack([host[0], MO.negate_affine(host[1])]).view(np.int64)).to(acc.device)
    return MO._pairing_verdict(pair, _g2_pair(params, acc.device))


def decide_all(params, accs, seed=None) -> bool:
    """every accumulator of accs (n, 2, 8) at once: multipliers m_i from zkhip_fr_random_device (as fold_check draws them: `seed` is 32 bytes, None
    draws them from os.urandom; a fixed seed is for tests), (sum m_i lhs_i, -sum m_i rhs_i) by two zkhip_msm_g1_device calls, one pairing
    check.  True for n = 0.  A set with a bad accumulator passes with probability about 1 / r."""
    _device_tensor("decide_all: the accumulators", accs, (accs.shape[0], 2, 8))
    n = accs.shape[0]
    if n == 0:
        return True
    g2 = _g2_pair(params, accs.device)
    seed = os.urandom(32) if seed is None else bytes(seed)
    if len(seed) != 32:
        raise ValueError("the seed is 32 bytes")
    lib = _lib.load()
    m = torch.empty((n, 4), dtype=torch.int64, device=accs.device)
    _lib.check(lib.zkhip_fr_random_device(seed, 0, 0, n, m.data_ptr(), None))
    one = V.words([1] * n).reshape(n, 1, 4)
    neg = torch.empty((n, 4), dtype=torch.int64, device=accs.device)
    MO.fold_rows_device(one, 1, m, True, neg, None)      # -m_i
    sums = torch.empty((2, 12), dtype=torch.int64, device=accs.device)
    pair = torch.empty((2, 8), dtype=torch.int64, device=accs.device)
    for side, scalars in enumerate((m, neg)):
        bases = accs[:, side, :].contiguous()
        _lib.check(lib.zkhip_msm_g1_device(scalars.data_ptr(), bases.data_ptr(), n, sums[side].data_ptr(), None))
    _lib.check(lib.zkhip_g1_batch_normalize_device(sums.data_ptr(), 2, pair.data_ptr(), None))
    return MO._pairing_verdict(pair, g2)

#!/usr/bin/env python3
"""KZG accumulators, timed on one MI355X: one process, the sides of every comparison alternating, wall ms, min / median / max; every timed
region ends in a device synchronise.

  the row MSM against the loop: zkhip_g1_row_msm_device for the A side and the C side of a batch (two calls) against the composition the
      library offered before it, a loop of 2 B zkhip_msm_g1_device calls over the same rows (the A side's bases [own_i | shared] laid out per row
      beforehand, outside the timed region).  Shapes: the wrapper's (33 columns, 20 own) and the voter's (954 columns, 430 own), c = 4 C-side
      columns; B = 1, 3, 64 and, for the wrapper's shape, 4096.  Random canonical scalars, points from zkhip_g1_gen_walk_device.  The two
      sides' results are compared (normalised, exact) before anything is timed
  end to end at the wrapper's opening plan (4 gate columns, 1 lookup: 33 columns), at k = 13 so that the proof is made quickly -- the verifier's
      work does not depend on k --, GWC under Poseidon, one proof's bytes repeated B times (B = 3, 64): accumulator.succinct_verify_proofs,
      accumulate of the B accumulators, decide of the result, decide_all of the B; beside them verifier.verify_transcript_proofs(fold=True) and
      the one-by-one path on the same bytes.  The split of succinct_verify_proofs -- head reading (B calls summed), the identity call, the rows
      of scalars, the two row MSM calls, the normalise -- is taken in runs of their own with those functions wrapped, a synchronise before and
      after each (the wrapped runs' totals are not reported); of accumulate, the transcript part (absorb 2 B points, squeeze) is timed alone
      beside the whole
    python tools/accumulate_time.py [--reps 9] [--batches 1,3,64,4096] [--no-rows] [--no-flow] [--flow-shape 13:4:1] [--flow-batches 3,64]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import torch

from zksnap_circuits_halo2_amd import _lib, accumulator as A, fields as F

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--batches", default="1,3,64,4096")
ap.add_argument("--no-rows", action="store_true")
ap.add_argument("--no-flow", action="store_true")
ap.add_argument("--flow-shape", default="13:4:1")
ap.add_argument("--flow-batches", default="3,64")
ap.add_argument("--flow-reps", type=int, default=5)
args = ap.parse_args()
lib = _lib.load()
R = F.R_MOD
DEV = torch.device("cuda", 0)
SHAPES = {"wrapper": (33, 20, 4), "voter": (954, 430, 4)}       # n_cols, n_own, c


def fmt(ts):
    return f"min {min(ts):9.3f} median {statistics.median(ts):9.3f} max {max(ts):9.3f}"


def series(sides, reps):
    """the sides in turn, `reps` times, after one round that warms clocks and scratch: {name: [ms]}"""
    out = {name: [] for name, _ in sides}
    for rep in range(reps + 1):
        for name, fn in sides:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                out[name].append((time.perf_counter() - t) * 1e3)
    return out


def random_elements(*shape):
    a = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device=DEV)
    a[..., 3] = torch.randint(0, 1 << 61, shape, dtype=torch.int64, device=DEV)          # below r: canonical words
    return a


def walk(n, seed):
    out = torch.empty((n, 8), dtype=torch.int64, device=DEV)
    t0, d = F.fr_encode([seed])[0], F.fr_encode([seed * 7 + 3])[0]                 # (kept alive across the call)
    _lib.check(lib.zkhip_g1_gen_walk_device(t0.ctypes.data, d.ctypes.data, n, out.data_ptr(), None))
    return out


def normalised(xyz):
    n = xyz.shape[0]
    out = torch.empty((n, 8), dtype=torch.int64, device=DEV)
    _lib.check(lib.zkhip_g1_batch_normalize_device(xyz.data_ptr(), n, out.data_ptr(), None))
    return out


if not args.no_rows:
    print(f"==== the row MSM against a loop of 2 B zkhip_msm_g1_device calls ({args.reps} alternating repetitions, wall ms, a timed region = A side + C side + synchronise) ====")
    for name, (n_cols, n_own, c) in SHAPES.items():
        for B in (int(b) for b in args.batches.split(",")):
            if name == "voter" and B > 64:
                continue
            rows_a, rows_c = random_elements(B, n_cols), random_elements(B, c)
            own, shared = walk(B * n_own, 0x1234 + B).reshape(B, n_own, 8), walk(n_cols - n_own, 0x99)
            per_row = torch.cat([own, shared[None].expand(B, -1, -1)], dim=1).contiguous()      # the loop's A-side bases, laid out beforehand
            own_c = own[:, :c, :].contiguous()
            out_row, out_loop = torch.empty((2, B, 12), dtype=torch.int64, device=DEV), torch.empty((2, B, 12), dtype=torch.int64, device=DEV)

            def row_call():
                A.row_msm_device(rows_a, own, shared, out=out_row[0])
                A.row_msm_device(rows_c, own, None, n_own=c, out=out_row[1])

            def loop():
                for i in range(B):
                    _lib.check(lib.zkhip_msm_g1_device(rows_a[i].data_ptr(), per_row[i].data_ptr(), n_cols, out_loop[0, i].data_ptr(), None))
                    _lib.check(lib.zkhip_msm_g1_device(rows_c[i].data_ptr(), own_c[i].data_ptr(), c, out_loop[1, i].data_ptr(), None))

            row_call()
            loop()
            assert torch.equal(normalised(out_row.reshape(2 * B, 12)), normalised(out_loop.reshape(2 * B, 12))), "the two sides disagree"
            got = series((("row MSM", row_call), ("loop", loop)), args.reps if B <= 64 else 3)
            for side, ts in got.items():
                print(f"    {name:8s} B = {B:5d}  {side:8s} {fmt(ts)}")
            row_med, loop_min = statistics.median(got["row MSM"]), min(got["loop"])
            print(f"    {name:8s} B = {B:5d}  row MSM median {'below' if row_med < loop_min else 'NOT below'} the loop's minimum ({row_med:.3f} vs {loop_min:.3f}; loop median / row median = "
                  f"{statistics.median(got['loop']) / row_med:.2f})")
            del rows_a, rows_c, own, shared, per_row, own_c, out_row, out_loop

if not args.no_flow:
    import prove_flow
    from zksnap_circuits_halo2_amd import verifier as V

    k, g, l = (int(x) for x in args.flow_shape.split(":"))
    print(f"==== end to end, shape k = {k}, {g} gate columns, {l} lookups, GWC under Poseidon: one proof's bytes repeated B times "
          f"({args.flow_reps} alternating repetitions, wall ms) ====")

    def measure(params, vk, k_, proof, shape_, plan_, *how):
        for B in (int(b) for b in args.flow_batches.split(",")):
            batch = [proof] * B
            succinct = lambda: A.succinct_verify_proofs(params, vk, k_, batch, shape_, plan_, *how)
            folded = lambda: V.verify_transcript_proofs(params, vk, k_, batch, shape_, plan_, *how, fold=True)
            one_by_one = lambda: V.verify_transcript_proofs(params, vk, k_, batch, shape_, plan_, *how)
            res = succinct()
            assert res.status.tolist() == [0] * B and folded() == [True] * B == one_by_one()
            accs = res.accumulators[:, 0].contiguous()
            acc = A.accumulate(accs)[0]
            assert A.decide(params, acc) and A.decide_all(params, accs)
            sides = (("succinct_verify_proofs", succinct), ("accumulate", lambda: A.accumulate(accs)), ("decide", lambda: A.decide(params, acc)),
                     ("decide_all", lambda: A.decide_all(params, accs)), ("verify fold=True", folded), ("verify one by one", one_by_one))
            for name, ts in series(sides, args.flow_reps).items():
                print(f"    B = {B:3d}  {name:24s} {fmt(ts)}   ({statistics.median(ts) / B:.3f} ms a proof)")
            # the phases inside succinct_verify_proofs: runs of their own, each wrapped function between two synchronises
            from zksnap_circuits_halo2_amd import multiopen as MO
            from zksnap_circuits_halo2_amd.transcript import transcript_classes
            spots = (("head reading (B calls)", V, "_read_proof_head"), ("identity call", V, "identity_statuses"), ("rows of scalars", MO, "gwc_scalars_device"),
                     ("row MSM (A, then C)", A, "row_msm_device"), ("normalise", A, "_normalize_device"))
            taken, reals = {name: [] for name, _, _ in spots}, {}

            def wrapped(name, real):
                def call(*a_, **kw):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    out = real(*a_, **kw)
                    torch.cuda.synchronize()
                    taken[name][-1] += (time.perf_counter() - t) * 1e3
                    return out
                return call

            for name, mod, attr in spots:
                reals[name] = getattr(mod, attr)
                setattr(mod, attr, wrapped(name, reals[name]))
            try:
                for _ in range(args.flow_reps + 1):
                    for name in taken:
                        taken[name].append(0.0)
                    succinct()
            finally:
                for name, mod, attr in spots:
                    setattr(mod, attr, reals[name])
            for name, ts in taken.items():
                print(f"    B = {B:3d}  inside it: {name:24s} {fmt(ts[1:])}")
            host = accs.cpu().numpy().view("uint64").reshape(B, 2, 8)

            def transcript_part():
                with transcript_classes(how[0] if how else "blake2b")[0]() as tr:
                    for i in range(B):
                        tr.common_point(host[i, 0])
                        tr.common_point(host[i, 1])
                    tr.squeeze_challenge()

            print(f"    B = {B:3d}  accumulate: transcript part alone  {fmt(series((('t', transcript_part),), args.flow_reps)['t'])}")
        return True

    real_verify = prove_flow.verify_transcript_proof
    prove_flow.verify_transcript_proof = measure
    try:
        prove_flow.run(k, g, lookups=l, verbose=False, transcript="poseidon", verify=True, multiopen="gwc")
    finally:
        prove_flow.verify_transcript_proof = real_verify

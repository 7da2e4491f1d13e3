#!/usr/bin/env python3
"""The pairing check and the verifiers built on it, timed on one MI355X: one process, clocks warmed first, 9 repetitions, wall ms, medians; every
timed region ends with the verdict on the host.

  zkhip_pairing_check at n = 2 and n = 64 (host form: upload, kernel, verdict back)
  the check of two pairs as ONE serial chain through the quad policy and through the single-lane policy (hook operation 11 of
      zkhip_test_fq12_op): the measured gain of sharing every Fq2 product among four lanes
  VerifierSHPLONK / VerifierGWC on the plans tools/prove_flow.py opens at (k, gate columns, lookups) = (22, 4, 1), (13, 256, 8), (15, 64, 8), split
      into the G1 side (normalisation + small MSMs) and the pairing
  ParamsKZG.verify at k = 22
  the `verify` lap of prove_flow.run(verify=True) beside prove_ms, three warm proofs per shape
  zkhip_verify_identity_device (the quotient identity at x, csrc/verify_identity.hip) at B = 1, 64 and 4096 proofs on the same plans: the records are
      random field elements already in HBM (the time does not depend on the verdicts), the program is compiled and marshalled once (that time is
      printed beside it), a timed region is the call and the statuses and the report back on the host
  the `verify` lap of the transcript flow with the identity and without it -- the openings alone are what the verifier was before the identity was
      added --, the two sides in turn in this one process
  the identity call with and without ONE instance column of 30 public values (zkhip_verify_identity_instances_device against
      zkhip_verify_identity_device on the same records), the repetitions of the two alternating, a second series of the call without as the A/A
      figure; beside it the host path a caller had before the device evaluated instance columns: the same evaluations on Python integers with
      one batched inversion per proof, and their upload
  the batch verifier: verifier.verify_transcript_proofs one by one against fold=True (one folded pairing check per batch, multiopen.fold_check) in this one
      process, the two sides alternating, for B in {1, 4, 16, 64} proofs and both multi-opens on the same shapes; the batch is ONE proof's bytes
      repeated B times (an honest input for timing: every copy is read, checked and folded like any other proof; the output says so); and the two
      calls behind it alone, zkhip_gwc_scalars_device, zkhip_fr_fold_rows_device and zkhip_shplonk_scalars_device, at B = 1, 64 and 4096 on
      random records
    python tools/verify_time.py [--reps 9] [--shapes 22:4:1,13:256:8,15:64:8] [--no-pairing] [--no-flow] [--no-srs] [--no-identity] [--no-instances] [--no-batch]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import numpy as np
import torch

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, arithmetic as A, fields as F, kzg, multiopen as MO, srs

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--shapes", default="22:4:1,13:256:8,15:64:8")
ap.add_argument("--no-flow", action="store_true")
ap.add_argument("--no-srs", action="store_true")
ap.add_argument("--srs-k", type=int, default=22)
ap.add_argument("--no-pairing", action="store_true")
ap.add_argument("--no-identity", action="store_true")
ap.add_argument("--batches", default="1,64,4096")
ap.add_argument("--no-instances", action="store_true")
ap.add_argument("--instance-len", type=int, default=30)
ap.add_argument("--no-batch", action="store_true")
ap.add_argument("--fold-batches", default="1,4,16,64")
ap.add_argument("--batch-reps", type=int, default=3)
args = ap.parse_args()
lib = _lib.load()
R = O.R_MOD


def fmt(ts):
    return f"min {min(ts):.3f} median {statistics.median(ts):.3f} max {max(ts):.3f}"


def timed(fn, reps=None, warm_s=0.5):
    t_end = time.perf_counter() + warm_s
    while True:
        fn()
        if time.perf_counter() >= t_end:
            break
    out = []
    for _ in range(reps or args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


# ---- the check itself ------------------------------------------------------------------------------------------------------------------------
def pairs(n):
    """n pairs (a_i G, b_i H) with sum a_i b_i = 0: 4 distinct points on either side"""
    a = [3 + i for i in range(4)]
    b = [11 + i for i in range(4)]
    ab = [(a[i % 4], b[(i // 4) % 4]) for i in range(n - 1)]
    s = sum(x * y for x, y in ab) % R
    ab.append((R - s, 1))
    g1 = F.g1_encode([O.scalar_mul(x % R, O.G1_GEN) for x, _ in ab])
    g2 = np.stack([srs.g2_encode(srs.g2_mul(y % R)) for _, y in ab])
    return g1, g2


if not args.no_pairing:
    print(f"zkhip_pairing_check, host form ({args.reps} repetitions, wall ms, the verdict on the host)")
    for n in (2, 64):
        g1, g2 = pairs(n)
        assert A.pairing_check(g1, g2)
        print(f"    n = {n:2d}                                                  {fmt(timed(lambda: A.pairing_check(g1, g2)))}")
    g1, g2 = pairs(2)
    operand = np.concatenate([g1.reshape(-1), g2.reshape(-1)]).astype(np.uint64)
    out = np.zeros(96, dtype=np.uint64)
    med = {}
    for name, flag in (("quad policy", 256), ("single-lane policy", 512)):
        def run(flag=flag):
            _lib.check(lib.zkhip_test_fq12_op(11 + flag, operand.ctypes.data, operand.ctypes.data, out.ctypes.data))
        run()
        assert out[0 if flag == 256 else 48] == 1
        ts = timed(run)
        med[name] = statistics.median(ts)
        print(f"    two pairs as one serial chain, {name:20s}        {fmt(ts)}")
    print(f"    single-lane / quad = {med['single-lane policy'] / med['quad policy']:.2f}")

# ---- ParamsKZG.verify ------------------------------------------------------------------------------------------------------------------------
if not args.no_srs:
    t0 = time.perf_counter()
    with kzg.ParamsKZG.setup(args.srs_k, 0x1122334455667788) as params:
        print(f"ParamsKZG.verify at k = {args.srs_k} (setup {time.perf_counter() - t0:.1f} s, not timed)")
        seed = bytes(range(32))
        assert params.verify(seed)
        print(f"    verify                                                  {fmt(timed(lambda: params.verify(seed), reps=3, warm_s=0.0))}")

# ---- the verifiers on the flow's plans, and the flow's own lap ---------------------------------------------------------------------------------
if not args.no_flow:
    import prove_flow

    for shape in args.shapes.split(","):
        k, g, l = (int(x) for x in shape.split(":"))
        print(f"==== prove_flow shape k = {k}, {g} gate columns, {l} lookups ====")

        def measure(params, k_, queries, vqueries, commit, proof, challenges):
            H, Hp = proof
            y, v, u = challenges
            Gx = MO._generator_xyz(params)
            pair = lambda left, right_neg: A.pairing_check(np.stack([left, right_neg]), np.stack([params.g2, params.s_g2]))
            # SHPLONK
            def g1_side():
                scalars, commitments = MO.shplonk_accumulate(vqueries, y, v, u)
                left = A.g1_combination(scalars, np.stack(MO.commitment_points(vqueries, commitments) + [Gx, H, Hp]))
                return left, A.g1_combination([-1], Hp.reshape(1, 12))
            left, right_neg = g1_side()
            assert pair(left, right_neg)
            print(f"    VerifierSHPLONK: {len(vqueries)} queries, {len(MO.shplonk_accumulate(vqueries, y, v, u)[1]) + 3} points")
            print(f"      G1 side (scalars, normalisation, MSM)                 {fmt(timed(g1_side))}")
            print(f"      pairing check                                         {fmt(timed(lambda: pair(left, right_neg)))}")
            print(f"      verify_proof                                          {fmt(timed(lambda: MO.VerifierSHPLONK(params).verify_proof(vqueries, H, Hp, y, v, u)))}")
            # GWC on the same plan
            gwc = MO.ProverGWC(k_, commit)
            fresh = [MO.ProverQuery(q.point, q.poly, q.eval) for q in queries]
            W = gwc.create_proof(fresh, v)
            gwc.close()
            def g1_side_gwc():
                lft, rgt, commitments = MO.gwc_accumulate(vqueries, len(W), v, u)
                Wl = [np.ascontiguousarray(w, dtype=np.uint64).reshape(12) for w in W]
                return A.g1_combination(rgt, np.stack(Wl + MO.commitment_points(vqueries, commitments) + [Gx])), A.g1_combination([-s for s in lft], np.stack(Wl))
            left_g, right_g = g1_side_gwc()
            assert pair(left_g, right_g)
            print(f"    VerifierGWC: {len(W)} witnesses")
            print(f"      G1 side (scalars, normalisation, MSM)                 {fmt(timed(g1_side_gwc))}")
            print(f"      pairing check                                         {fmt(timed(lambda: pair(left_g, right_g)))}")
            print(f"      verify_proof                                          {fmt(timed(lambda: MO.VerifierGWC(params).verify_proof(vqueries, W, v, u)))}")

        prove_flow.run(k, g, lookups=l, verbose=False, verify=True, on_proof=measure)
        laps = []
        for _ in range(3):
            res = prove_flow.run(k, g, lookups=l, verbose=False, verify=True)
            assert all(res["checks"].values())
            laps.append((res["timings_ms"]["verify"], res["prove_ms"]))
        print("    flow, three warm proofs: verify lap / prove_ms = " + ", ".join(f"{a:.1f} / {b:.1f}" for a, b in laps))

def random_elements(*shape):
    a = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device="cuda")
    a[..., 3] = torch.randint(0, 1 << 61, shape, dtype=torch.int64, device="cuda")          # below r: canonical words
    return a


# ---- the quotient identity at x: the call on its own, and the flow's verify lap with and without it ------------------------------------------------
if not args.no_identity:
    import prove_flow
    from zksnap_circuits_halo2_amd import evaluation as E, prover as P, verifier as V

    for shape in args.shapes.split(","):
        k, g, l = (int(x) for x in shape.split(":"))
        cs = E.halo2_lib_shape(g, l)
        u = (1 << k) - (cs.blinding_factors + 1)
        plan = P.opening_plan(cs, g, l, u, False, "halo2")
        t0 = time.perf_counter()
        prog = E.identity_program(cs, plan, k)
        t1 = time.perf_counter()
        marshalled = prog._marshal()
        t2 = time.perf_counter()
        print(f"==== identity at x, shape k = {k}, {g} gate columns, {l} lookups: {len(plan)} evaluations, {len(prog.insns)} instructions, {prog.registers_used()} registers "
              f"(compiled in {(t1 - t0) * 1e3:.1f} ms, marshalled in {(t2 - t1) * 1e3:.1f} ms, once per key) ====")
        for B in (int(b) for b in args.batches.split(",")):
            evals, challenges = random_elements(B, len(plan)), random_elements(B, 5)
            status, (failures, first) = E.verify_identity_device(marshalled, evals, challenges, k, u)
            assert len(status) == B and failures == int((status != 0).sum())
            ts = timed(lambda: E.verify_identity_device(marshalled, evals, challenges, k, u))
            print(f"    B = {B:5d}                                               {fmt(ts)}   ({statistics.median(ts) / B * 1e3:.2f} us a proof)")
            del evals, challenges
        if not args.no_flow:
            with_identity = prove_flow.verify_transcript_proof
            openings_alone = lambda params, vk, k_, proof, shape_, plan_, *how: V.verify_transcript_proofs(params, vk, k_, [proof], shape_, plan_, *how, identity=False)[0]
            laps = {"openings alone": [], "identity + openings": []}
            try:
                for _ in range(3):
                    for name, verifier in (("openings alone", openings_alone), ("identity + openings", with_identity)):
                        prove_flow.verify_transcript_proof = verifier
                        res = prove_flow.run(k, g, lookups=l, verbose=False, transcript=True, verify=True)
                        assert all(res["checks"].values())
                        laps[name].append(res["timings_ms"]["verify"])
            finally:
                prove_flow.verify_transcript_proof = with_identity
            for name, ts in laps.items():
                print(f"    transcript flow, verify lap, {name:22s}      {fmt(ts)}   (three proofs; every run makes its key anew, so every lap compiles and marshals the identity once)")

# ---- instance columns: what the identity call pays for evaluating one on the device, against the host path -----------------------------------------
if not args.no_instances:
    import random

    from zksnap_circuits_halo2_amd import evaluation as E, prover as P

    def host_instance_evals(k, xs, values, length):
        """e[p] = sum_i v[p][i] l_i(x_p) on Python integers: the denominators x_p - omega^i of a proof share one inversion (Montgomery's trick)"""
        n, w = 1 << k, [pow(F.omega_for(k), i, R) for i in range(length)]
        n_inv, out = pow(n, R - 2, R), []
        for x, v in zip(xs, values):
            den, run = [(x - wi) % R for wi in w], [1]
            for d in den:
                run.append(run[-1] * d % R)
            inv, acc = pow(run[-1], R - 2, R), 0
            for i in range(length - 1, -1, -1):
                acc = (acc + v[i] * w[i] % R * (inv * run[i] % R)) % R
                inv = inv * den[i] % R
            out.append(acc * (pow(x, n, R) - 1) % R * n_inv % R)
        return out

    length = args.instance_len
    for shape in args.shapes.split(","):
        k, g, l = (int(x) for x in shape.split(":"))
        plain_cs, cs = E.halo2_lib_shape(g, l), E.halo2_lib_shape(g, l, instances=1)
        u = (1 << k) - (cs.blinding_factors + 1)
        plain_plan, plan = P.opening_plan(plain_cs, g, l, u, False, "halo2"), P.opening_plan(cs, g, l, u, False, "halo2")
        queries = E.instance_queries(cs)
        plain_prog, prog = E.identity_program(plain_cs, plain_plan, k)._marshal(), E.identity_program(cs, plan, k, instance_queries=queries)._marshal()
        print(f"==== identity at x with one instance column of {length} values, shape k = {k}, {g} gate columns, {l} lookups: {len(plain_plan)} / {len(plan)} evaluations "
              f"without / with ({args.reps} alternating repetitions, wall ms, medians) ====")
        rng = random.Random(k)
        for B in (int(b) for b in args.batches.split(",")):
            plain_evals, evals, challenges, instances = random_elements(B, len(plain_plan)), random_elements(B, len(plan)), random_elements(B, 5), random_elements(B, length)
            xs, values = [rng.randrange(R) for _ in range(B)], [[rng.randrange(R) for _ in range(length)] for _ in range(B)]
            without = lambda: E.verify_identity_device(plain_prog, plain_evals, challenges, k, u)
            with_column = lambda: E.verify_identity_device(prog, evals, challenges, k, u, instances=instances, column_lens=[length], queries=queries)
            def host():
                e = host_instance_evals(k, xs, values, length)
                torch.from_numpy(F.fr_encode(e).view(np.int64)).cuda()
                torch.cuda.synchronize()
            series = {"without": [], "with": [], "without (A/A)": [], "host": []}
            timed(with_column, reps=1)                                     # clocks and scratch warm
            for _ in range(args.reps):
                for name, fn in (("without", without), ("with", with_column), ("without (A/A)", without), ("host", host)):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn()
                    series[name].append((time.perf_counter() - t) * 1e3)
            med = {name: statistics.median(ts) for name, ts in series.items()}
            for name, ts in series.items():
                print(f"    B = {B:5d}  {name:15s}                              {fmt(ts)}")
            print(f"    B = {B:5d}  added by the column on the device {med['with'] - med['without']:+.3f} ms (A/A {med['without (A/A)'] - med['without']:+.3f} ms); "
                  f"host integers + upload {med['host']:.3f} ms")

# ---- the batch verifier: one folded pairing check per batch against one check per proof ------------------------------------------------------------
if not args.no_batch:
    import prove_flow
    from zksnap_circuits_halo2_amd import evaluation as E, prover as P, verifier as V

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

    for shape in args.shapes.split(","):
        k, g, l = (int(x) for x in shape.split(":"))
        for mo in ("gwc", "shplonk"):
            print(f"==== batch verifier, shape k = {k}, {g} gate columns, {l} lookups, multiopen = {mo}: one proof's bytes repeated B times "
                  f"({args.batch_reps} alternating repetitions, wall ms) ====")

            def measure(params, vk, k_, proof, shape_, plan_, *how):
                for B in (int(b) for b in args.fold_batches.split(",")):
                    batch = [proof] * B
                    one_by_one = lambda: V.verify_transcript_proofs(params, vk, k_, batch, shape_, plan_, *how)
                    folded = lambda: V.verify_transcript_proofs(params, vk, k_, batch, shape_, plan_, *how, fold=True)
                    assert one_by_one() == [True] * B == folded()
                    got = series((("one by one", one_by_one), ("fold=True", folded)), args.batch_reps)
                    for name, ts in got.items():
                        print(f"    B = {B:3d}  {name:12s}                                  {fmt(ts)}   ({statistics.median(ts) / B:.2f} ms a proof)")
                    print(f"    B = {B:3d}  one by one / fold = {statistics.median(got['one by one']) / statistics.median(got['fold=True']):.2f}")
                return True

            real = prove_flow.verify_transcript_proof
            prove_flow.verify_transcript_proof = measure
            try:
                prove_flow.run(k, g, lookups=l, verbose=False, transcript=True, verify=True, multiopen=mo)
            finally:
                prove_flow.verify_transcript_proof = real
        # the two calls alone, on random records
        cs = E.halo2_lib_shape(g, l)
        plan = P.opening_plan(cs, g, l, (1 << k) - (cs.blinding_factors + 1), False, "halo2")
        gp = MO.gwc_plan(plan)
        n_cols, n_own = gp.n_sets + gp.n_slots + 1, gp.n_sets + len(gp.own_keys)
        print(f"==== the batch verifier's two calls alone, shape k = {k}, {g} gate columns, {l} lookups: {gp.n_evals} queries, {gp.n_sets} sets, {gp.n_slots} polynomials "
              f"({n_cols} columns, {n_own} own); random records in HBM, a timed region ends with a device synchronise ====")
        for B in (int(b) for b in args.batches.split(",")):
            evals, points, r = random_elements(B, gp.n_evals), random_elements(B, 3), random_elements(B)
            def scalars():
                MO.gwc_scalars_device(gp, evals, points, k)
                torch.cuda.synchronize()
            rows_a, _ = MO.gwc_scalars_device(gp, evals, points, k)
            out_own, out_shared = torch.empty((B * n_own, 4), dtype=torch.int64, device="cuda"), torch.empty((n_cols - n_own, 4), dtype=torch.int64, device="cuda")
            def fold():
                MO.fold_rows_device(rows_a, n_own, r, False, out_own, out_shared)
                torch.cuda.synchronize()
            print(f"    B = {B:5d}  zkhip_gwc_scalars_device (plan marshalled in the call)   {fmt(timed(scalars))}")
            print(f"    B = {B:5d}  zkhip_fr_fold_rows_device                                {fmt(timed(fold))}")
            del evals, points, r, rows_a, out_own, out_shared
        sp = MO.shplonk_plan(plan)
        print(f"==== the SHPLONK scalars alone, same shape: {sp.n_evals} queries, {sp.n_points} points, {sp.n_sets} rotation sets "
              f"({sum(len(pts) for pts in sp.set_points)} pairs), {sp.n_slots} polynomials ({sp.n_slots + 3} columns) ====")
        for B in (int(b) for b in args.batches.split(",")):
            evals, points = random_elements(B, sp.n_evals), random_elements(B, 4)
            def shplonk_scalars():
                MO.shplonk_scalars_device(sp, evals, points, k)
                torch.cuda.synchronize()
            assert not bool(MO.shplonk_scalars_device(sp, evals, points, k)[2].any())
            print(f"    B = {B:5d}  zkhip_shplonk_scalars_device (plan marshalled in the call) {fmt(timed(shplonk_scalars))}")
            del evals, points

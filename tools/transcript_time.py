#!/usr/bin/env python3
"""What the Blake2b transcript costs per proof (profiles/r14_transcript.txt).  One process, alternating repetitions, medians.

  flow   tools/prove_flow.py with and without `transcript=True`, and the seeded flow against itself (the A/A spread): `prove_ms`, and the
         transcript's own laps.
  calls  the bytes of one proof's transcript -- P commitments in the flow's phase batches and S evaluations, counted from the flow's plan --
         through the new calls (write_points / write_scalars on device buffers, squeezes) against the parent commit's way of getting the same
         bytes: download every 96-byte Jacobian point, normalise it with Python big integers (prove_flow's `affine()`), download the
         evaluations, and hashlib over the result.  Both sides end with the same final challenge, which is compared.

Usage: transcript_time.py K GATE_COLS LOOKUPS [--reps 9] [--no-flow] [--once]     (--once: one transcript flow and nothing else, for a kernel trace)"""
import hashlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import numpy as np
import torch

import prove_flow
from zksnap_circuits_halo2_amd import _lib, fields as F
from zksnap_circuits_halo2_amd.transcript import Blake2bWrite

R, Q = F.R_MOD, F.Q_MOD


def median(v):
    return statistics.median(v)


def flow_rows(k, g, lk, reps):
    kinds = {"seeded": {}, "seeded_again": {}, "transcript": {"transcript": True}}
    prove = {name: [] for name in kinds}
    laps = []
    prove_flow.run(k, g, lookups=lk, verbose=False, transcript=True)                  # warm: tables, scratch, compiled programs
    res = None
    for _ in range(reps):
        for name, kw in kinds.items():
            res = prove_flow.run(k, g, lookups=lk, verbose=False, **kw)
            prove[name].append(res["prove_ms"])
            if name == "transcript":
                laps.append(res["timings_ms"]["transcript"])
    print(f"flow ({k}, {g}, {lk}): prove_ms median of {reps}: seeded {median(prove['seeded']):.2f}  seeded again {median(prove['seeded_again']):.2f}  "
          f"transcript {median(prove['transcript']):.2f}  (its `transcript` laps {median(laps):.2f}); proof {res['proof_bytes']} bytes")
    return res


def call_rows(shape, n_scalars, reps):
    lib = _lib.load()
    n_adv, n_lk, n_sets = shape["advice"], shape["lookups"], shape["permutation_sets"]
    batches = [b for b in (n_adv, 2 * n_lk, n_sets + n_lk, 1 if shape["random_poly"] else 0, 3, 1, 1) if b]
    total = sum(batches)
    # commitments: a walk of curve points given random z's on the device side of the interface (Jacobian, as an MSM leaves them)
    rng = np.random.default_rng(5)
    walk = torch.zeros((total, 8), dtype=torch.int64, device="cuda")
    t0w, dw = F.fr_encode([0xABCDEF])[0], F.fr_encode([0x1234567])[0]
    _lib.check(lib.zkhip_g1_gen_walk_device(t0w.ctypes.data, dw.ctypes.data, total, walk.data_ptr(), None))
    aff = walk.cpu().numpy().view(np.uint64)
    inv = pow(F.MONT, -1, Q)
    pts = [tuple(sum(int(aff[i, 4 * c + j]) << (64 * j) for j in range(4)) * inv % Q for c in range(2)) for i in range(total)]
    jac = np.zeros((total, 12), dtype=np.uint64)
    for i, (x, y) in enumerate(pts):
        z = int(rng.integers(2, 1 << 62)) * 0x9E3779B97F4A7C15 % Q
        for c, v in enumerate((x * z * z % Q, y * z * z * z % Q, z)):
            m = v * F.MONT % Q
            jac[i, 4 * c:4 * c + 4] = [(m >> (64 * j)) & ((1 << 64) - 1) for j in range(4)]
    d_points = torch.from_numpy(jac.view(np.int64)).to("cuda")
    d_scalars = torch.from_numpy(F.fr_encode([int(v) for v in rng.integers(1, 1 << 62, n_scalars)]).view(np.int64)).to("cuda")
    offs = np.cumsum([0] + batches)

    def new_calls():
        with Blake2bWrite() as t:
            for b in range(len(batches) - 2):
                t.write_points(d_points[offs[b]:offs[b + 1]])
                t.squeeze_challenge()
            t.write_scalars(d_scalars)
            for b in (len(batches) - 2, len(batches) - 1):
                t.squeeze_challenge()
                t.write_points(d_points[offs[b]:offs[b + 1]])
            return t.squeeze_challenge(), t.finalize()

    def parent_way():
        h = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
        proof = bytearray()

        def point(i):
            x, y = F.g1_decode_jacobian(d_points[i].cpu().numpy().view(np.uint64))    # prove_flow's affine(): one download and one inversion per point
            h.update(b"\x01" + x.to_bytes(32, "little") + y.to_bytes(32, "little"))
            enc = bytearray(x.to_bytes(32, "little"))
            enc[31] |= (y & 1) << 6
            proof.extend(enc)

        def squeeze():
            h.update(b"\x00")
            return int.from_bytes(h.copy().digest(), "little") % R

        for b in range(len(batches) - 2):
            for i in range(offs[b], offs[b + 1]):
                point(i)
            squeeze()
        for s in F.fr_decode(d_scalars.cpu().numpy().view(np.uint64)):
            rep = s.to_bytes(32, "little")
            h.update(b"\x02" + rep)
            proof.extend(rep)
        for b in (len(batches) - 2, len(batches) - 1):
            squeeze()
            point(offs[b])
        return squeeze(), bytes(proof)

    assert new_calls() == parent_way(), "the two ways disagree"
    times = {"new": [], "parent": []}
    for _ in range(reps):
        for name, fn in (("new", new_calls), ("parent", parent_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    print(f"calls: {total} points in {len(batches)} batches + {n_scalars} scalars: new calls {median(times['new']):.3f} ms  "
          f"parent's way (download + Python affine + hashlib) {median(times['parent']):.3f} ms  (median of {reps}; same bytes, same challenge)")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    k, g, lk = (int(a) for a in args[:3])
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
    if "--once" in sys.argv:
        out = prove_flow.run(k, g, lookups=lk, verbose=False, transcript=True)
        print(f"one transcript flow ({k}, {g}, {lk}): prove_ms {out['prove_ms']:.2f}, proof {out['proof_bytes']} bytes")
        sys.exit(0)
    if "--no-flow" in sys.argv:
        last = prove_flow.run(k, g, lookups=lk, verbose=False, transcript=True)
    else:
        last = flow_rows(k, g, lk, reps)
    call_rows(last["proof_shape"], len(last["proof_plan"]), reps)

#!/usr/bin/env python3
"""What the PLUME check costs on the device (DESIGN.md sections 4b and 9, profiles/r19_plume.txt).  One process, REPS repetitions after one
warm repetition of every size, the sides taken in turn, medians (minimum in brackets), wall ms; every device region ends with a device
synchronise.

  verify    plume.verify_many_device over B voters already in device memory, B = 1, 2, 4 .. 2^16.  The voters are POOL valid ones generated
            with `gen_native` and repeated to fill the batch: the kernel has no data-dependent path but the map's second square root, which a
            wavefront of 32 voters takes almost always.  The verdicts are compared with 0 on the first repetition.
  h2c       plume.hash_to_curve_many_device over the same B public keys.
  lincomb   plume.lincomb_device over B random 256-bit scalar pairs and the same points.
  host      the library's own `verify_native` on one core over the first HOST_SAMPLE voters of the batch, SCALED to B (labelled).  This is the
            reference's flow: one voter at a time before a round's inputs are built.
  crossover the first B at which the device call plus the read-back of the report (`.failures`) is below the host loop, over every B.

Usage: plume_time.py [--reps 7] [--quick] [--out profiles/r19_plume.txt]      (--quick: B up to 64, a rehearsal)"""
import hashlib
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from zksnap_circuits_halo2_amd import plume as PL  # noqa: E402

median = statistics.median
POOL = 32
HOST_SAMPLE = 4
MSG = bytes([1, 0])


def fmt(xs):
    return f"{median(xs):10.3f} ({min(xs):.3f})"


def main():
    argv, reps = sys.argv[1:], 7
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    quick = "--quick" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(os.path.dirname(HERE), "profiles", "r19_plume.txt")
    import torch

    rng = random.Random(19)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def sync():
        torch.cuda.synchronize()

    t0 = time.perf_counter()
    pool = [PL.gen_native(rng.randrange(1, PL.N), MSG, rng.randrange(1, PL.N)) for _ in range(POOL)]
    gen_ms = (time.perf_counter() - t0) * 1e3 / POOL
    say(f"PLUME nullifiers, {torch.cuda.get_device_name(0)}: median of {reps} (min) in ms after one warm repetition, sides in turn; msg = 01 00; "
        f"{POOL} generated voters repeated to fill a batch (gen_native: {gen_ms:.1f} ms each on the host)")
    pk_pool, nul_pool = PL.encode_points([v[0] for v in pool]), PL.encode_points([v[1] for v in pool])
    s_pool, c_pool = PL.encode_scalars([v[2] for v in pool]), PL.encode_scalars([v[3] for v in pool])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(19)
    series = []
    for B in [1 << k for k in range(0, 7 if quick else 17)]:
        fill = lambda t: t.repeat((B + POOL - 1) // POOL, 1)[:B].contiguous()
        pk, nul, s, c = fill(pk_pool), fill(nul_pool), fill(s_pool), fill(c_pool)
        a = torch.randint(-(1 << 63), (1 << 63) - 1, (B, 4), dtype=torch.int64, device="cuda", generator=gen)
        b = torch.randint(-(1 << 63), (1 << 63) - 1, (B, 4), dtype=torch.int64, device="cuda", generator=gen)
        hb = min(B, HOST_SAMPLE)
        t_ver, t_h2c, t_lin, t_host, t_cross = [], [], [], [], []
        for r in range(reps + 1):
            sync()
            t0 = time.perf_counter()
            found = PL.verify_many_device(MSG, pk, nul, s, c)
            sync()
            t1 = time.perf_counter()
            h, h_status = PL.hash_to_curve_many_device(MSG, pk)
            sync()
            t2 = time.perf_counter()
            out, l_status = PL.lincomb_device(a, pk, b, nul)
            sync()
            t3 = time.perf_counter()
            failures = PL.verify_many_device(MSG, pk, nul, s, c).failures
            t4 = time.perf_counter()
            verdicts = [PL.verify_native(MSG, v[1], v[0], v[2], v[3]) for v in pool[:hb]]
            t5 = time.perf_counter()
            if r == 0:
                assert failures == 0 and verdicts == [0] * hb and not found.status.any().item(), "a generated voter was refused"
                assert torch.equal(h, found.h) and not h_status.any().item() and not l_status.any().item()
                first = PL.decode_points(out[:1])[0]
                assert first == PL.lincomb(PL.decode_scalars(a[:1])[0], pool[0][0], PL.decode_scalars(b[:1])[0], pool[0][1]), "device and host lincomb differ"
            else:
                t_ver.append((t1 - t0) * 1e3)
                t_h2c.append((t2 - t1) * 1e3)
                t_lin.append((t3 - t2) * 1e3)
                t_cross.append((t4 - t3) * 1e3)
                t_host.append((t5 - t4) * 1e3 * B / hb)
        ver, host = median(t_ver), median(t_host)
        series.append((B, median(t_cross), host))
        say(f"B {B:6d}:  verify {fmt(t_ver)}   h2c {fmt(t_h2c)}   lincomb {fmt(t_lin)}   verify + report read back {fmt(t_cross)}   host verify_native {fmt(t_host)}"
            f"{'' if hb == B else f' [{hb} timed, SCALED by {B // hb}]'}   host / device {host / ver:10.1f}   device per voter {ver * 1e3 / B:9.2f} us")
    below = [B for B, dev, host in series if dev < host]
    say(f"the device call's median (report read back) first drops below the one-core host loop's at B = {below[0] if below else 'no measured B'} of {[B for B, _, _ in series]}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

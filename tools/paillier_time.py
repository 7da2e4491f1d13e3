#!/usr/bin/env python3
"""What the Paillier tally and the batched encryption cost (DESIGN.md sections 4b and 9, profiles/r17_paillier.txt).  One process, REPS
repetitions after one warm repetition, the sides taken in turn, medians (minimum in brackets), wall ms; every device region ends with a device
synchronise, the crossover's with the tally on the host.

  tally     paillier.tally_device over B ballots of C = 5 ciphertexts already in device memory (random 384-bit words: unreduced inputs are
            part of the contract), n the 176-bit modulus of the tests.
  host      the reference's loop on one core: `add_native` ballot by ballot over Python integers.  Above HOST_SAMPLE ballots the loop runs
            over the first HOST_SAMPLE and the time is SCALED (labelled).  Its rows are compared with the device's over that prefix.
  fr scan   zkhip_fr_prefix_product_device over the same NUMBER of elements (5 B Fr elements, 32 bytes each): the yardstick of a 12-limb
            run-time ring against the 9-limb compile-time field, same scan shape.
  encrypt   paillier.encrypt_many_device over 5 * 2^16 (vote, r) pairs, random 256-bit votes (the worst case of the per-lane ladder) and
            one-hot votes (the reference's), against `enc_native` over a sample, SCALED.
  crossover B = 1, 2, 4 .. 1024: the device call plus `.total()` on the host against the host loop plus nothing; the first B where the
            device median is below the host median.

Usage: paillier_time.py [--reps 9] [--quick] [--out profiles/r17_paillier.txt]      (--quick: small sizes only, a rehearsal)"""
import os
import random
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from zksnap_circuits_halo2_amd import _lib, paillier as P  # noqa: E402

median = statistics.median
HOST_SAMPLE = 1 << 14
ENC_SAMPLE = 256
C = 5


def fmt(xs):
    return f"{median(xs):10.3f} ({min(xs):.3f})"


def host_tally(n, rows):
    acc = [1] * C
    out = [acc]
    for row in rows:
        acc = [P.add_native(n, x, y) for x, y in zip(acc, row)]
        out.append(acc)
    return out


def main():
    argv, reps = sys.argv[1:], 9
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    quick = "--quick" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(os.path.dirname(HERE), "profiles", "r17_paillier.txt")
    import torch

    lib = _lib.load()
    rng = random.Random(17)
    n = rng.getrandbits(176) | (1 << 175) | 1
    g = n + 1
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def sync():
        torch.cuda.synchronize()

    say(f"Paillier tally, {torch.cuda.get_device_name(0)}: median of {reps} (min) in ms after one warm repetition, sides in turn; n has {n.bit_length()} bits, C = {C}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    sizes = [1 << 6, 1 << 10] if quick else [1 << 10, 1 << 16, 1 << 20]
    for B in sizes:
        ballots = torch.randint(-(1 << 63), (1 << 63) - 1, (B, C, 6), dtype=torch.int64, device="cuda", generator=gen)
        fr = torch.randint(1, 1 << 61, (B * C, 4), dtype=torch.int64, device="cuda", generator=gen)        # four words below 2^61: a reduced Montgomery element
        fr_out = torch.empty_like(fr)
        hb = min(B, HOST_SAMPLE)
        rows = P.decode(ballots[:hb])
        t_dev, t_fr, t_host = [], [], []
        for r in range(reps + 1):
            sync()
            t0 = time.perf_counter()
            tally = P.tally_device(n, ballots)
            sync()
            t1 = time.perf_counter()
            _lib.check(lib.zkhip_fr_prefix_product_device(fr.data_ptr(), B * C, fr_out.data_ptr(), None))
            sync()
            t2 = time.perf_counter()
            want = host_tally(n, rows)
            t3 = time.perf_counter()
            if r == 0:
                assert P.decode(tally.running[:hb + 1]) == want, "device and host tallies differ"
            else:
                t_dev.append((t1 - t0) * 1e3)
                t_fr.append((t2 - t1) * 1e3)
                t_host.append((t3 - t2) * 1e3 * B / hb)
        dev, host, frm = median(t_dev), median(t_host), median(t_fr)
        say(f"tally  B {B:8d}:  device {fmt(t_dev)}   host loop {fmt(t_host)}{'' if hb == B else f' [first {hb} ballots timed, SCALED by {B // hb}]'}   host / device {host / dev:9.2f}"
            f"   fr scan of {B * C} elements {fmt(t_fr)}   tally / fr scan {dev / frm:6.2f}   device per ciphertext {dev * 1e6 / (B * C):8.1f} ns")
        del ballots, fr, fr_out, tally

    count = C * (1 << (8 if quick else 16))
    for kind in ("random 256-bit votes", "one-hot votes"):
        if kind.startswith("random"):
            m = torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda", generator=gen)
        else:
            m = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
            m[::C, 0] = 1
        rr = torch.randint(0, (1 << 48) - 1, (count, 3), dtype=torch.int64, device="cuda", generator=gen)      # r below 2^176, as `gen_biguint(ENC_BIT_LEN)`
        ms, rs = P.decode(m[:ENC_SAMPLE]), P.decode(rr[:ENC_SAMPLE])
        t_dev, t_host = [], []
        for r in range(reps + 1):
            sync()
            t0 = time.perf_counter()
            enc = P.encrypt_many_device(n, g, m, rr)
            sync()
            t1 = time.perf_counter()
            want = [P.enc_native(n, g, x, y) for x, y in zip(ms, rs)]
            t2 = time.perf_counter()
            if r == 0:
                assert P.decode(enc[:ENC_SAMPLE]) == want, "device and host encryptions differ"
            else:
                t_dev.append((t1 - t0) * 1e3)
                t_host.append((t2 - t1) * 1e3 * count / ENC_SAMPLE)
        say(f"encrypt {count} ciphertexts, {kind}:  device {fmt(t_dev)}   enc_native {fmt(t_host)} [{ENC_SAMPLE} timed, SCALED by {count // ENC_SAMPLE}]"
            f"   host / device {median(t_host) / median(t_dev):9.2f}   device per ciphertext {median(t_dev) * 1e3 / count:8.3f} us")

    series = []
    for B in [1 << k for k in range(0, 11)]:
        ballots = torch.randint(-(1 << 63), (1 << 63) - 1, (B, C, 6), dtype=torch.int64, device="cuda", generator=gen)
        rows = P.decode(ballots)
        t_dev, t_host = [], []
        for r in range(reps + 1):
            sync()
            t0 = time.perf_counter()
            total = P.tally_device(n, ballots).total()
            t1 = time.perf_counter()
            want = host_tally(n, rows)[-1]
            t2 = time.perf_counter()
            assert total == want
            if r:
                t_dev.append((t1 - t0) * 1e3)
                t_host.append((t2 - t1) * 1e3)
        series.append((B, median(t_dev), median(t_host)))
        say(f"crossover  B {B:5d}:  device call + total on the host {fmt(t_dev)}   host loop {fmt(t_host)}")
    below = [B for B, dev, host in series if dev < host]
    say(f"the device tally's median first drops below the host loop's at B = {below[0] if below else 'no measured B'} of {[B for B, _, _ in series]}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

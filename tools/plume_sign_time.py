#!/usr/bin/env python3
"""What signing a population of PLUME voters costs on the device (DESIGN.md sections 4b and 9, profiles/r20_plume_sign.txt).  One process, REPS
repetitions after one warm repetition of every size, the sides taken in turn, medians (minimum in brackets), wall ms; every device region ends
with a device synchronise.

  sign      plume.sign_many_device over B DISTINCT voters, B = 1, 2, 4 .. 2^16: sk and r are seeded 255-bit draws made on the device (below n,
            and zero with probability 2^-255).  The first HOST_SAMPLE voters are compared with `gen_native` on the first repetition.
  sign'     the same call again in the same repetition (A/A): the spread between the two medians is the margin of every ratio below.
  +status   sign, then the status tensor read back to the host (`.status.cpu()`): what a caller waits for.
  verify    plume.verify_many_device over the batch just signed; its report is compared with 0 failures on the first repetition.
  lincomb   plume.lincomb_device over B random 256-bit scalar pairs and the signed batch's pk and nullifier.
  host      `gen_native` on one core over the first HOST_SAMPLE voters of the batch, SCALED to B (labelled): the only way to sign before the
            device call existed.
  ratio     sign / (verify + lincomb): a signature is the verifier's chain plus one more ladder.

Usage: plume_sign_time.py [--reps 7] [--quick] [--out profiles/r20_plume_sign.txt]      (--quick: B up to 64, a rehearsal)"""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from zksnap_circuits_halo2_amd import plume as PL  # noqa: E402

median = statistics.median
HOST_SAMPLE = 4
MSG = bytes([1, 0])


def fmt(xs):
    return f"{median(xs):9.3f} ({min(xs):.3f})"


def main():
    argv, reps = sys.argv[1:], 7
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    quick = "--quick" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(os.path.dirname(HERE), "profiles", "r20_plume_sign.txt")
    import torch

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def sync():
        torch.cuda.synchronize()

    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)

    def words(B, top):
        t = torch.randint(-(1 << 63), (1 << 63) - 1, (B, 4), dtype=torch.int64, device="cuda", generator=gen)
        if top:                                                # clear bit 255: the value is below 2^255 < n
            t[:, 3] &= (1 << 63) - 1
        return t

    say(f"PLUME signing, {torch.cuda.get_device_name(0)}: median of {reps} (min) in ms after one warm repetition, sides in turn; msg = 01 00; "
        f"every voter of a batch distinct (seeded 255-bit sk and r)")
    series = []
    for B in [1 << k for k in range(0, 7 if quick else 17)]:
        sk, r = words(B, True), words(B, True)
        a, b = words(B, False), words(B, False)
        hb = min(B, HOST_SAMPLE)
        sk_host, r_host = PL.decode_scalars(sk[:hb]), PL.decode_scalars(r[:hb])
        t_sign, t_again, t_read, t_ver, t_lin, t_host = [], [], [], [], [], []
        for rep in range(reps + 1):
            sync()
            t0 = time.perf_counter()
            sig = PL.sign_many_device(MSG, sk, r)
            sync()
            t1 = time.perf_counter()
            found = PL.verify_many_device(MSG, sig.pk, sig.nullifier, sig.s, sig.c)
            sync()
            t2 = time.perf_counter()
            out, l_status = PL.lincomb_device(a, sig.pk, b, sig.nullifier)
            sync()
            t3 = time.perf_counter()
            again = PL.sign_many_device(MSG, sk, r)
            sync()
            t4 = time.perf_counter()
            status = PL.sign_many_device(MSG, sk, r).status.cpu()
            t5 = time.perf_counter()
            made = [PL.gen_native(x, MSG, y) for x, y in zip(sk_host, r_host)]
            t6 = time.perf_counter()
            if rep == 0:
                got = list(zip(PL.decode_points(sig.pk[:hb]), PL.decode_points(sig.nullifier[:hb]), PL.decode_scalars(sig.s[:hb]), PL.decode_scalars(sig.c[:hb])))
                assert got == made, "device and host signatures differ"
                assert found.failures == 0 and not status.any().item() and not l_status.any().item(), "a signed voter was refused"
                assert all(torch.equal(x, y) for x, y in ((sig.pk, again.pk), (sig.nullifier, again.nullifier), (sig.s, again.s), (sig.c, again.c)))
            else:
                t_sign.append((t1 - t0) * 1e3)
                t_ver.append((t2 - t1) * 1e3)
                t_lin.append((t3 - t2) * 1e3)
                t_again.append((t4 - t3) * 1e3)
                t_read.append((t5 - t4) * 1e3)
                t_host.append((t6 - t5) * 1e3 * B / hb)
        sign, again_ms, ver, lin, host = median(t_sign), median(t_again), median(t_ver), median(t_lin), median(t_host)
        spread = abs(sign - again_ms) / min(sign, again_ms)
        series.append((B, median(t_read), host, sign / (ver + lin), spread))
        say(f"B {B:6d}:  sign {fmt(t_sign)}   sign' {fmt(t_again)}   A/A spread {100 * spread:5.2f} %   sign + status read back {fmt(t_read)}   verify {fmt(t_ver)}   "
            f"lincomb {fmt(t_lin)}   sign / (verify + lincomb) {sign / (ver + lin):6.3f}   host gen_native {fmt(t_host)}"
            f"{'' if hb == B else f' [{hb} timed, SCALED by {B // hb}]'}   host / device {host / sign:9.1f}   device per voter {sign * 1e3 / B:9.2f} us")
    above = [B for B, dev, host, _, _ in series if B >= 32 and dev >= host]
    say(f"(a) sign + status read back is below the one-core host gen_native loop at every measured B >= 32: {'yes' if not above else 'NO, not at B = ' + str(above)}")
    over = [(B, ratio, spread) for B, _, _, ratio, spread in series if ratio > 1 + spread]
    say("(b) sign / (verify + lincomb) above 1 by more than the A/A spread of its own row: " + (", ".join(f"B = {B} ({ratio:.3f}, spread {100 * spread:.2f} %)" for B, ratio, spread in over) or "nowhere"))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

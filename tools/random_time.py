#!/usr/bin/env python3
"""Random field elements drawn in HBM against what a host had to do before the calls existed, using only calls it had then.

  whole column   zkhip_fr_random_device (n = 2^22, 2^24)           against  zkhip_upload of a READY host column of the same bytes (pageable memory,
                 as a Rust Vec is).  The host's time to draw the column is left out, which flatters the upload.
  rows form      zkhip_fr_random_rows_device, 5 rows of every      against  that many zkhip_upload calls of 160 bytes, one per column
                 column: (k = 13, 270 columns), (k = 15, 947)

One process, clocks warmed first, 9 alternating repetitions, medians; every timed region ends in a synchronise.  The new call against itself
(A/A) puts the noise on the page.  The fill's bytes over its call time are also given as a share of the HBM peak (8.0 TB/s spec, 6.29 TB/s
measured copy rate); the kernel's own time comes from a run under `rocprofv3 --kernel-trace --stats` with --profile (fills only, no timing).
    python tools/random_time.py [--reps 9] [--profile] [--flow]
--flow adds tools/prove_flow.py at k = 22 and k = 13 (256 gate columns, 8 lookups), with and without device_randomness, three warm proofs a side.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import numpy as np
import torch

from zksnap_circuits_halo2_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--flow", action="store_true")
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
SEED = (C.c_uint8 * 32)(*range(32))
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def fmt(ts):
    return f"min {min(ts):.3f} median {statistics.median(ts):.3f} max {max(ts):.3f}"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def compare(title, sides, warm_s=1.5):
    """sides: name -> callable, the first is the new call and the second the parent's path; returns the medians"""
    t_end = time.perf_counter() + warm_s                      # clock ramp: profiles/r03_clock_ramp.txt
    while time.perf_counter() < t_end:
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name in sides}
    for _ in range(args.reps):
        for name, fn in sides.items():
            res[name].append(timed(fn))
    med = {name: statistics.median(v) for name, v in res.items()}
    print(f"{title} ({args.reps} alternating repetitions, wall ms incl. launches, each ending in a synchronise)")
    for name, v in res.items():
        print(f"    {name:34s} {fmt(v)}")
    new, parent, aa = list(sides)[:3]
    spread = abs(med[new] - med[aa])
    print(f"    new / parent = {med[new] / med[parent]:.4f} ({med[parent] / med[new]:.1f}x), A/A spread {spread:.3f} ms -> "
          f"{'the new call wins' if med[new] < med[parent] else 'THE PARENT PATH WINS'}", flush=True)
    return med


if args.profile:                                              # under rocprofv3 --kernel-trace --stats: the kernels alone
    for k in (22, 24):
        out = torch.empty((1 << k, 4), dtype=torch.int64, device=dev)
        for _ in range(20):
            _lib.check(lib.zkhip_fr_random_device(SEED, 0, 0, 1 << k, out.data_ptr(), None))
        torch.cuda.synchronize()
    cols = torch.empty((947, 1 << 15, 4), dtype=torch.int64, device=dev)
    ptrs = (C.c_void_p * 947)(*[cols[c].data_ptr() for c in range(947)])
    for _ in range(20):
        _lib.check(lib.zkhip_fr_random_rows_device(SEED, 0, 0, ptrs, 947, (1 << 15) - 5, 5, None))
    torch.cuda.synchronize()
    print("profile run done", flush=True)
    sys.exit(0)

# ---- whole-column fill ------------------------------------------------------------------------------------------------------------------
for k in (22, 24):
    n = 1 << k
    out = torch.empty((n, 4), dtype=torch.int64, device=dev)
    up = torch.empty((n, 4), dtype=torch.int64, device=dev)
    host = np.random.default_rng(k).integers(0, 1 << 61, size=(n, 4), dtype=np.uint64)     # a ready column in pageable memory

    def fill():
        _lib.check(lib.zkhip_fr_random_device(SEED, 0, 0, n, out.data_ptr(), None))

    def upload():
        _lib.check(lib.zkhip_upload(up.data_ptr(), host.ctypes.data, n * 32))

    med = compare(f"whole column, n = 2^{k} ({n * 32 >> 20} MiB)", {"zkhip_fr_random_device": fill, "zkhip_upload of a ready column": upload,
                                                                   "zkhip_fr_random_device (A/A)": fill})
    rate = n * 32 / (med["zkhip_fr_random_device"] * 1e-3)
    print(f"    fill: {rate / 1e9:.1f} GB/s written over the call's wall time = {100 * rate / HBM_SPEC:.1f} % of the 8.0 TB/s spec, "
          f"{100 * rate / HBM_COPY:.1f} % of the 6.29 TB/s measured copy rate (the kernel is bound by its arithmetic, not by its stores)", flush=True)
    del out, up, host

# ---- rows form --------------------------------------------------------------------------------------------------------------------------
for k, n_cols in ((13, 270), (15, 947)):
    n, count = 1 << k, 5
    row0 = n - count
    cols = torch.zeros((n_cols, n, 4), dtype=torch.int64, device=dev)
    ptrs = (C.c_void_p * n_cols)(*[cols[c].data_ptr() for c in range(n_cols)])
    tails = np.random.default_rng(k).integers(0, 1 << 61, size=(n_cols, count, 4), dtype=np.uint64)
    dst = [cols[c].data_ptr() + row0 * 32 for c in range(n_cols)]
    src = [tails[c].ctypes.data for c in range(n_cols)]

    def rows_call():
        _lib.check(lib.zkhip_fr_random_rows_device(SEED, 0, 0, ptrs, n_cols, row0, count, None))

    def uploads():
        for c in range(n_cols):
            _lib.check(lib.zkhip_upload(dst[c], src[c], count * 32))

    compare(f"blinding rows, k = {k}, {n_cols} columns x {count} rows", {"zkhip_fr_random_rows_device": rows_call, f"{n_cols} zkhip_upload calls of 160 bytes": uploads,
                                                                         "zkhip_fr_random_rows_device (A/A)": rows_call})
    del cols

if args.flow:
    import prove_flow

    for (k, g, l) in ((22, 4, 1), (13, 256, 8)):
        prove_flow.run(k, g, lookups=l, verbose=False)                                       # warm: code objects, plans, scratch
        prove_flow.run(k, g, lookups=l, verbose=False, device_randomness=True)
        laps = {False: [], True: []}
        extra = []
        for rep in range(3):
            for on in (False, True):
                r = prove_flow.run(k, g, lookups=l, verbose=False, device_randomness=on)
                assert all(r["checks"].values())
                laps[on].append(r["prove_ms"])
                if on:
                    extra.append(r["timings_ms"]["vanishing_random_poly"])
        print(f"prove_flow.run({k}, {g}, lookups={l}) prover steps, 3 warm alternating proofs a side: default {fmt(laps[False])}; device_randomness "
              f"{fmt(laps[True])} (of which the added lap vanishing_random_poly, fill + commit: {fmt(extra)})", flush=True)

#!/usr/bin/env python3
"""Division by a point set's vanishing polynomial: the fold of `zkhip_fr_kate_division_device` as the multi-open provers ran it (m one-element
`sub_const_at` row programs, then per root one division and one `zero_at` row program) against one `zkhip_fr_divide_by_roots_device`.

Same process, same buffers, interleaved repetitions, clocks warmed first; an A/A pair of the fold against itself puts the noise on the page.
    python tools/divide_by_roots_time.py [--reps 7] [--logs 22,24] [--ms 1,2,3,4,6]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch

from zksnap_circuits_halo2_amd import _lib, fields as F
from zksnap_circuits_halo2_amd.multiopen import _sub_const_at, _zero_at

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--logs", default="22,24")
ap.add_argument("--ms", default="1,2,3,4,6")
args = ap.parse_args()
lib = _lib.load()
rng = np.random.default_rng(8)


def fr_random(n):
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, 0x30644E72E131A029, size=n, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).cuda()


def fmt(ts):
    return f"min {min(ts):.3f} median {statistics.median(ts):.3f} max {max(ts):.3f}"


for log_n in [int(x) for x in args.logs.split(",")]:
    n = 1 << log_n
    a, b0, b1 = fr_random(n), torch.empty((n, 4), dtype=torch.int64, device="cuda"), torch.empty((n, 4), dtype=torch.int64, device="cuda")
    for m in [int(x) for x in args.ms.split(",")]:
        points = [int.from_bytes(rng.bytes(40), "little") % F.R_MOD for _ in range(m)]
        words = F.fr_encode(points)
        low = [int.from_bytes(rng.bytes(40), "little") % F.R_MOD for _ in range(m)]

        def fold():
            # what ProverSHPLONK ran per rotation set before the one-pass routine: patch the m low coefficients, then m x (division, zero the top)
            for t, val in enumerate(low):
                _sub_const_at(a.data_ptr(), t, val, 0)
            src, dst = a, b0
            for i in range(m):
                _lib.check(lib.zkhip_fr_kate_division_device(src.data_ptr(), n, words[i].ctypes.data, dst.data_ptr(), None))
                _zero_at(dst.data_ptr(), n - 1, 0)
                src, dst = dst, (b1 if dst is b0 else b0)

        def one_pass():
            _lib.check(lib.zkhip_fr_divide_by_roots_device(a.data_ptr(), n, words.ctypes.data, m, b0.data_ptr(), None, None))

        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        t_end = time.perf_counter() + 1.5                           # clock ramp: profiles/r03_clock_ramp.txt
        while time.perf_counter() < t_end:
            fold()
            one_pass()
        torch.cuda.synchronize()
        res = {"fold": [], "fold (A/A)": [], "one pass": []}
        for _ in range(args.reps):
            res["fold"].append(timed(fold))
            res["one pass"].append(timed(one_pass))
            res["fold (A/A)"].append(timed(fold))
        med = {k: statistics.median(v) for k, v in res.items()}
        spread = abs(med["fold"] - med["fold (A/A)"])
        print(f"2^{log_n} m={m} ({args.reps} interleaved repetitions, wall ms incl. launches): " + "; ".join(f"{k}: {fmt(v)}" for k, v in res.items())
              + f" | one pass / fold = {med['one pass'] / med['fold']:.3f}, A/A spread {spread:.3f} ms, gain {med['fold'] - med['one pass']:.3f} ms", flush=True)

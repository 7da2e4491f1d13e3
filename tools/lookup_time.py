#!/usr/bin/env python3
"""The lookup argument of L range lookups against one table: the per-lookup loop (`zkhip_lookup_permute_device`, a numerator and a denominator row
program, `zkhip_fr_grand_product_device`, L times) against the two calls that take every lookup at once (`zkhip_lookup_permute_many_device`,
`zkhip_lookup_products_device`).

Same process, same buffers, interleaved repetitions, clocks warmed first, medians; the loop against itself (A/A) puts the noise on the page.  The two
halves of both sides (permute / products) are also timed on their own.
    python tools/lookup_time.py [--reps 9] [--shapes 13:8,15:8,15:11,18:4,22:1] [--flow]
--flow adds the `lookup_permute_and_product` lap of tools/prove_flow.py at run(13, 256, lookups=8) and run(15, 64, lookups=8), keyword off and on.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import torch

from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F
from zksnap_circuits_halo2_amd.tensors import fr_from_small as small_ints

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--shapes", default="13:8,15:8,15:11,18:4,22:1")
ap.add_argument("--bits", type=int, default=8)
ap.add_argument("--flow", action="store_true")
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
R = F.R_MOD
BETA, GAMMA, THETA = 0xB17A % R, (1 << 201) + 5, 3
torch.manual_seed(9)


def fmt(ts):
    return f"min {min(ts):.3f} median {statistics.median(ts):.3f} max {max(ts):.3f}"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


pn, pd = E.lookup_product_programs(1, 1, BETA, GAMMA, THETA)
for shape in args.shapes.split(","):
    k, L = (int(x) for x in shape.split(":"))
    n, u = 1 << k, (1 << k) - 6
    bits = min(args.bits, k - 1)
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    table = small_ints(rows % (1 << bits), k)
    inputs = []
    for _ in range(L):                                   # a witness column: values of the range, padded with zeros
        v = torch.randint(0, 1 << bits, (n,), dtype=torch.int64, device=dev)
        v[torch.rand(n, device=dev) < 0.4] = 0
        inputs.append(small_ints(v, k))
    pa1, ps1, z1, den1 = (torch.zeros((L, n, 4), dtype=torch.int64, device=dev) for _ in range(4))
    pa2, ps2, z2 = (torch.zeros((L, n, 4), dtype=torch.int64, device=dev) for _ in range(3))
    tabs = [table] * L

    def loop_permute():
        for l in range(L):
            _lib.check(lib.zkhip_lookup_permute_device(inputs[l].data_ptr(), table.data_ptr(), u, pa1[l].data_ptr(), ps1[l].data_ptr(), None))

    def loop_products():
        for l in range(L):
            pn.run_device([inputs[l].data_ptr(), table.data_ptr()], k, z1[l].data_ptr())
            pd.run_device([pa1[l].data_ptr(), ps1[l].data_ptr()], k, den1[l].data_ptr())
            _lib.check(lib.zkhip_fr_grand_product_device(z1[l].data_ptr(), den1[l].data_ptr(), n, z1[l].data_ptr(), None))

    def loop():                                          # the parent's sequence, lookup by lookup
        for l in range(L):
            _lib.check(lib.zkhip_lookup_permute_device(inputs[l].data_ptr(), table.data_ptr(), u, pa1[l].data_ptr(), ps1[l].data_ptr(), None))
            pn.run_device([inputs[l].data_ptr(), table.data_ptr()], k, z1[l].data_ptr())
            pd.run_device([pa1[l].data_ptr(), ps1[l].data_ptr()], k, den1[l].data_ptr())
            _lib.check(lib.zkhip_fr_grand_product_device(z1[l].data_ptr(), den1[l].data_ptr(), n, z1[l].data_ptr(), None))

    def one_permute():
        E.permute_expression_pairs_device(inputs, tabs, u, k, pa2, ps2)

    def one_products():
        E.lookup_products_device(inputs, tabs, pa2, ps2, u, k, BETA, GAMMA, z=z2)

    def one_call():
        one_permute()
        one_products()

    t_end = time.perf_counter() + 1.5                     # clock ramp: profiles/r03_clock_ramp.txt
    while time.perf_counter() < t_end:
        loop()
        one_call()
    torch.cuda.synchronize()
    assert torch.equal(pa1[:, :u], pa2[:, :u]) and torch.equal(ps1[:, :u], ps2[:, :u]) and torch.equal(z1[:, :u + 1], z2[:, :u + 1]), "the two sides differ"
    sides = {"loop": loop, "one call": one_call, "loop (A/A)": loop, "loop permute": loop_permute, "one-call permute": one_permute,
             "loop products": loop_products, "one-call products": one_products}
    res = {name: [] for name in sides}
    for _ in range(args.reps):
        for name, fn in sides.items():
            res[name].append(timed(fn))
    med = {name: statistics.median(v) for name, v in res.items()}
    spread = abs(med["loop"] - med["loop (A/A)"])
    print(f"k={k} L={L} ({args.reps} interleaved repetitions, wall ms incl. launches and host waits)")
    for name, v in res.items():
        print(f"    {name:18s} {fmt(v)}")
    gain = med["loop"] - med["one call"]
    print(f"    one call / loop = {med['one call'] / med['loop']:.3f}, gain {gain:.3f} ms, A/A spread {spread:.3f} ms -> "
          f"{'one call wins' if gain > spread else ('loop wins' if -gain > spread else 'within the spread')}", flush=True)

if args.flow:
    import prove_flow

    for (k, g) in ((13, 256), (15, 64)):
        laps = {False: [], True: []}
        for rep in range(3):
            for on in (False, True):
                r = prove_flow.run(k, g, lookups=8, verbose=False, lookups_one_call=on)
                assert all(r["checks"].values())
                laps[on].append(r["timings_ms"]["lookup_permute_and_product"])
        print(f"prove_flow.run({k}, {g}, lookups=8) lap lookup_permute_and_product, 3 interleaved runs each: loop {fmt(laps[False])}; one call {fmt(laps[True])}", flush=True)

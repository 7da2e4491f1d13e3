#!/usr/bin/env python3
"""What Poseidon costs (DESIGN.md sections 4b and 9, profiles/r15_poseidon.txt).  One process per section, alternating repetitions, medians;
every timed region ends with a value on the host.

  tree      Merkle trees of 2^16 and 2^20 leaves through zkhip_poseidon_merkle_device (the region ends with the root on the host) against the
            library's own host form on one core over the same leaves: node by node through zkhip_poseidon_hash, whole for 2^16, the first
            HOST_NODES nodes of level 1 for 2^20 (the host's time per node does not depend on the tree; --host-full hashes all of them).
            The roots are compared.  Then the device time per field product beside the 9 x 29-bit product's own time.
  host      microseconds per permutation of the host form (zkhip_poseidon_permute over 1000 states).
  flow      the `transcript` lap and `prove_ms` of tools/prove_flow.py under Poseidon beside Blake2b, SHPLONK both, at (K, G, L).
  dispatch  `prove_ms` of run(transcript=True) on this tree against ANOTHER checkout (the parent commit, built), process by process in turn:
            ROUNDS rounds of (other, this), each process one warm run and RUNS timed ones, its median taken.  The condition: the medians of
            the two sides differ by no more than the other side's own spread over its rounds.

Usage: poseidon_time.py tree [--host-full] | host | flow K G L | dispatch OTHER_ROOT [K G L] | flow-ms ROOT K G L RUNS     [--reps 9]"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCTS_PER_PERMUTATION = 8 * 18 + 57 * 12          # x^5 is three products a word, the matrix nine a round
PRODUCT_NS = (431.6, 570.6)                          # profiles/r05_fp64_field.txt: ns per wave-multiplication per SIMD, best and worst row of the 9 x 29-bit product
HOST_NODES = 1 << 14
median = statistics.median


def flow_ms(root, k, g, lk, runs):
    """prove_ms of `runs` transcript=True flows of the checkout at `root`, after one warm run; prints them as JSON"""
    sys.path.insert(0, os.path.join(root, "tools"))
    import prove_flow

    prove_flow.run(k, g, lookups=lk, verbose=False, transcript=True)
    print(json.dumps([prove_flow.run(k, g, lookups=lk, verbose=False, transcript=True)["prove_ms"] for _ in range(runs)]))


def dispatch(other, k, g, lk, rounds=5, runs=5):
    this = os.path.dirname(HERE)
    meds = {other: [], this: []}
    for _ in range(rounds):
        for root in (other, this):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "flow-ms", root, str(k), str(g), str(lk), str(runs)], capture_output=True, text=True,
                                 timeout=600, check=True).stdout
            meds[root].append(median(json.loads(out.strip().splitlines()[-1])))
    a, b = meds[other], meds[this]
    spread = max(a) - min(a)
    diff = abs(median(a) - median(b))
    print(f"dispatch ({k}, {g}, {lk}), prove_ms of run(transcript=True), median of {runs} per process, {rounds} processes a side in turn:")
    print(f"  other  {' '.join(f'{v:.2f}' for v in a)}   median {median(a):.2f}  spread (max - min) {spread:.2f}")
    print(f"  this   {' '.join(f'{v:.2f}' for v in b)}   median {median(b):.2f}")
    print(f"  |difference of the medians| {diff:.2f} ms  {'<=' if diff <= spread else '>'}  the other side's own spread {spread:.2f} ms: {'holds' if diff <= spread else 'DOES NOT HOLD'}")
    return diff <= spread


def main():
    argv, reps = sys.argv[1:], 9
    if "--reps" in argv:
        at = argv.index("--reps")
        reps = int(argv[at + 1])
        del argv[at:at + 2]
    args = [a for a in argv if not a.startswith("--")]
    what = args[0] if args else "tree"
    if what == "flow-ms":
        return flow_ms(args[1], *(int(a) for a in args[2:6]))
    if what == "dispatch":
        shape = tuple(int(a) for a in args[2:5]) if len(args) >= 5 else (13, 256, 8)
        sys.exit(0 if dispatch(os.path.abspath(args[1]), *shape) else 1)

    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import numpy as np

    from zksnap_circuits_halo2_amd import _lib, fields as F, poseidon as PS

    lib = _lib.load()
    if what == "host":
        states = F.fr_encode(list(range(1, 3001)))
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _lib.check(lib.zkhip_poseidon_permute(states.ctypes.data, 1000))
            times.append((time.perf_counter() - t0) * 1e3)
        print(f"host permutation: {median(times):.2f} us per permutation (median of {reps} x 1000), {median(times) * 1e3 / PRODUCTS_PER_PERMUTATION:.1f} ns per field product")
        return

    import torch

    if what == "flow":
        import prove_flow

        k, g, lk = (int(a) for a in args[1:4])
        kinds = {"blake2b": True, "poseidon": "poseidon"}
        laps, prove = {n: [] for n in kinds}, {n: [] for n in kinds}
        prove_flow.run(k, g, lookups=lk, verbose=False, transcript="poseidon")      # warm: tables, scratch, compiled programs
        for _ in range(reps):
            for name, tr in kinds.items():
                res = prove_flow.run(k, g, lookups=lk, verbose=False, transcript=tr)
                laps[name].append(res["timings_ms"]["transcript"])
                prove[name].append(res["prove_ms"])
        absorbed = 2 * (res["proof_bytes"] // 32 - len(res["proof_plan"])) + len(res["proof_plan"]) + 1
        print(f"flow ({k}, {g}, {lk}), SHPLONK, median of {reps}: `transcript` laps blake2b {median(laps['blake2b']):.2f} ms  poseidon {median(laps['poseidon']):.2f} ms;  "
              f"prove_ms blake2b {median(prove['blake2b']):.2f}  poseidon {median(prove['poseidon']):.2f};  proof {res['proof_bytes']} bytes, {absorbed} absorbed elements")
        return

    # tree: the two sizes in turn, repetition by repetition
    rng = np.random.default_rng(15)
    sizes = (16, 20)
    h_leaves = {L: rng.integers(0, 1 << 61, size=(1 << L, 4), dtype=np.int64) for L in sizes}      # four words below 2^61 are a Montgomery Fr below r
    d_all = {L: torch.from_numpy(h_leaves[L]).to("cuda") for L in sizes}
    times, roots = {L: [] for L in sizes}, {}
    for L in sizes:
        PS.merkle_device(d_all[L])
    for _ in range(reps):
        for L in sizes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            roots[L] = PS.merkle_device(d_all[L])[-1].cpu().numpy()
            times[L].append((time.perf_counter() - t0) * 1e3)
    # level 1 of the larger tree as one flat launch of zkhip_poseidon_hash_many_device: the kernels' rate with every lane busy and nothing handed on
    pairs = d_all[20].reshape(1 << 19, 2, 4)
    flat = []
    PS.hash_many_device(pairs)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        PS.hash_many_device(pairs)[-1].cpu()
        flat.append((time.perf_counter() - t0) * 1e3)
    flat_ns = median(flat) * 1e6 / ((1 << 19) * 2 * PRODUCTS_PER_PERMUTATION / 64 / 1024)
    print(f"hash_many 2^19 x 2 (level 1 of the 2^20 tree, flat): {median(flat):.3f} ms (median of {reps}) = {flat_ns:.0f} ns per wave-product per SIMD")
    for log_n in sizes:
        n, leaves, dev, root = 1 << log_n, h_leaves[log_n], times[log_n], roots[log_n]
        # the host form, one core: level by level, children side by side in memory
        full = log_n <= 16 or "--host-full" in sys.argv
        level = np.ascontiguousarray(leaves.view(np.uint64))
        t0 = time.perf_counter()
        host_nodes = 0
        while len(level) > 1 and (full or host_nodes == 0):
            count = len(level) // 2 if full else HOST_NODES
            up = np.zeros((count, 4), dtype=np.uint64)
            src, dst = level.ctypes.data, up.ctypes.data
            for i in range(count):
                lib.zkhip_poseidon_hash(src + 64 * i, 2, dst + 32 * i)
            host_nodes += count
            level = up
        host_ms = (time.perf_counter() - t0) * 1e3
        per_node_us = host_ms * 1e3 / host_nodes
        if full:
            assert np.array_equal(level[0], root.view(np.uint64)), "host and device roots differ"
        d = median(dev)
        products = (n - 1) * 2 * PRODUCTS_PER_PERMUTATION
        # all lanes busy: 1024 SIMDs x 64 lanes; the time of one wave-product per SIMD that the tree's rate amounts to
        wave_product_ns = d * 1e6 / (products / 64 / 1024)
        print(f"tree 2^{log_n}: device {d:.3f} ms (median of {reps}, root on the host; min {min(dev):.3f})  host form {per_node_us:.1f} us per node "
              f"({'all' if full else host_nodes} nodes hashed{', roots equal' if full else ''}) = {per_node_us * (n - 1) / 1e3:.0f} ms for the tree: "
              f"{per_node_us * (n - 1) / 1e3 / d:.0f} x")
        print(f"  {products / 1e6:.0f} M field products: {d * 1e6 / products * 1e3:.2f} ps each over the device = {wave_product_ns:.0f} ns per wave-product per SIMD "
              f"(the 9 x 29-bit product alone: {PRODUCT_NS[0]} .. {PRODUCT_NS[1]} ns, profiles/r05_fp64_field.txt): ratio {wave_product_ns / PRODUCT_NS[0]:.2f} .. {wave_product_ns / PRODUCT_NS[1]:.2f}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a batch of insertions into the indexed Merkle tree costs (DESIGN.md sections 4b and 9, profiles/r16_imt.txt).  One process, REPS
repetitions with the sides taken in turn, medians; every timed region ends with the last root of the batch on the host.

  device   IndexedMerkleTree.insert_batch over B values (Montgomery words, already encoded), then the last root copied to the host.
  host     the strongest way the library offered before the tree object: one insertion after another, the low leaf from a sorted list
           (bisect), the two leaves rehashed and their two paths recomputed node by node through zkhip_poseidon_hash, the same witnesses
           (roots, preimages, both proofs) written into host arrays.  One core.  Run twice, side by side (host and host'), as the A/A figure:
           what two runs of the same code differ by.  At B = 65536 the host sides insert the first 4096 values and the time is SCALED by 16.
  rebuild  (depth 3 and 10 only) the reference's way: the whole tree rebuilt twice per insertion -- hash_many_device over all preimages and
           MerkleTree over the leaves -- with the proofs and roots read from the rebuilt trees.

Where device and host start from the same tree and insert the same values, their last roots are compared.

Usage: imt_time.py [--reps 9] [--quick]      (--quick: small sizes only, a rehearsal)"""
import bisect
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from zksnap_circuits_halo2_amd import _lib, fields as F, poseidon as PS  # noqa: E402

median = statistics.median
HOST_SAMPLE = 4096
HASH_LATENCY_MS = 0.64                                   # profiles/r15_poseidon.txt: one level of a tree, one lane's hash


class HostTree:
    """the tree in host arrays, updated one insertion at a time with the library's host hash"""

    def __init__(self, depth, lib):
        self.depth, self.lib, self.n = depth, lib, 1 << depth
        z = np.zeros(12, dtype=np.uint64)
        h = np.zeros(4, dtype=np.uint64)
        lib.zkhip_poseidon_hash(z.ctypes.data, 3, h.ctypes.data)
        self.levels = []
        for L in range(depth + 1):
            self.levels.append(np.tile(h, (self.n >> L, 1)))
            pair = np.concatenate([h, h])
            lib.zkhip_poseidon_hash(pair.ctypes.data, 2, h.ctypes.data)
        self.base = [lv.ctypes.data for lv in self.levels]
        self.pre = np.zeros((self.n, 3, 4), dtype=np.uint64)
        self.pre_base = self.pre.ctypes.data
        self.sorted_vals, self.sorted_idx, self.used = [0], [0], 1

    def _rehash(self, i):
        hash_, base = self.lib.zkhip_poseidon_hash, self.base
        hash_(self.pre_base + 96 * i, 3, base[0] + 32 * i)
        for L in range(self.depth):
            i >>= 1
            hash_(base[L] + 64 * i, 2, base[L + 1] + 32 * i)

    def insert_batch(self, words, canon, out):
        """words: (B, 4) Montgomery; canon: their integers; out: (roots, low_leaves, new_leaves, low_indices, low_proofs, new_proofs) host arrays"""
        roots, low_leaves, new_leaves, low_indices, low_proofs, new_proofs = out
        levels, depth, pre = self.levels, self.depth, self.pre
        roots[0] = levels[depth][0]
        for i in range(len(words)):
            v, j = canon[i], self.used
            at = bisect.bisect_left(self.sorted_vals, v)
            low = self.sorted_idx[at - 1]
            low_leaves[i] = pre[low]
            low_indices[i] = low
            for L in range(depth):
                low_proofs[i, L] = levels[L][(low >> L) ^ 1]
            pre[j, 0] = words[i]
            pre[j, 1:] = pre[low, 1:]
            pre[low, 1] = words[i]
            pre[low, 2] = F.fr_encode([j])[0]
            self._rehash(low)
            for L in range(depth):
                new_proofs[i, L] = levels[L][(j >> L) ^ 1]
            new_leaves[i] = pre[j]
            self._rehash(j)
            roots[i + 1] = levels[depth][0]
            self.sorted_vals.insert(at, v)
            self.sorted_idx.insert(at, j)
            self.used += 1
        return roots[len(words)].copy()


def host_out(b, depth):
    u = np.uint64
    return (np.zeros((b + 1, 4), u), np.zeros((b, 3, 4), u), np.zeros((b, 3, 4), u), np.zeros(b, np.uint32), np.zeros((b, depth, 4), u), np.zeros((b, depth, 4), u))


def rebuild_batch(words, canon, depth):
    """the reference's way over the device calls the library had: two whole-tree rebuilds per insertion, proofs and roots read from them"""
    import torch

    n = 1 << depth
    pre = torch.zeros((n, 3, 4), dtype=torch.int64, device="cuda")
    tree = PS.MerkleTree(PS.hash_many_device(pre))
    vals, idx = [0], [0]
    root = None
    for i in range(len(words)):
        v, j = canon[i], len(vals)
        at = bisect.bisect_left(vals, v)
        low = idx[at - 1]
        tree.get_root(), tree.get_proof(low)
        w = torch.from_numpy(words[i].view(np.int64)).to("cuda")
        pre[j, 0] = 0
        pre[j, 1:] = pre[low, 1:]                                   # the new leaf's links, parked: its val stays 0 until the second rebuild
        pre[low, 1] = w
        pre[low, 2] = torch.from_numpy(F.fr_encode([j])[0].view(np.int64)).to("cuda")
        keep = pre[j].clone()
        pre[j] = 0
        tree = PS.MerkleTree(PS.hash_many_device(pre))              # the tree with the low leaf updated
        tree.get_proof(j)
        pre[j] = keep
        pre[j, 0] = w
        tree = PS.MerkleTree(PS.hash_many_device(pre))              # and with the new leaf in
        root = tree.get_root()
        vals.insert(at, v)
        idx.insert(at, j)
    return root


def main():
    argv, reps = sys.argv[1:], 9
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    quick = "--quick" in argv
    import torch

    lib = _lib.load()
    rng = np.random.default_rng(16)
    configs = [(3, 7, True), (10, 256, True)] + [(20, b, False) for b in (1, 8, 12, 14, 16, 256, 4096, 65536)]      # 8 .. 14: where the two paths cross
    if quick:
        configs = [(3, 7, True), (10, 16, True), (12, 1, False), (12, 64, False)]
    print(f"indexed Merkle tree, {torch.cuda.get_device_name(0)}: median of {reps} (min) in ms, sides in turn, the last root on the host each time")
    series = []
    for depth, b, with_rebuild in configs:
        fresh = (reps + 1) * b >= (1 << depth)                       # the tree cannot take every repetition's batch: a new tree per repetition
        hb = min(b, HOST_SAMPLE)
        scale = b / hb
        # four words below 2^61 are a reduced Montgomery element; distinct and nonzero (checked by the insert itself)
        batches = [rng.integers(1, 1 << 61, size=(b, 4), dtype=np.int64).view(np.uint64) for _ in range(reps + 1)]
        canons = [F.fr_decode(w[:hb]) for w in batches]
        outs = [host_out(hb, depth), host_out(hb, depth)]
        make = lambda: (PS.IndexedMerkleTree(depth), HostTree(depth, lib), HostTree(depth, lib))       # noqa: E731
        tree, host_a, host_b = make()
        times = {"device": [], "host": [], "host'": [], "rebuild": []}
        for r in range(reps + 1):                                   # repetition 0 warms every side up and is not counted
            if fresh and r:
                tree.close()
                tree, host_a, host_b = make()
            words, canon = batches[r], canons[r]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch = tree.insert_batch(words)
            d_root = batch.roots[-1].cpu().numpy().view(np.uint64)
            t_dev = time.perf_counter() - t0
            roots = []
            t_host = []
            for side, out in ((host_a, outs[0]), (host_b, outs[1])):
                t0 = time.perf_counter()
                roots.append(side.insert_batch(words[:hb], canon, out))
                t_host.append((time.perf_counter() - t0) * scale)
            assert np.array_equal(roots[0], roots[1])
            if hb == b:
                assert np.array_equal(roots[0], d_root), "host and device roots differ"
                assert np.array_equal(outs[0][4], batch.low_proofs.cpu().numpy().view(np.uint64)) and np.array_equal(outs[0][5], batch.new_proofs.cpu().numpy().view(np.uint64))
            if with_rebuild:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rb_root = rebuild_batch(words, canon, depth)
                t_rb = time.perf_counter() - t0
                if fresh:
                    assert rb_root == F.fr_decode(d_root.reshape(1, 4))[0], "rebuild and device roots differ"
            if r:
                times["device"].append(t_dev * 1e3)
                times["host"].append(t_host[0] * 1e3)
                times["host'"].append(t_host[1] * 1e3)
                if with_rebuild:
                    times["rebuild"].append(t_rb * 1e3)
        tree.close()
        dev, host, host2 = median(times["device"]), median(times["host"]), median(times["host'"])
        line = (f"depth {depth:2d}  B {b:5d}:  device {dev:10.3f} ({min(times['device']):.3f})   host {host:11.3f} ({min(times['host']):.3f})"
                f"   host' {host2:11.3f}   A/A |host - host'| {abs(host - host2):.3f}   host / device {host / dev:8.2f}")
        if scale != 1:
            line += f"   [host: {hb} insertions timed, SCALED by {scale:.0f}]"
        if with_rebuild:
            line += f"   rebuild {median(times['rebuild']):.3f} ({min(times['rebuild']):.3f})"
        line += f"   device per launch {dev / (depth + 2):.3f}, per insertion {dev * 1e3 / b:.1f} us; host per insertion {host * 1e3 / b:.1f} us"
        print(line, flush=True)
        if not with_rebuild:
            series.append((depth, b, dev, host))
    if series:
        depth = series[0][0]
        below = [b for _, b, dev, host in series if dev < host]
        print(f"depth {depth}: the device call's median first drops below the host path's at B = {below[0] if below else 'no measured B'} of {[b for _, b, _, _ in series]}")
        small = [dev for _, b, dev, _ in series if 2 * b <= 1024]
        if small:
            print(f"depth {depth}: a batch of at most 512 insertions takes {min(small):.3f} .. {max(small):.3f} ms = {min(small) / (depth + 2):.3f} .. {max(small) / (depth + 2):.3f} ms per launch "
                  f"of its {depth + 2}, beside {HASH_LATENCY_MS} ms for one lane's hash (profiles/r15_poseidon.txt)")
        for _, b, dev, host in series:
            if b >= 4096:
                print(f"depth {depth}, B = {b}: device median {'below' if dev < host else 'NOT below'} the host path's ({dev:.3f} against {host:.3f} ms, {host / dev:.1f} x)")


if __name__ == "__main__":
    main()

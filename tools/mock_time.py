#!/usr/bin/env python3
"""The three witness checks (zkhip_check_rows_device / _copies_ / _lookups_) against what the library offered for the same questions before
they existed, on the witnesses tools/prove_flow.py proves (prover.halo2_lib_witness): (k, gate columns, lookups) = (22, 4, 1), (13, 256, 8), (15, 64, 8).

  gates     zkhip_check_rows_device, every gate polynomial in one launch    against  one zkhip_fr_eval_rows_device per polynomial into a scratch
                                                                                      column, a download and a host scan for a non-zero word
            ... and against zkhip_fr_eval_rows_sum_device on the SAME programs (weights 1): the check does that call's row arithmetic and stores
            nothing, so it must not be slower than it by more than that call's own A/A spread
  copies    zkhip_check_copies_device                                       against  a download of the permutation's columns and numpy
  lookups   zkhip_check_lookups_device                                      against  a download of the input / table columns and numpy

One process, clocks warmed first, 9 alternating repetitions, medians; every timed region ends with the answer on the host (the records read
back, or the host scan done).  Then the flow itself: the `mock_prover` lap beside the prover steps, three warm proofs.  A CPU MockProver
figure -- what the reference pays -- cannot be measured here: there is no Rust toolchain.
    python tools/mock_time.py [--reps 9] [--shapes 22:4:1,13:256:8,15:64:8] [--no-flow]"""
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

import prove_flow
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F, mock as M, prover

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--shapes", default="22:4:1,13:256:8,15:64:8")
ap.add_argument("--no-flow", action="store_true")
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)


def fmt(ts):
    return f"min {min(ts):.3f} median {statistics.median(ts):.3f} max {max(ts):.3f}"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def compare(title, sides, warm_s=1.0):
    """sides: name -> callable, run in turn; returns the medians"""
    t_end = time.perf_counter() + warm_s
    while True:
        for fn in sides.values():
            fn()
        if time.perf_counter() >= t_end:
            break
    res = {name: [] for name in sides}
    for _ in range(args.reps):
        for name, fn in sides.items():
            res[name].append(timed(fn))
    print(f"{title} ({args.reps} alternating repetitions, wall ms, each ending with the answer on the host)")
    for name, v in res.items():
        print(f"    {name:58s} {fmt(v)}")
    return {name: statistics.median(v) for name, v in res.items()}


def verdict(what, new, parent):
    print(f"    {what}: new / parent = {new / parent:.4f} ({parent / new:.1f}x) -> {'the new call wins' if new < parent else 'THE PARENT PATH WINS'}", flush=True)


def all_members(inp, tab):
    """every row of inp ((m, 4) uint64 words) is a row of tab, exactly.  Where the low word tells the table's distinct rows apart it is the search
    key (a sort of 8-byte keys); otherwise the rows are compared as 32-byte records (numpy sorts those ten times slower)"""
    w0, idx = np.unique(tab[:, 0], return_index=True)
    rep = tab[idx]
    if (rep[np.searchsorted(w0, tab[:, 0])] == tab).all():
        pos = np.searchsorted(w0, inp[:, 0])
        pos[pos == len(w0)] = 0
        return bool((rep[pos] == inp).all())
    key = np.dtype([("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("d", "<u8")])
    return bool(np.isin(np.ascontiguousarray(inp).view(key).ravel(), np.unique(np.ascontiguousarray(tab).view(key).ravel())).all())


def measure(cs, k, fixed, advice, assembly, theta):
    n, u = 1 << k, (1 << k) - (cs.blinding_factors + 1)
    columns = list(fixed) + list(advice)
    ptrs = [c.data_ptr() for c in columns]
    progs = M.gate_programs(cs)
    P = len(progs)
    reports = torch.zeros((max(P, len(cs.lookups), 1), 2), dtype=torch.int64, device=dev)
    answer = np.zeros((reports.shape[0], 2), dtype=np.uint64)

    def read(count):
        _lib.check(lib.zkhip_stream_sync(None))
        _lib.check(lib.zkhip_download(answer.ctypes.data, C.c_void_p(reports.data_ptr()), count * 16))
        assert not answer[:count, 0].any(), "the flow's witness is satisfied"

    # ---- gates ----------------------------------------------------------------------------------------------------------------------------
    scratch = torch.empty((n, 4), dtype=torch.int64, device=dev)
    host_col = np.empty((n, 4), dtype=np.uint64)
    total = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ones = [1] * P

    def check_rows():
        M.enqueue_check_rows(progs, ptrs, k, 0, u, reports.data_ptr())
        read(P)

    def eval_download_scan():
        for p in progs:
            p.run_device(ptrs, k, scratch.data_ptr())
            _lib.check(lib.zkhip_download(host_col.ctypes.data, C.c_void_p(scratch.data_ptr()), n * 32))
            assert not host_col[:u].any()

    def rows_sum():
        E.run_programs_sum_device(progs, ones, ptrs, k, total.data_ptr())

    med = compare(f"k = {k}, {P} gate polynomials over {len(columns)} columns, rows [0, {u})",
                  {"zkhip_check_rows_device": check_rows, f"{P} x (eval_rows_device + download + host scan)": eval_download_scan,
                   "zkhip_fr_eval_rows_sum_device, same programs": rows_sum, "zkhip_fr_eval_rows_sum_device (A/A)": rows_sum})
    verdict("gates", med["zkhip_check_rows_device"], med[f"{P} x (eval_rows_device + download + host scan)"])
    s1, s2 = med["zkhip_fr_eval_rows_sum_device, same programs"], med["zkhip_fr_eval_rows_sum_device (A/A)"]
    over = med["zkhip_check_rows_device"] - min(s1, s2)
    print(f"    check - eval_rows_sum = {over:+.3f} ms, eval_rows_sum A/A spread {abs(s1 - s2):.3f} ms -> "
          f"{'within the spread (or faster)' if over <= abs(s1 - s2) else 'ABOVE THE SPREAD'}", flush=True)
    del scratch, total

    # ---- copies ---------------------------------------------------------------------------------------------------------------------------
    qc = E.quotient_columns(cs)
    base = {"fixed": qc.fixed, "advice": qc.advice, "instance": qc.instance}
    perm = [columns[base[kind] + idx] for kind, idx in cs.permutation_columns]
    npc = len(perm)
    mc_h, mr_h = np.ascontiguousarray(assembly.map_col, dtype=np.uint32), np.ascontiguousarray(assembly.map_row, dtype=np.uint32)
    mc = torch.from_numpy(mc_h.view(np.int32)).to(dev)
    mr = torch.from_numpy(mr_h.view(np.int32)).to(dev)
    host_perm = np.empty((npc, n, 4), dtype=np.uint64)
    moved = np.nonzero((mc_h != np.arange(npc, dtype=np.uint32)[:, None]) | (mr_h != np.arange(n, dtype=np.uint32)[None, :]))      # known once per circuit

    def check_copies():
        M.enqueue_check_copies(perm, k, mc.data_ptr(), mr.data_ptr(), reports.data_ptr())
        read(1)

    def download_numpy_copies():
        for c in range(npc):
            _lib.check(lib.zkhip_download(host_perm[c].ctypes.data, C.c_void_p(perm[c].data_ptr()), n * 32))
        assert not (host_perm[moved] != host_perm[mc_h[moved], mr_h[moved]]).any()

    med = compare(f"k = {k}, copy constraints over {npc} columns ({len(moved[0])} cells in cycles)",
                  {"zkhip_check_copies_device": check_copies, f"download of {npc} columns + numpy over the moved cells": download_numpy_copies})
    verdict("copies", *med.values())
    del host_perm

    # ---- lookups --------------------------------------------------------------------------------------------------------------------------
    L = len(cs.lookups)
    inputs = [advice[lk.input_expressions[0].a] for lk in cs.lookups]            # the flow's lookups are single columns: compressed = the column
    tables = [fixed[lk.table_expressions[0].a] for lk in cs.lookups]
    host_in, host_tab = np.empty((L, n, 4), dtype=np.uint64), np.empty((n, 4), dtype=np.uint64)

    def check_lookups():
        M.enqueue_check_lookups(inputs, tables, k, u, reports.data_ptr())
        read(L)

    def download_numpy_lookups():
        _lib.check(lib.zkhip_download(host_tab.ctypes.data, C.c_void_p(tables[0].data_ptr()), n * 32))                  # one shared table
        for l in range(L):
            _lib.check(lib.zkhip_download(host_in[l].ctypes.data, C.c_void_p(inputs[l].data_ptr()), n * 32))
        assert all_members(host_in[:, :u].reshape(-1, 4), host_tab[:u])

    med = compare(f"k = {k}, {L} lookups against one table, {u} usable rows",
                  {"zkhip_check_lookups_device": check_lookups, f"download of {L} + 1 columns + numpy (unique, searchsorted)": download_numpy_lookups})
    verdict("lookups", *med.values())


for shape in args.shapes.split(","):
    k, g, l = (int(x) for x in shape.split(":"))
    print(f"==== prove_flow shape k = {k}, {g} gate columns, {l} lookups ====", flush=True)
    torch.manual_seed(1)
    w = prover.halo2_lib_witness(k, g, l, prover.TorchBlinding())
    measure(w.cs, k, w.fixed, w.advice, w.assembly, prover.SeededChallenges(1).theta())
    del w
    if args.no_flow:
        continue
    prove_flow.run(k, g, lookups=l, verbose=False, mock=True)                                # warm: code objects, plans, scratch
    laps, proofs = [], []
    for rep in range(3):
        r = prove_flow.run(k, g, lookups=l, verbose=False, mock=True)
        assert all(r["checks"].values())
        laps.append(r["timings_ms"]["mock_prover"])
        proofs.append(r["prove_ms"])
    print(f"prove_flow.run({k}, {g}, lookups={l}, mock=True), 3 warm proofs: lap mock_prover (three checks, buffers, read-back) {fmt(laps)}; prover steps "
          f"{fmt(proofs)}.  No CPU MockProver figure: the reference's cannot be built here.", flush=True)

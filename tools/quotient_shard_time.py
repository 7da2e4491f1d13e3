#!/usr/bin/env python3
"""Measurement only: the quotient numerator sharded by rows (zkhip_fr_eval_rows_sharded_device) on the wrapper shape of
tools/quotient_time.py -- k = 22, extended_k = 24, the proving key's 16 cosets EXTENDED, the proof's 13 columns COEFF -- on one card, in one
process.  Prints
  (a) the current composition: zkhip_coeff_to_extended_device per COEFF column + the whole-domain zkhip_fr_eval_rows_device;
  (b) the sharded entry on one device (S = 1);
  (c) the whole-domain launch against 8 windows of 2^21 rows run one after another (zkhip_fr_eval_rows_window_device), per executor (the
      interpreter in a child process with ZKHIP_VM_JIT=0);
  (d) S = 3 and S = 8 contexts of the same card: wall time (NOT a speed claim: every context is the same card) and the bytes each device
      receives / sends, COMPUTED from the copy plan (exchange_bytes restates it), not counted from the copies the library issues;
  (e) the 8-card projection of the quotient phase at k = 24, from one card's measured transform share and window kernel plus an ASSUMED
      xGMI rate, for both key forms;
  (f) the key as a row-shard set (ZKHIP_COL_ROW_SHARDS): S = 1 against EXTENDED and against the composition, 5 repetitions each,
      interleaved, in this process; S = 3 / 8 wall time on contexts of one card (not a speed claim) and the exchange bytes of both key
      forms from the copy plan;
  (g) the closed-form Lagrange kernel (zkhip_lagrange_cosets_row_shards_device) against the ifft + coeff_to_extended of the three
      indicator columns it replaces, at ext_k = 24.
`quotient_shard_time.py` (everything) | `quotient_shard_time.py windows` (only (c), the executor the environment selects) |
`quotient_shard_time.py rowshards` (only (f) and (g)) | `quotient_shard_time.py keygen` (keygen_device at k = 22 with and without row_shards) |
`quotient_shard_time.py contexts 1 2 8` (the sharded quotient with both key forms and the row-shard scatter / gather on that many contexts of
one card, one line per count: wall time, for comparing two builds of the library, not a speed claim)."""
import ctypes as C
import os
import random
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import zksnap_circuits_halo2_amd as Z  # noqa: E402
from zksnap_circuits_halo2_amd import _lib, evaluation as E, fields as F  # noqa: E402

lib = _lib.load()
LINK_GBPS = 64.0                     # assumed xGMI rate (bench.py's projection assumes the same)
REPS = 5


def wrapper_cs():
    gates = [[E.Fixed(i) * (E.Advice(i, 0) + E.Advice(i, 1) * E.Advice(i, 2) - E.Advice(i, 3))] for i in range(4)]
    lookups = [E.Lookup([E.Advice(4)], [E.Fixed(5)])]
    perm = [("advice", i) for i in range(5)] + [("fixed", 4), ("instance", 0)]
    return E.ConstraintSystem(num_fixed=6, num_advice=5, num_instance=1, gates=gates, lookups=lookups, permutation_columns=perm,
                              blinding_factors=5, degree=4)


cs = wrapper_cs()
qc = E.quotient_columns(cs)
KEY = set(range(qc.fixed, qc.advice)) | {qc.l0, qc.l_last, qc.l_active_row} | set(range(qc.sigma, qc.perm_product))
FORMS = [E.COL_EXTENDED if i in KEY else E.COL_COEFF for i in range(qc.total)]
rng = random.Random(1)
CH = tuple(rng.randrange(F.R_MOD) for _ in range(4))


def rand(rows):
    t = torch.randint(0, 1 << 62, (rows, 4), dtype=torch.int64, device="cuda")
    t[:, 3] &= (1 << 61) - 1
    return t


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def shard_range(n, j, S):
    base, extra = divmod(n, S)
    lo = j * base + min(j, extra)
    return lo, lo + base + (1 if j < extra else 0)


def init(S):
    os.environ["ZKHIP_TEST_DUPLICATE_DEVICES"] = "1"       # S contexts of card 0 (zkhip_init reads it)
    lib.zkhip_shutdown()
    _lib.check(lib.zkhip_init((C.c_int * S)(*([0] * S)), S))


def windows_of(prog, cols, ek, row0, count):
    lo, hi = prog.halos(ek)
    idx = (torch.arange(row0 - lo, row0 + count + hi, device="cuda") % (1 << ek))
    return [c[idx].contiguous() for c in cols]


def whole_vs_windows(prog, ek, parts=8):
    cols = [rand(1 << ek) for _ in range(qc.total)]
    out = torch.zeros((1 << ek, 4), dtype=torch.int64, device="cuda")
    ptrs = [c.data_ptr() for c in cols]
    whole = timed(lambda: prog.run_device(ptrs, ek, out.data_ptr()))
    count = (1 << ek) // parts
    wins = [windows_of(prog, cols, ek, j * count, count) for j in range(parts)]
    wptrs = [[w.data_ptr() for w in ws] for ws in wins]
    out2 = torch.zeros_like(out)

    def run_windows():
        for j in range(parts):
            prog.run_window_device(wptrs[j], ek, j * count, count, out2[j * count:].data_ptr())
    win = timed(run_windows)
    assert torch.equal(out, out2), "windows differ from the whole-domain launch"
    return whole, win


def exchange_bytes(n_cols, n_coeff, k, ek, halo, S, j, key_shards=False):
    """bytes device j receives from other devices: its COEFF columns (pulled from the primary), the window pieces of every column it does
    not hold itself -- with key_shards the key's n_cols - n_coeff columns are already in its own windows -- and (a secondary) nothing more:
    its results leave it (sent bytes: count * 32)"""
    N = 1 << ek
    lo, hi = shard_range(N, j, S)
    W = halo + (hi - lo)
    olo, ohi = shard_range(n_coeff, j, S)
    pulled = (ohi - olo) * (1 << k) * 32 if j else 0
    n_ext = 0 if key_shards else n_cols - n_coeff
    remote_cols = (n_ext if j else 0) + (n_coeff - (ohi - olo))
    return pulled + remote_cols * W * 32, (hi - lo) * 32 if j else 0


def primary_sent_bytes(n_cols, n_coeff, k, ek, halo, S, j, key_shards=False):
    """bytes that leave the primary for device j (j > 0): j's COEFF columns, the windows of the COEFF columns the primary owns and (key
    EXTENDED) the windows of the key's columns"""
    if j == 0:
        return 0
    N = 1 << ek
    lo, hi = shard_range(N, j, S)
    W = halo + (hi - lo)
    olo, ohi = shard_range(n_coeff, j, S)
    own0 = shard_range(n_coeff, 0, S)[1]
    n_ext = 0 if key_shards else n_cols - n_coeff
    return (ohi - olo) * (1 << k) * 32 + (own0 + n_ext) * W * 32


def plan_line(n_cols, n_coeff, k, ek, halo, S):
    """per device received / sent-out-of-the-primary MB for both key forms, COMPUTED from the copy plan"""
    parts = []
    for key in (False, True):
        moved = [(exchange_bytes(n_cols, n_coeff, k, ek, halo, S, j, key)[0], primary_sent_bytes(n_cols, n_coeff, k, ek, halo, S, j, key)) for j in range(S)]
        parts.append(("row-shard key" if key else "EXTENDED key") + ": " + " ".join(f"{a / 2**20:.0f}/{b / 2**20:.0f}" for a, b in moved)
                     + f" (primary sends {sum(b for _, b in moved) / 2**30:.2f} GiB)")
    return "per device received / sent out of the primary MB, COMPUTED from the copy plan -- " + "; ".join(parts)


def main():
    k, ek = 22, 24
    prog = E.evaluate_h_program(cs, k, ek, *CH)
    lo, hi = prog.halos(ek)
    dom = Z.EvaluationDomain(4, k)
    print(f"wrapper shape: k={k} extended_k={ek} columns={qc.total} ({FORMS.count(E.COL_COEFF)} COEFF, {FORMS.count(E.COL_EXTENDED)} EXTENDED) "
          f"insns={len(prog.insns)} halos=({lo}, {hi})  box: {torch.cuda.get_device_name(0)}, one process", flush=True)
    torch.manual_seed(3)
    cols = [rand(1 << (ek if f == E.COL_EXTENDED else k)) for f in FORMS]
    coeff_idx = [i for i, f in enumerate(FORMS) if f == E.COL_COEFF]
    ext = {i: torch.empty((1 << ek, 4), dtype=torch.int64, device="cuda") for i in coeff_idx}
    out_a = torch.zeros((1 << ek, 4), dtype=torch.int64, device="cuda")
    out_b = torch.zeros_like(out_a)
    init(1)

    def composition():
        for i in coeff_idx:
            _lib.check(lib.zkhip_coeff_to_extended_device(cols[i].data_ptr(), 1 << k, k, ext[i].data_ptr(), 1 << ek, ek, 1, dom.extended_omega.ctypes.data,
                                                          dom.g_coset.ctypes.data, None))
        prog.run_device([(ext[i] if i in ext else cols[i]).data_ptr() for i in range(qc.total)], ek, out_a.data_ptr())

    columns = [(c.data_ptr(), f) for c, f in zip(cols, FORMS)]
    sharded = lambda out: E.evaluate_rows_sharded_device(prog, columns, k, ek, dom, out.data_ptr())
    ta = timed(composition)
    tb = timed(lambda: sharded(out_b))
    assert torch.equal(out_a, out_b)
    print(f"(a) composition (13 coeff_to_extended + whole-domain launch)    {ta:8.3f} ms")
    print(f"(b) sharded entry, S = 1                                        {tb:8.3f} ms   (b)/(a) = {tb / ta:.4f}", flush=True)
    del ext
    # (c)
    tw, tn = whole_vs_windows(prog, ek)
    print(f"(c) compiled     : whole-domain 2^{ek} {tw:8.3f} ms   8 windows of 2^{ek - 3} in sequence {tn:8.3f} ms   ratio {tn / tw:.4f}", flush=True)
    env = dict(os.environ, ZKHIP_VM_JIT="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "windows"], capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0:
        raise SystemExit("interpreter child failed: " + r.stdout[-2000:] + r.stderr[-2000:])
    print(r.stdout.strip().replace("(c) compiled     ", "(c) interpreter  "), flush=True)
    # (d)
    nC = len(coeff_idx)
    for S in (3, 8):
        init(S)
        out_d = torch.zeros_like(out_a)
        td = timed(lambda: sharded(out_d))
        assert torch.equal(out_d, out_a), S
        moved = [exchange_bytes(qc.total, nC, k, ek, lo + hi, S, j) for j in range(S)]
        print(f"(d) S = {S} contexts of ONE card: {td:8.3f} ms wall (not a speed claim); per device received / sent MB, COMPUTED from the copy plan: "
              + " ".join(f"{a / 2**20:.0f}/{b / 2**20:.0f}" for a, b in moved), flush=True)
    init(1)
    del cols, out_a, out_b
    torch.cuda.empty_cache()
    # (e) k = 24 on 8 cards
    k8, ek8, S = 24, 26, 8
    prog8 = E.evaluate_h_program(cs, k8, ek8, *CH)
    dom8 = Z.EvaluationDomain(4, k8)
    share = -(-nC // S)
    src = rand(1 << k8)
    dst = torch.empty((share, 1 << ek8, 4), dtype=torch.int64, device="cuda")

    def transforms():
        for b in range(share):
            _lib.check(lib.zkhip_coeff_to_extended_device(src.data_ptr(), 1 << k8, k8, dst[b].data_ptr(), 1 << ek8, ek8, 1, dom8.extended_omega.ctypes.data,
                                                          dom8.g_coset.ctypes.data, None))
    t_tr = timed(transforms, 3)
    del dst
    count = (1 << ek8) // S
    wcols = [rand(count + lo + hi) for _ in range(qc.total)]
    wout = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
    wp = [w.data_ptr() for w in wcols]
    t_win = timed(lambda: prog8.run_window_device(wp, ek8, 3 * count, count, wout.data_ptr()), 3)
    for key in (False, True):
        recv = max(exchange_bytes(qc.total, nC, k8, ek8, lo + hi, S, j, key)[0] for j in range(S))
        t_link = recv / (LINK_GBPS * 1e9) * 1e3
        print(f"(e) PROJECTION, ASSUMED link rate {LINK_GBPS:.0f} GB/s, key {'as row shards' if key else 'EXTENDED'} -- quotient phase at k = {k8} on {S} cards "
              f"(unmeasured on multi-GPU hardware): per device {share} coset transform(s) 2^{k8}->2^{ek8} {t_tr:.3f} ms (measured) + window kernel "
              f"2^{ek8 - 3} rows {t_win:.3f} ms (measured) + exchange {recv / 2**20:.0f} MB (computed from the copy plan) / {LINK_GBPS:.0f} GB/s = "
              f"{t_link:.3f} ms (assumed rate) -> {t_tr + t_win + t_link:.3f} ms", flush=True)
    print("(e) k = 24 on 8 cards, " + plan_line(qc.total, nC, k8, ek8, lo + hi, S), flush=True)


def row_shard_key():
    """(f) and (g)"""
    k, ek = 22, 24
    prog = E.evaluate_h_program(cs, k, ek, *CH)
    lo, hi = prog.halos(ek)
    dom = Z.EvaluationDomain(4, k)
    torch.manual_seed(3)
    cols = [rand(1 << (ek if f == E.COL_EXTENDED else k)) for f in FORMS]
    coeff_idx = [i for i, f in enumerate(FORMS) if f == E.COL_COEFF]
    key_idx = [i for i, f in enumerate(FORMS) if f == E.COL_EXTENDED]
    nC = len(coeff_idx)
    init(1)
    ext = {i: torch.empty((1 << ek, 4), dtype=torch.int64, device="cuda") for i in coeff_idx}
    out_a = torch.zeros((1 << ek, 4), dtype=torch.int64, device="cuda")
    out_b, out_c = torch.zeros_like(out_a), torch.zeros_like(out_a)

    def composition():
        for i in coeff_idx:
            _lib.check(lib.zkhip_coeff_to_extended_device(cols[i].data_ptr(), 1 << k, k, ext[i].data_ptr(), 1 << ek, ek, 1, dom.extended_omega.ctypes.data,
                                                          dom.g_coset.ctypes.data, None))
        prog.run_device([(ext[i] if i in ext else cols[i]).data_ptr() for i in range(qc.total)], ek, out_a.data_ptr())

    def shards_of_key():
        rs = E.RowShards(ek, len(key_idx), lo, hi)
        for c, i in enumerate(key_idx):
            rs.scatter_device(c, cols[i].data_ptr())
        return rs

    extended_cols = [(c.data_ptr(), f) for c, f in zip(cols, FORMS)]
    rs = shards_of_key()
    rs_cols = [(rs.ref(key_idx.index(i)), E.COL_ROW_SHARDS) if i in key_idx else (cols[i].data_ptr(), E.COL_COEFF) for i in range(qc.total)]
    runs = {"composition": (composition, out_a),
            "EXTENDED key": (lambda: E.evaluate_rows_sharded_device(prog, extended_cols, k, ek, dom, out_b.data_ptr()), out_b),
            "row-shard key": (lambda: E.evaluate_rows_sharded_device(prog, rs_cols, k, ek, dom, out_c.data_ptr()), out_c)}
    times = {name: [] for name in runs}
    for fn, _ in runs.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(REPS):                                    # interleaved: every repetition runs all three, one after another
        for name, (fn, _) in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(out_a, out_b) and torch.equal(out_a, out_c)
    print(f"(f) S = 1, k={k} ext_k={ek}, {REPS} interleaved repetitions each (ms, sorted): "
          + "; ".join(f"{name} " + " ".join(f"{t:.3f}" for t in sorted(v)) for name, v in times.items()), flush=True)
    rs.destroy()
    del ext
    torch.cuda.empty_cache()
    for S in (3, 8):
        init(S)
        rs = shards_of_key()
        rs_cols = [(rs.ref(key_idx.index(i)), E.COL_ROW_SHARDS) if i in key_idx else (cols[i].data_ptr(), E.COL_COEFF) for i in range(qc.total)]
        out_d = torch.zeros_like(out_a)
        te = timed(lambda: E.evaluate_rows_sharded_device(prog, extended_cols, k, ek, dom, out_d.data_ptr()))
        assert torch.equal(out_d, out_a), S
        out_d.zero_()
        tr = timed(lambda: E.evaluate_rows_sharded_device(prog, rs_cols, k, ek, dom, out_d.data_ptr()))
        assert torch.equal(out_d, out_a), S
        rs.destroy()
        print(f"(f) S = {S} contexts of ONE card (wall time, NOT a speed claim): EXTENDED key {te:8.3f} ms, row-shard key {tr:8.3f} ms; "
              + plan_line(qc.total, nC, k, ek, lo + hi, S), flush=True)
    init(1)
    del cols, out_a, out_b, out_c
    torch.cuda.empty_cache()
    # (g) the Lagrange kernel against the three transforms it replaces
    n, N = 1 << k, 1 << ek
    u = n - (cs.blinding_factors + 1)
    ind = torch.zeros((3, n, 4), dtype=torch.int64, device="cuda")
    l_ext = torch.empty((3, N, 4), dtype=torch.int64, device="cuda")
    one = torch.from_numpy(F.fr_encode([1]).view("int64")).cuda()[0]

    def transforms():
        ind.zero_()
        ind[0, 0], ind[1, u], ind[2, :u] = one, one, one
        _lib.check(lib.zkhip_ifft_scaled_batch_device(ind.data_ptr(), dom.omega_inv.ctypes.data, k, dom.ifft_divisor.ctypes.data, 3, n, None))
        _lib.check(lib.zkhip_coeff_to_extended_device(ind.data_ptr(), n, k, l_ext.data_ptr(), N, ek, 3, dom.extended_omega.ctypes.data, dom.g_coset.ctypes.data, None))

    rs = E.RowShards(ek, 3, lo, hi)
    kernel = lambda: _lib.check(lib.zkhip_lagrange_cosets_row_shards_device(k, u, dom.omega.ctypes.data, dom.extended_omega.ctypes.data,
                                                                            dom.g_coset.ctypes.data, rs.handle, 0, None))
    tt, tk = timed(transforms), timed(kernel)
    same = all(np.array_equal(rs.download(c), l_ext[c].cpu().numpy().view(np.uint64)) for c in range(3))
    rs.destroy()
    print(f"(g) l0 / l_last / l_active_row at k={k} ext_k={ek} (u = {u}): indicator columns + ifft_scaled + coeff_to_extended {tt:8.3f} ms, "
          f"closed-form kernel {tk:8.3f} ms (equal bytes: {same})", flush=True)
    assert same


def keygen_timing():
    """keygen_device at k = 22 on the wrapper shape's key (6 fixed, 7 sigma columns), warm, with and without row_shards"""
    from zksnap_circuits_halo2_amd import keygen as KG
    k = 22
    n = 1 << k
    init(1)
    fixed = [rand(n).cpu().numpy().view(np.uint64) for _ in range(cs.num_fixed)]
    asm = KG.Assembly(n, len(cs.permutation_columns))
    rg = random.Random(5)
    for _ in range(1000):
        asm.copy(rg.randrange(len(cs.permutation_columns)), rg.randrange(n - 8), rg.randrange(len(cs.permutation_columns)), rg.randrange(n - 8))
    with Z.ParamsKZG.setup(k, 0xBEEF) as params:
        res = {}
        for rs in (False, True, False, True):                # the first of each is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pk = KG.keygen_device(params, cs, fixed, asm, row_shards=rs)
            res[rs] = (time.perf_counter() - t0) * 1e3
            pk.free()
    print(f"keygen_device k={k} (6 fixed + 7 sigma columns), warm: default {res[False]:.1f} ms, row_shards {res[True]:.1f} ms (one device)", flush=True)


def contexts_timing(counts):
    k, ek = 22, 24
    prog = E.evaluate_h_program(cs, k, ek, *CH)
    lo, hi = prog.halos(ek)
    dom = Z.EvaluationDomain(4, k)
    torch.manual_seed(3)
    cols = [rand(1 << (ek if f == E.COL_EXTENDED else k)) for f in FORMS]
    key_idx = [i for i, f in enumerate(FORMS) if f == E.COL_EXTENDED]
    extended_cols = [(c.data_ptr(), f) for c, f in zip(cols, FORMS)]
    out = torch.zeros((1 << ek, 4), dtype=torch.int64, device="cuda")
    back = torch.zeros_like(out)
    for S in counts:
        init(S)
        rs = E.RowShards(ek, len(key_idx), lo, hi)

        def scatter():
            for c, i in enumerate(key_idx):
                rs.scatter_device(c, cols[i].data_ptr())

        ts = timed(scatter)
        tg = timed(lambda: rs.gather_device(0, back.data_ptr()))
        assert torch.equal(back, cols[key_idx[0]]), S
        rs_cols = [(rs.ref(key_idx.index(i)), E.COL_ROW_SHARDS) if i in key_idx else (cols[i].data_ptr(), E.COL_COEFF) for i in range(qc.total)]
        te = timed(lambda: E.evaluate_rows_sharded_device(prog, extended_cols, k, ek, dom, out.data_ptr()))
        tr = timed(lambda: E.evaluate_rows_sharded_device(prog, rs_cols, k, ek, dom, out.data_ptr()))
        rs.destroy()
        print(f"contexts S = {S}: quotient EXTENDED key {te:8.3f} ms, row-shard key {tr:8.3f} ms, scatter of {len(key_idx)} columns {ts:8.3f} ms, "
              f"gather of one {tg:8.3f} ms", flush=True)
    init(1)


if __name__ == "__main__":
    if sys.argv[1:2] == ["contexts"]:
        contexts_timing([int(a) for a in sys.argv[2:]] or [1, 2, 8])
    elif sys.argv[1:] == ["windows"]:
        prog = E.evaluate_h_program(cs, 22, 24, *CH)
        tw, tn = whole_vs_windows(prog, 24)
        print(f"(c) compiled     : whole-domain 2^24 {tw:8.3f} ms   8 windows of 2^21 in sequence {tn:8.3f} ms   ratio {tn / tw:.4f}")
    elif sys.argv[1:] == ["rowshards"]:
        row_shard_key()
    elif sys.argv[1:] == ["keygen"]:
        keygen_timing()
    else:
        main()
        row_shard_key()

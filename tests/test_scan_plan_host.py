"""CPU (`-m "not gpu"`): csrc/scan_plan.hpp -- the level plan every chunked scan of poly.hip and paillier.hip walks, and the workspace sizes
built on it -- compiled for the host under ASan + UBSan (tests/cpp/scan_plan_host_check.cpp) and compared with Python integers.

The plan: L = scan_levels(n), the counts are the iterated ceil(n / 16), the offsets are 256-aligned, increasing and leave every level its
count x row_bytes, the total covers the last level, the last level is one chunk.  The sizes: none of the six *_workspace_bytes is larger than
the formula it replaced (restated below), and each still holds its driver's levels and what rides with them."""
import os
import subprocess

import pytest

from test_gpu_fr_scans import SCAN_SIZES, chunks_of, scan_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]

SIZES = sorted(set(SCAN_SIZES) | {0, 16 ** 6, 16 ** 6 + 1, 1 << 28, (1 << 40) + 1})
LANES = [1, 8, 65535]
ROW_BYTES = [32, 48] + [32 * lanes for lanes in LANES[1:]]
LOG_NS = [0, 1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 28]                 # 16^l, 2 * 16^l: a level more from the second on
PERMS = [(1, 1), (8, 3), (135, 4), (65535, 1)]                               # (columns, columns per set)


def _run(cmd, **kw):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600, **kw)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("scan_plan") / "scan_plan_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "scan_plan_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return str(out)


def _ask(exe, cases):
    """one line of integers per case; anything a sanitiser prints fails the run or the line count"""
    run = _run([exe], input="".join(" ".join(str(x) for x in c) + "\n" for c in cases))
    assert run.returncode == 0 and run.stdout.endswith(f"scan plan host check done: {len(cases)} cases\n"), run.stdout[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases) + 1, run.stdout[-4000:]
    return [[int(x) for x in line.split()] for line in lines[:-1]]


def al(b):
    return (b + 255) // 256 * 256


def plan_bytes(n, row_bytes):
    """the levels of a scan over n elements, each 256-aligned, in Python integers"""
    total = 0
    while n > 16:
        n = chunks_of(n)
        total += al(n * row_bytes)
    return total


def test_the_plan_is_the_iterated_ceil_n_over_16_with_aligned_disjoint_levels(exe):
    cases = [("plan", n, rb) for n in SIZES for rb in ROW_BYTES]
    for (_, n, rb), got in zip(cases, _ask(exe, cases)):
        L, total, rest = got[0], got[1], got[2:]
        assert L == scan_levels(n) and len(rest) == 2 * L + 1, (n, rb, got)
        counts, offs = [n] + rest[0:2 * L:2] + [rest[-1]], rest[1:2 * L:2]
        for k in range(1, L + 2):
            assert counts[k] == chunks_of(counts[k - 1]), (n, rb, k, got)
        assert counts[L] <= 16, (n, rb, got)                                  # the last level is one chunk (level 0 itself without stored levels)
        ends = offs[1:] + [total]
        for k in range(L):
            assert offs[k] % 256 == 0 and offs[k] + counts[k + 1] * rb <= ends[k], (n, rb, k, got)
        assert offs == sorted(set(offs)) and (not offs or offs[0] == 0), (n, rb, got)
        assert total == plan_bytes(n, rb) < 1 << 64, (n, rb, got)


# ---- the formulas these sizes had before the plan, as plain integer arithmetic
def old_poly(n):
    total, m = 8192, n
    while m > 1:
        m = chunks_of(m)
        total += al(m * 32) + 256
    return total + al(n * 36)


def old_batch(n, count):
    total, m = 8192 + al(count * 8), n
    while m > 1:
        m = chunks_of(m)
        total += al(count * m * 32) + 256
    return total


def old_roots(n, m):
    total, c = 256, n
    while c > 1:
        c = chunks_of(c)
        total += al(m * c * 32)
    return max(total, old_poly(n))


def perm_tables(nperm, log_n):
    h = (log_n + 1) // 2
    return al(nperm * 16) + al(nperm * 32) + ((1 << h) + ((1 << log_n) >> h)) * 32 + 768


def old_perm(nperm, chunk, log_n):
    return perm_tables(nperm, log_n) + old_poly(-(-nperm // chunk) << log_n)


def old_lookup(n_lookups, log_n):
    return al(n_lookups * 16) + 256 + plan_bytes(1 << log_n, 32 * n_lookups) + old_poly(n_lookups << log_n)


def old_paillier(n, n_cols):
    return 256 + plan_bytes(n, 48 * n_cols)


def test_no_workspace_grew_and_each_still_holds_its_levels_and_riders(exe):
    """(case, the old size, what the driver carves: its levels, the 256-byte constant block, the n x 36 bytes of the batch inversion, the
    pointer tables)"""
    cases = []
    for n in SIZES:
        cases.append((("poly", n), old_poly(n), plan_bytes(n, 32) + 256 + n * 36))
        for lanes in LANES:
            cases.append((("batch", n, lanes), old_batch(n, lanes), lanes * 8 + 256 + plan_bytes(n, 32 * lanes)))
            cases.append((("paillier", n, lanes), old_paillier(n, lanes), plan_bytes(n, 48 * lanes)))
        for m in range(1, 9):
            cases.append((("roots", n, m), old_roots(n, m), max(plan_bytes(n, 32 * m), plan_bytes(n, 32) + 256)))
    for log_n in LOG_NS:
        for lanes in LANES:
            whole = lanes << log_n                                             # the batch inversion takes all lookups as one array
            cases.append((("lookup", lanes, log_n), old_lookup(lanes, log_n), lanes * 16 + max(plan_bytes(1 << log_n, 32 * lanes), whole * 36)))
        for nperm, chunk in PERMS:
            whole = -(-nperm // chunk) << log_n                                # all sets as one array, inverted and then scanned
            cases.append((("perm", nperm, chunk, log_n), old_perm(nperm, chunk, log_n), perm_tables(nperm, log_n) - 768 + 64 + 255 + max(plan_bytes(whole, 32), whole * 36)))
    for (case, old, needs), (got,) in zip(cases, _ask(exe, [c[0] for c in cases])):
        assert needs <= got <= old, (case, needs, got, old)

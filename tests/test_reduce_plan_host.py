"""CPU (`-m "not gpu"`): csrc/reduce_plan.hpp -- the launches `msm_reduce_buckets` picks from (B, WB) -- compiled for the host under ASan + UBSan
(tests/cpp/reduce_plan_host_check.cpp).  The program checks, for c = 2 .. 21 and bucket-set counts on both sides of every bound, that the
planned launches consume steps 1 .. c-2 exactly once, that strides chain and stay inside the ping-pong buffers, and that the finish kernel's
levels fit its LDS buffers; this file compares every printed plan with the rules restated in Python integers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
STEP, QUAD, PAIR, FINISH = 0, 1, 2, 3
QUAD_MAX, PAIR_MAX_LANES, FINISH_MAX_SETS, FINISH_ADDS = 65536, 1 << 16, 64, 128


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    out = tmp_path_factory.mktemp("reduce_plan") / "reduce_plan_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "reduce_plan_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    run = _run([str(out)])
    lines = run.stdout.splitlines()
    assert run.returncode == 0 and lines and lines[-1] == f"reduce plan host check done: {len(lines) - 1} cases", run.stdout[-4000:]
    return [[int(x) for x in line.split()] for line in lines[:-1]]


def adds(N, s):
    return N // 2 + s * (N // 4)


def expected(c, WB):
    """(kind, s, steps, N, in_stride, out_stride) per launch"""
    B = 1 << (c - 1)
    finish = WB <= FINISH_MAX_SETS
    N, s, stride, out = B, 1, B, []
    while N > 2:
        a = adds(N, s)
        if finish and a <= FINISH_ADDS:
            break
        a2 = adds(N // 2, s + 1) if N >= 8 else 0
        if a * WB > QUAD_MAX:
            kind, steps, o = STEP, 1, a
        elif finish and N >= 8 and a2 > FINISH_ADDS and a2 * WB * 8 < PAIR_MAX_LANES:
            kind, steps, o = PAIR, 2, a2
        else:
            kind, steps, o = QUAD, 1, a
        out.append((kind, s, steps, N, stride, o))
        stride, N, s = o, N >> steps, s + steps
    if finish:
        out.append((FINISH, s, c - 2 - (s - 1), N, stride, 0))
    return out


def test_every_plan_follows_the_rules(plans):
    assert {p[0] for p in plans} == set(range(2, 22))
    for c, WB, finish, nz, last_stride, *rest in plans:
        got = [tuple(rest[i:i + 6]) for i in range(0, len(rest), 6)]
        assert got == expected(c, WB), (c, WB, got)
        assert finish == (WB <= FINISH_MAX_SETS) and nz == c - 2, (c, WB)
        assert sum(l[2] for l in got) == c - 2 if finish else len(got) == c - 2, (c, WB, got)


def test_the_flagship_plan(plans):
    """c = 20, one bucket set: four single-lane steps, three quad steps (a pair there would be 2^16 lanes or more), four pairs, the finish
    from step 16"""
    (p,) = [p for p in plans if p[0] == 20 and p[1] == 1]
    kinds = [(p[5 + i], p[6 + i]) for i in range(0, len(p) - 5, 6)]
    assert kinds == [(STEP, 1), (STEP, 2), (STEP, 3), (STEP, 4), (QUAD, 5), (QUAD, 6), (QUAD, 7), (PAIR, 8), (PAIR, 10), (PAIR, 12), (PAIR, 14), (FINISH, 16)]


def test_small_windows_are_the_finish_kernel_alone_and_large_batches_keep_single_steps(plans):
    for c, WB, finish, nz, last_stride, *rest in plans:
        kinds = rest[0::6]
        if WB > FINISH_MAX_SETS:
            assert not finish and FINISH not in kinds and PAIR not in kinds and len(kinds) == c - 2 and last_stride == c, (c, WB)
        elif c <= 8:
            assert kinds == [FINISH], (c, WB)                   # B <= 128: step 1 has 96 additions at most

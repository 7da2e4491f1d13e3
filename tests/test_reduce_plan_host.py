"""CPU (`-m "not gpu"`): csrc/reduce_plan.hpp -- every launch `msm_reduce_buckets` makes for (B, WB, prepared), and the index maps of its
pyramid kernels -- compiled for the host under ASan + UBSan (tests/cpp/reduce_plan_host_check.cpp).  The program checks, for c = 2 .. 21,
bucket-set counts on both sides of every bound and both kinds of bases, that the planned launches consume steps 1 .. c-2 exactly once, that
strides chain and stay inside the ping-pong buffers, that the finish kernel's levels fit its LDS buffers, that a fused pair is the plan's
first launch with N >= 8 and a lane count inside its window, and -- by executing every plan on integers with the kernels' own index maps,
each state in a heap buffer of exactly its size -- that every lane reads and writes inside its state and that the launches together
compute sum_k (k + 1) b_k.  This file compares every printed plan with the rules restated in Python integers: the pyramid's entries as the
two rules that used to live apart (single steps, then whether the first two go in one launch), the grid widths and the tail as
`msm_reduce_buckets` computed them at the launch site before the plan did."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
STEP, QUAD, PAIR, FINISH, FUSED, HORNER_QUAD, HORNER, STORE, FOLD = range(9)
QUAD_MAX, PAIR_MAX_LANES, FINISH_MAX_SETS, FINISH_ADDS = 65536, 1 << 16, 64, 128
MIN_LANES, END_LANES = 1 << 17, 1 << 18
HEAD, ENTRY = 7, 7                    # numbers of a printed line in front of the entries, and per entry


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


def _entries(rest):
    return [tuple(rest[i:i + ENTRY]) for i in range(0, len(rest), ENTRY)]


def adds(N, s):
    return N // 2 + s * (N // 4)


def expected_steps(c, WB):
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


def expected_fuse(c, WB):
    """(fused, lanes): steps 1 and 2 are both single-lane entries (more than QUAD_MAX additions over all sets; step 2 has B / 2) and the launch
    of B / 4 lanes per set is one round of two wavefronts per SIMD"""
    B = 1 << (c - 1)
    lanes = B // 4 * WB
    fused = B >= 8 and (B // 2) * WB > QUAD_MAX and MIN_LANES <= lanes < END_LANES
    return (1, lanes) if fused else (0, 0)


def expected(c, WB, prepared):
    """(kind, s, steps, N, in_stride, out_stride, grid) per launch: the single steps, the first two replaced by one launch where the fuse
    rule says so (the buckets in, the state behind step 2 out), then the tail; every grid width as the launch site used to compute it"""
    steps = expected_steps(c, WB)
    if expected_fuse(c, WB)[0]:
        (k1, s1, _, N1, in1, _), (k2, s2, _, _, _, out2) = steps[:2]
        assert (k1, s1, k2, s2) == (STEP, 1, STEP, 2)
        steps[:2] = [(FUSED, 1, 2, N1, in1, out2)]
    out = []
    for kind, s, n, N, i, o in steps:
        grid = {STEP: (o + 127) // 128, QUAD: (4 * o + 127) // 128, PAIR: (8 * o + 127) // 128, FUSED: (N // 4 + 127) // 128, FINISH: WB}[kind]
        out.append((kind, s, n, N, i, o, grid))
    direct = prepared and WB <= 2048
    if WB > FINISH_MAX_SETS:              # no finish kernel: the state after the last step is [X0, X1, Z^0 .. Z^(c-3)]
        if WB <= 2048:
            out.append((HORNER_QUAD, c - 1, 0, 2, c, 0, WB))
        else:
            out.append((HORNER, c - 1, 0, 2, c, 0, (WB * 32 + 63) // 64))
    if prepared and not direct:
        out.append((STORE, c - 1, 0, 2, 0, 0, (WB + 63) // 64))       # (K = WB results)
    elif not prepared:
        out.append((FOLD, c - 1, 0, 2, 0, 0, 1))
    return out, direct


def test_every_plan_follows_the_rules(plans):
    assert {p[0] for p in plans} == set(range(2, 22)) and {p[2] for p in plans} == {0, 1}
    for c, WB, prepared, finish, direct, nz, last_stride, *rest in plans:
        got = _entries(rest)
        want, want_direct = expected(c, WB, bool(prepared))
        assert got == want and bool(direct) == want_direct, (c, WB, prepared, got)
        assert finish == (WB <= FINISH_MAX_SETS) and nz == c - 2, (c, WB)
        pyramid = [l for l in got if l[0] in (STEP, QUAD, PAIR, FUSED, FINISH)]
        assert sum(l[2] for l in pyramid) == c - 2, (c, WB, got)
        if not finish:
            assert len(pyramid) == c - 2 - sum(l[0] == FUSED for l in pyramid), (c, WB, got)


def test_every_line_follows_the_rule(plans):
    """the fuse rule on its own: every printed plan holds the fused launch exactly where the rule says, as its first entry, with the rule's
    lane count over all sets"""
    assert {p[0] for p in plans} == set(range(2, 22))
    for c, WB, prepared, finish, direct, nz, last_stride, *rest in plans:
        got = _entries(rest)
        kinds = [l[0] for l in got]
        fused, lanes = (1, got[0][3] // 4 * WB) if got[0][0] == FUSED else (0, 0)
        assert (fused, lanes) == expected_fuse(c, WB), (c, WB)
        assert kinds.count(FUSED) == fused, (c, WB, prepared)


def test_the_flagship_plan(plans):
    """c = 20, one bucket set, prepared: steps 1 + 2 in one launch, two single-lane steps, three quad steps (a pair there would be 2^16
    lanes or more), four pairs, the finish from step 16, which writes the result itself"""
    (p,) = [p for p in plans if p[:3] == [20, 1, 1]]
    kinds = [(l[0], l[1]) for l in _entries(p[HEAD:])]
    assert kinds == [(FUSED, 1), (STEP, 3), (STEP, 4), (QUAD, 5), (QUAD, 6), (QUAD, 7), (PAIR, 8), (PAIR, 10), (PAIR, 12), (PAIR, 14), (FINISH, 16)]
    assert p[4] == 1


def test_the_flagship_and_the_boundaries(plans):
    """(B, WB) = (2^19, 1): steps 1 + 2 go in one launch of 2^17 lanes; (2^17, 1) has one single-lane entry and (2^18, 1) a launch of 2^16
    lanes: nothing fused; 16 sets of 2^15 are fused, 8 (2^16 lanes) and 43 (more than 2^18) are not"""
    got = {}
    for c, WB, prepared, *rest in plans:
        first = _entries(rest[HEAD - 3:])[0]
        got[(c, WB, prepared)] = (1, first[3] // 4 * WB) if first[0] == FUSED else (0, 0)
    assert all(FUSED not in [l[0] for l in _entries(p[HEAD:])[1:]] for p in plans)
    for prepared in (0, 1):
        assert got[(20, 1, prepared)] == (1, 1 << 17)
        assert got[(18, 1, prepared)] == (0, 0) and got[(19, 1, prepared)] == (0, 0)
        assert got[(16, 16, prepared)] == (1, 1 << 17) and got[(16, 8, prepared)] == (0, 0) and got[(16, 43, prepared)] == (0, 0)
        assert got[(21, 1, prepared)] == (0, 0) and got[(13, 100, prepared)] == (0, 0)


def test_small_windows_are_the_finish_kernel_alone_and_large_batches_keep_single_steps(plans):
    for c, WB, prepared, finish, direct, nz, last_stride, *rest in plans:
        kinds = [l[0] for l in _entries(rest)]
        pyramid = [k for k in kinds if k in (STEP, QUAD, PAIR, FUSED, FINISH)]
        if WB > FINISH_MAX_SETS:
            assert not finish and FINISH not in kinds and PAIR not in kinds and last_stride == c, (c, WB)
            assert len(pyramid) == c - 2 - pyramid.count(FUSED), (c, WB)
            assert kinds[len(pyramid)] == (HORNER_QUAD if WB <= 2048 else HORNER), (c, WB)
        elif c <= 8:
            assert pyramid == [FINISH], (c, WB)                 # B <= 128: step 1 has 96 additions at most
        assert kinds[len(pyramid) + (0 if finish else 1):] == ([] if direct else [STORE if prepared else FOLD]), (c, WB, prepared)

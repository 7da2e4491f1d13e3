"""CPU (`-m "not gpu"`): csrc/reduce_fuse.hpp -- whether `msm_reduce_buckets` carries steps 1 and 2 of the bucket reduction in one launch --
compiled for the host under ASan + UBSan (tests/cpp/reduce_fuse_host_check.cpp).  The program checks, for c = 2 .. 21 and the bucket-set
counts of the plan's own check, that a fused pair is the plan's first two entries, both single-lane steps, with N >= 8, that the fused
launch's strides are the state sizes around the two steps, that nothing reads or writes past B elements and that the plan is left unchanged;
this file compares every printed line with the rule restated in Python integers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
QUAD_MAX = 65536
MIN_LANES, END_LANES = 1 << 17, 1 << 18


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)


@pytest.fixture(scope="module")
def fusions(tmp_path_factory):
    out = tmp_path_factory.mktemp("reduce_fuse") / "reduce_fuse_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "reduce_fuse_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    run = _run([str(out)])
    lines = run.stdout.splitlines()
    assert run.returncode == 0 and lines and lines[-1] == f"reduce fuse host check done: {len(lines) - 1} cases", run.stdout[-4000:]
    return [[int(x) for x in line.split()] for line in lines[:-1]]


def expected(c, WB):
    """(fused, lanes): steps 1 and 2 are both single-lane entries (more than QUAD_MAX additions over all sets; step 2 has B / 2) and the launch
    of B / 4 lanes per set is one round of two wavefronts per SIMD"""
    B = 1 << (c - 1)
    lanes = B // 4 * WB
    fused = B >= 8 and (B // 2) * WB > QUAD_MAX and MIN_LANES <= lanes < END_LANES
    return (1, lanes) if fused else (0, 0)


def test_every_line_follows_the_rule(fusions):
    assert {f[0] for f in fusions} == set(range(2, 22))
    for c, WB, fused, lanes in fusions:
        assert (fused, lanes) == expected(c, WB), (c, WB)


def test_the_flagship_and_the_boundaries(fusions):
    """(B, WB) = (2^19, 1): steps 1 + 2 go in one launch of 2^17 lanes; (2^17, 1) has one single-lane entry and (2^18, 1) a launch of 2^16
    lanes: nothing fused; 16 sets of 2^15 are fused, 8 (2^16 lanes) and 43 (more than 2^18) are not"""
    got = {(c, WB): (fused, lanes) for c, WB, fused, lanes in fusions}
    assert got[(20, 1)] == (1, 1 << 17)
    assert got[(18, 1)] == (0, 0) and got[(19, 1)] == (0, 0)
    assert got[(16, 16)] == (1, 1 << 17) and got[(16, 8)] == (0, 0) and got[(16, 43)] == (0, 0)
    assert got[(21, 1)] == (0, 0) and got[(13, 100)] == (0, 0)

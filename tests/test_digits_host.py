"""CPU (`-m "not gpu"`): csrc/msm_digits.hpp -- the scalar conversion by the Montgomery reduction alone and the signed recoding specialised
on the (20, 13, 4) window layout -- compiled for the host under ASan + UBSan (tests/cpp/digits_host_check.cpp).  The program checks, on 0, 1,
r - 1, (r - 1) / 2, 2^k and 2^k - 1 at every window boundary, scalars whose every window is 2^(cw-1) - 1 or 2^(cw-1) (the carry runs through
all 13 windows), scalars whose top window takes a carry, and 4000 seeded random scalars, that the conversion returns the canonical integer,
that sum_w d_w 2^(off_w) is that integer, that |d_w| <= 2^(cw-1), and that the digits equal the generic recoding's digit for digit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = tmp_path_factory.mktemp("digits") / "digits_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "digits_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    return _run([str(out)])


def test_conversion_and_recoding_match_the_big_integers(report):
    lines = report.stdout.splitlines()
    assert report.returncode == 0 and lines and lines[-1].startswith("digits host check done: "), report.stdout[-4000:]
    assert "runtime error" not in report.stdout and "AddressSanitizer" not in report.stdout, report.stdout[-4000:]


def test_every_listed_scalar_ran(report):
    """4 + 4 * 12 boundary scalars + 2 * 16 inside the top window + 6 + 2 + 1 carry patterns + 4000 random"""
    assert report.stdout.splitlines()[-1] == f"digits host check done: {4 + 48 + 32 + 6 + 2 + 1 + 4000} scalars", report.stdout[-2000:]

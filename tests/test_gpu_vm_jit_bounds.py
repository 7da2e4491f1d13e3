"""GPU (-m gpu): both executors of a row program -- the interpreter of csrc/rowvm.hip and the run-time compiled kernels of csrc/rowvm_jit.hip --
on the programs of tests/jit_bounds.py, which put a register AT the generator's magnitude thresholds, over 64 rows on the 8 x 8 grid of
[0, 1, r-1, r-2, 2, (r+1)/2, (r-1)/2, one seeded value]: on some rows a register is m (r-1), on others an exact multiple of r.  The expectation
is the oracle's interpreter (oracle/bn254.py `row_program_run`), compared as canonical bytes.

Which executor ran is read from `zkhip_test_rows_compiled_count`: the interpreter takes over silently when a compilation fails, so every
compiled case must raise the counter by one and every interpreted case must leave it alone.  The executor switch $ZKHIP_VM_JIT is read once
per process: the compiled cases run in a fresh child process with ZKHIP_VM_JIT=2, about 8 programs (8 compilations) per child."""
import functools
import json
import os
import subprocess
import sys

import pytest

import jit_bounds as J

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def expected(scenario):
    """label -> the oracle's bytes, once per scenario"""
    return {job.label: J.expected_bytes(job) for job in J.jobs_of(scenario)}


def rows_that_differ(got, exp):
    return [i for i in range(len(exp) // 32) if got[32 * i:32 * i + 32] != exp[32 * i:32 * i + 32]]


def run_compiled(scenario):
    """the jobs of `scenario` in one fresh process under ZKHIP_VM_JIT=2: every output against the oracle, every launch against the counter"""
    jobs = J.jobs_of(scenario)
    code = "import sys; sys.path[:0] = [%r, %r]; import jit_bounds; jit_bounds.child_main(%r)" % (ROOT, HERE, scenario)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=dict(os.environ, ZKHIP_VM_JIT="2", ZKHIP_VM_JIT_LOG="1"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "compilation failed" not in res.stderr, res.stderr[-3000:]
    lines = [json.loads(l[4:]) for l in res.stdout.splitlines() if l.startswith("JOB ")]
    assert [l["label"] for l in lines] == [j.label for j in jobs]
    exp = expected(scenario)
    wrong = []
    for job, line in zip(jobs, lines):
        got = bytes.fromhex(line["out"])
        if got != exp[job.label]:
            wrong.append("%s: rows %s differ from the oracle" % (job.label, rows_that_differ(got, exp[job.label])[:8]))
        if line["compiled"] != (1 if job.compiled else 0):
            wrong.append("%s: %d compiled launches, expected %d" % (job.label, line["compiled"], int(job.compiled)))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("group", range(J.N_GROUPS))
def test_directed_programs_through_the_interpreter(lib, group):
    """in this process (the default mode compiles only from 2^18 rows): the counter must not move"""
    scenario = "directed:%d" % group
    exp = expected(scenario)
    for job in J.jobs_of(scenario):
        got, compiled = J.run_job(lib, job)
        assert compiled == 0, job.label
        assert got == exp[job.label], "%s: rows %s differ from the oracle" % (job.label, rows_that_differ(got, exp[job.label])[:8])


@pytest.mark.parametrize("group", range(J.N_GROUPS))
def test_directed_programs_through_compiled_kernels(group):
    run_compiled("directed:%d" % group)


def test_negated_zero_product_is_zero_in_both_executors(lib):
    """-(col0 * col1) on a row where col0 = 0: K r - 0 is an exact multiple of r and must be stored as 32 zero bytes"""
    scenario = "directed:%d" % ([d.name for d in J.DIRECTED].index("neg_of_product") // J.GROUP)
    job = [j for j in J.jobs_of(scenario) if j.label == "neg_of_product"][0]
    assert job.cols[0][0] == 0 and job.cols[1][0] == 0 and job.cols[0][8] == 0 and job.cols[1][8] == 1
    exp = expected(scenario)["neg_of_product"]
    assert exp[:32] == bytes(32) and exp[8 * 32:9 * 32] == bytes(32)
    got, compiled = J.run_job(lib, job)
    assert compiled == 0 and got[:32] == bytes(32) and got[8 * 32:9 * 32] == bytes(32) and got == exp
    # the compiled executor's run of the same job is test_directed_programs_through_compiled_kernels[that group], against the same bytes


def test_one_cached_kernel_serves_other_constants_accumulate_and_not_other_rotations_or_rows():
    """in one child: the same instructions with other constant values, the same program with accumulate off and then on (PREV), other rotation
    values in the same slots, the same program at 2^6 and then 2^7 rows and back"""
    run_compiled("reuse")


def test_both_sides_of_the_compiler_limits():
    """256 instructions compiled, 257 interpreted; 96 columns compiled, 97 interpreted; a program with no column at all compiled"""
    run_compiled("limits")

"""CPU (`-m "not gpu"`): csrc/rowvm_blob.hpp -- the one blob layout and the one fill behind every launch of the row-program interpreter --
compiled for the host under ASan + UBSan (tests/cpp/rowvm_blob_host_check.cpp).  The program checks, for program shapes on both sides of
every rounding, alone and side by side, around the 2^12 split of the power tables, over whole columns and window buffers: that the pieces
of the plan are 256-aligned, disjoint and inside its total; that the fill stays inside a heap buffer of exactly the staged size; that, under
a host model of the kernel's address rule, operands a and b of every micro-op (padding included) at the first and the last row land inside
the named column or inside the program's own constants; that a product's single memory operand is second; that each part record points
into its own region.  This file compares the sizes it prints with the byte formulas of the two launch paths this layout replaced, restated
in integers: a workspace never smaller than before, equal where several programs share a launch, and at most the 256 bytes of one part
record larger for one program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
INSNS, CONSTS, ROTS, COLUMNS, PROGS, LOG_ROWS, MODES = (1, 2, 3, 4, 5, 1000), (0, 1, 7, 8, 9), (0, 1, 3, 256), (0, 1, 31, 32, 33), (1, 2, 5, 257), (0, 11, 12, 13), 3
UOP, PART, POW_LO_BITS = 64, 40, 12


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    out = tmp_path_factory.mktemp("rowvm_blob") / "rowvm_blob_host_check"
    build = _run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc"),
                  os.path.join(ROOT, "tests", "cpp", "rowvm_blob_host_check.cpp"), "-o", str(out)])
    assert build.returncode == 0, build.stdout
    run = _run([str(out)])
    lines = run.stdout.splitlines()
    assert run.returncode == 0 and lines and lines[-1] == f"rowvm blob host check done: {len(lines) - 1} cases", run.stdout[-4000:]
    return [[int(x) for x in line.split()] for line in lines[:-1]]


def a256(x):
    return (x + 255) & ~255


def region(n_insns, n_constants, n_rotations):
    return a256((n_insns + 4) * UOP) + a256(n_constants * 32 + 32) + a256(n_rotations * 4 + 4)


def tables(log_rows):
    return a256((1 << POW_LO_BITS) * 32) + a256((((1 << log_rows) >> POW_LO_BITS) + 1) * 32)


def single_before(n_insns, n_constants, n_rotations, n_columns, log_rows):
    """row_vm_workspace_bytes as it was: [micro-ops | constants | rotation offsets | columns | omega | power tables]"""
    return region(n_insns, n_constants, n_rotations) + a256(n_columns * 8 + 8) + 256 + tables(log_rows)


def multi_before(shapes, n_columns, log_rows):
    """row_vm_multi_workspace_bytes as it was: [columns | omega | part records | a region per program | power tables]"""
    return a256(n_columns * 8 + 8) + 256 + a256(len(shapes) * PART) + sum(region(*s) for s in shapes) + tables(log_rows)


def shapes_of(n_insns, n_constants, n_rotations, n_progs):
    """the programs of a printed case (shape_of in the C++ program): the named shape in the middle, short ones beside it"""
    ii, ci, ri = INSNS.index(n_insns), CONSTS.index(n_constants), ROTS.index(n_rotations)
    return [(n_insns, n_constants, n_rotations) if j == n_progs // 2 else (INSNS[(ii + j) % 5], CONSTS[(ci + j) % 5], ROTS[(ri + j) % 3])
            for j in range(n_progs)]


def test_every_listed_shape_was_checked(plans):
    shapes = len(INSNS) * len(CONSTS) * len(ROTS) * len(COLUMNS) * len(LOG_ROWS)
    assert len(plans) == shapes * (len(PROGS) - 1) * MODES + shapes          # (257 programs: one of the modes per shape, in turn)
    assert {p[6] for p in plans if p[4] == 257} == set(range(MODES))
    for column, values in enumerate((INSNS, CONSTS, ROTS, COLUMNS, PROGS, LOG_ROWS, range(MODES))):
        assert {p[column] for p in plans} == set(values)


def test_the_workspace_is_never_smaller_and_at_most_one_part_record_larger(plans):
    for n_insns, n_constants, n_rotations, n_columns, n_progs, log_rows, mode, staged, total in plans:
        case = (n_insns, n_constants, n_rotations, n_columns, n_progs, log_rows, mode)
        shapes = shapes_of(n_insns, n_constants, n_rotations, n_progs)
        assert total == multi_before(shapes, n_columns, log_rows), case
        assert staged == total - tables(log_rows), case
        if n_progs == 1:
            before = single_before(n_insns, n_constants, n_rotations, n_columns, log_rows)
            assert before <= total <= before + 256, case

"""GPU (-m gpu): zkhip_fr_fold_rows_device against Python integers (tests/gwc_reference.py fold): out_own[i][j] = +- r_i rows[i][j] and
out_shared[j] = +- sum_i r_i rows[i][n_own + j], for n_rows 1, 2, 63, 64, 65, 257, the kernel's workgroup size and one more, the first n_rows that
needs the second reduction level and one more (both read from csrc/gwc_fold.hpp), the shapes (n_cols, n_own) = (1, 0), (1, 1), (7, 3), (40, 33),
both signs, rows and multipliers drawn from {0, 1, r - 1, random}; a sub-range through offset pointers; zeros for an empty batch."""
import functools
import os
import random
import re

import numpy as np
import pytest
import torch

import gwc_reference as GR
from zksnap_circuits_halo2_amd import fields as F, multiopen as MO, tensors as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = F.R_MOD
DEV = torch.device("cuda", 0)


def _constant(name):
    text = open(os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc", "gwc_fold.hpp")).read()
    return int(re.search(r"constexpr uint32_t " + name + r" = (\d+);", text).group(1))


THREADS, LANE_ROWS = _constant("FOLD_THREADS"), _constant("FOLD_LANE_ROWS")
SPAN = THREADS * LANE_ROWS                          # FOLD_SPAN = FOLD_THREADS * FOLD_LANE_ROWS: rows of a column one workgroup sums
N_ROWS = sorted({1, 2, 63, 64, 65, 257, THREADS, THREADS + 1, SPAN + 1, SPAN + 2})
SHAPES = [(1, 0), (1, 1), (7, 3), (40, 33)]


def test_the_span_is_what_the_header_says():
    text = open(os.path.join(ROOT, "zksnap_circuits_halo2_amd", "csrc", "gwc_fold.hpp")).read()
    assert "constexpr uint32_t FOLD_SPAN = FOLD_THREADS * FOLD_LANE_ROWS;" in text and (THREADS, SPAN) == (256, 4096)


@functools.lru_cache(None)
def inputs(n_rows, n_cols):
    rng = random.Random(f"fold-{n_rows}-{n_cols}")
    rows = [GR.pick(rng, n_cols) for _ in range(n_rows)]
    r = GR.pick(rng, n_rows)
    d_rows = T.fr_words([a for row in rows for a in row], DEV).reshape(n_rows, n_cols, 4)
    return rows, r, d_rows, T.fr_words(r, DEV)


def run_fold(d_rows, n_own, d_r, negate):
    n, n_cols = d_rows.shape[0], d_rows.shape[1]
    out_own = torch.full((n * n_own + 1, 4), -1, dtype=torch.int64, device=DEV)                  # one element more than is written: it must stay as it is
    out_shared = torch.full((n_cols - n_own + 1, 4), -1, dtype=torch.int64, device=DEV)
    MO.fold_rows_device(d_rows, n_own, d_r, negate, out_own[:n * n_own], out_shared[:n_cols - n_own])
    torch.cuda.synchronize()
    assert bool((out_own[-1] == -1).all()) and bool((out_shared[-1] == -1).all())
    own = T.fr_ints(out_own[:n * n_own]) if n * n_own else []
    return [own[i * n_own:(i + 1) * n_own] for i in range(n)], (T.fr_ints(out_shared[:n_cols - n_own]) if n_cols > n_own else [])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n_rows", N_ROWS)
def test_fold_rows_against_integers(n_rows, shape):
    n_cols, n_own = shape
    rows, r, d_rows, d_r = inputs(n_rows, n_cols)
    for negate in (False, True):
        assert run_fold(d_rows, n_own, d_r, negate) == GR.fold(rows, n_own, r, negate), (n_rows, shape, negate)


def test_a_sub_range_is_the_same_call_with_offset_pointers():
    rows, r, d_rows, d_r = inputs(SPAN + 2, 7)
    for lo, hi in ((5, 70), (1, SPAN + 2), (SPAN, SPAN + 2)):
        assert run_fold(d_rows[lo:hi], 3, d_r[lo:hi], True) == GR.fold(rows[lo:hi], 3, r[lo:hi], True), (lo, hi)


def test_an_empty_batch_writes_zeros_to_the_shared_part():
    for n_cols, n_own in ((7, 3), (1, 0), (40, 33)):
        out_shared = torch.full((n_cols - n_own + 1, 4), -1, dtype=torch.int64, device=DEV)
        empty = torch.empty((0, n_cols, 4), dtype=torch.int64, device=DEV)
        MO.fold_rows_device(empty, n_own, torch.empty((0, 4), dtype=torch.int64, device=DEV), False, None, out_shared[:n_cols - n_own])
        torch.cuda.synchronize()
        assert bool((out_shared[:-1] == 0).all()) and bool((out_shared[-1] == -1).all())
    MO.fold_rows_device(torch.empty((0, 3, 4), dtype=torch.int64, device=DEV), 3, torch.empty((0, 4), dtype=torch.int64, device=DEV), True, None, None)      # nothing to write

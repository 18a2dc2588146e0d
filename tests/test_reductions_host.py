"""The restatements of tests/reductions.py against math.fsum, without a GPU.

A restatement is a fixed tree of additions.  Every addition multiplies what passes through it by at most 1 + u (u = 2^-53; additions are exact
where the result is subnormal), so a result whose longest chain from an input has `depth` additions is off by at most
((1 + u)^depth - 1) sum |x| <= depth u (1 + depth u) sum |x|.  The depth is read off the loop structure, per routine, in the docstrings
below and in reductions.depth_*; nothing here is fitted to what the code gives.  On sets whose every partial sum is exact (cancelling
multiples of 2^-10, equal rows of 24 bits, a single row, a single non-zero row) every order gives math.fsum's number exactly.  And the order
is the routine's and no other: on magnitudes 2^-60 ... 2^60 it differs from the row-order sum somewhere."""
import math

import numpy as np
import pytest

import reductions as R

EXACT = ("cancel", "equal", "minus_zero", "mixed_zero", "subnormal")


def check_columns(name, cols, got, depth):
    """cols[n][k], got[k]"""
    for k in range(cols.shape[1]):
        col, t = cols[:, k], float(got[k])
        if not np.all(np.isfinite(col)):
            assert np.isnan(t) or np.isinf(t), (name, k, t)
            continue
        exact = math.fsum(col)
        assert abs(t - exact) <= R.bound(depth, col), (name, k, t, exact, R.bound(depth, col))
        if name in EXACT or name.startswith("one_hot") or len(col) == 1:
            assert t == exact, (name, k, t, exact)
        if name == "equal":
            assert t == len(col) * col[0], (name, k)


@pytest.mark.parametrize("n", R.ROWS)
def test_reduce_jobs_host(n):
    """reduce_jobs_block, depth ceil(ceil(n / 1024) / 4) + 2 + 7 + 8: a thread's partial sum takes every fourth of its ceil(n / 1024) rows
    (the first addition is to +0.0 and exact, but counted), (p0 + p1) + (p2 + p3) is two more, the tree over the 128 row groups has seven
    levels, and the final loop adds the eight workgroups' rows one after the other from +0.0.  n = 8193: 3 + 17 = 20."""
    for name, rows in R.make_rows(n):
        for nv in (3, 7, 8):
            check_columns(name, rows[:, :nv], R.reduce_jobs(rows, nv), R.depth_reduce_jobs(n))
    assert R.depth_reduce_jobs(8193) == 20 and R.depth_reduce_jobs(1) == 18 and R.depth_reduce_jobs(4097) == 19


@pytest.mark.parametrize("n", R.ROWS)
def test_reduce_gather_host(n):
    """reduce_gather_row, depth ceil(ceil(n / 1024) / 4) + 2 + 10: the same per-thread sums, then a tree of ten levels over 1024 threads"""
    for name, rows in R.make_rows(n, ncol=R.GB_NV):
        check_columns(name, rows, [R.reduce_gather(rows[:, k]) for k in range(R.GB_NV)], R.depth_reduce_gather(n))


def test_the_orders_are_these_orders():
    """on the wide-magnitude set each restatement differs from the row-order sum in some column, and the wave's shuffle order (wave_sum) from
    the DPP butterfly's (tree64)"""
    from test_gpu_wave_reduce import tree64
    for n in (1025, 4097):
        rows = dict(R.make_rows(n))["spread"]
        seq = R.rows_in_order(rows, True)
        assert not np.all(R.same_bits(R.reduce_jobs(rows, 8), seq))
        assert not np.all(R.same_bits([R.reduce_gather(rows[:, k]) for k in range(8)], seq))
    rows = dict(R.make_rows(R.BLOCK, ncol=12))["spread"]
    assert not np.all(R.same_bits(R.block_reduce(rows), R.rows_in_order(rows, True)))
    assert not np.all(R.same_bits(R.wave_sum_shfl(rows[:64]), [tree64(rows[:64, k]) for k in range(12)]))
    # ... and a tail element that went to p[0] instead of p[u], or a main loop that took one row too few, would show: the four partial sums
    # of a thread are distinct chains
    rows = dict(R.make_rows(8193))["spread"]
    a = R.reduce_jobs(rows, 8)
    b = R.reduce_jobs(np.concatenate([rows[:4096], rows[5120:6144], rows[4096:5120], rows[6144:]]), 8)      # (second trip: p[0] and p[1] swapped)
    assert not np.all(R.same_bits(a, b))


@pytest.mark.parametrize("nv", (3, 7, 12))
def test_block_reduce_host(nv):
    """block_reduce_store<NV, 4>, depth 6 + 3: six shuffle steps in a wave, three additions over the four waves"""
    for name, rows in R.make_rows(R.BLOCK, ncol=nv):
        check_columns(name, rows, R.block_reduce(rows), R.DEPTH_BLOCK_REDUCE)


@pytest.mark.parametrize("n", (1, 2, 512, 1023, 1024))
def test_row_order_host(n):
    """the row-order finishers: n additions from +0.0 (k_group_ke_sum, k_class_kinetic_sum: n = 512; k_mol_sum), n - 1 from row 0
    (k_census_final); and the sum / minimum / maximum columns of RowsSumMinMax, whose extrema are exact"""
    for name, rows in R.make_rows(n, ncol=6):
        check_columns(name, rows, R.rows_in_order(rows, True), n)
        if name != "minus_zero" and name != "mixed_zero":      # (from row 0 a sum of -0.0 alone stays -0.0: the same number, other bits)
            assert np.all(R.same_bits(R.rows_in_order(rows, True), R.rows_in_order(rows, False))), name
        check_columns(name, rows, R.rows_in_order(rows, False), max(n - 1, 1))
        t = R.census_sum_min_max(rows)
        check_columns(name, rows[:, 0::3], t[0::3], max(n - 1, 1))
        if np.all(np.isfinite(rows)):
            assert np.array_equal(t[1::3], rows[:, 1::3].min(axis=0)) and np.array_equal(t[2::3], rows[:, 2::3].max(axis=0)), name


def test_maximum_drops_a_nan_row():
    rows = np.abs(dict(R.make_rows(1025))["nan_row"])
    assert np.isnan(rows[:, 7]).sum() == 1
    assert R.reduce_jobs_max(rows) == np.nanmax(rows[:, 7])
    assert R.reduce_jobs_max(np.zeros((5, 8))) == 0.0

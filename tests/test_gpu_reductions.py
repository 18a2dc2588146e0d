"""GPU tests (-m gpu) of the cross-workgroup reductions -- the level between a wave's sum and a number the library reports -- each run by itself
through the hooks of include/ddcmi_test.h (ddcmi_debug_reductions.inl, bonded.hip: the very kernels of the product with the product's launch
shapes) and held bit for bit, as uint64, against the restatements of tests/reductions.py (NaN against NaN counts as equal).

  * reduce_jobs_block (k_reduce_jobs with one and two jobs, k_reduce_jobs_images, k_reduce_hist) and reduce_gather_row (k_reduce_gather,
    k_reduce_gather_hist) at reductions.ROWS rows: one row group only, the first and last row of every workgroup's share, tails of 0, 1, 2
    and 3 rows behind the four-way loop, its first and second trip; on the row sets of reductions.make_rows, whose one-hot sets change a bit
    for any row read twice or not at all.  Columns >= nv are NaN in the input and must not reach the output.
  * column 7 as a maximum and the displacement word: exact <= d <= exact (1 + 2e-7) with exact = disp_dt sqrt(max) in decimal arithmetic.
    A NaN in column 7 drops out: fmax returns its other operand, so the bound ignores a workgroup that filed a NaN (none does: the
    kick kernels file |v|^2 of floats through an integer maximum).
  * tickets: launches repeated and interleaved on one scratch array give the same bits every time.
  * history: sequences of flushes with different numbers of pending steps on one scratch array; every step of every flush gets the bits
    k_reduce_jobs forms from the same rows and no word the kernel owns stays poisoned.  Before the tickets of k_reduce_hist got a place
    that does not move with the number of pending steps, the sequences (15, 7) and (32, 5, 32, 1) failed: see test_history_sequences.
  * block_reduce_store / block_vmax_store, k_census_final, k_group_ke_sum, k_class_kinetic_sum, k_mol_sum.
  * every hook refuses counts out of range."""
import ctypes
import decimal
import math

import numpy as np
import pytest

import reductions as R

pytestmark = pytest.mark.gpu
EINVAL = -2
POISON = 12345.0
FRONT_ONE, FRONT_TWO, FRONT_IMAGES = range(3)

c_int_p = ctypes.POINTER(ctypes.c_int)
c_double_p = ctypes.POINTER(ctypes.c_double)


def dp(a):
    return a.ctypes.data_as(c_double_p)


def ip(a):
    return a.ctypes.data_as(c_int_p)


@pytest.fixture(scope="module")
def lib(built):
    import ddcmd_amd._lib as L
    lib = L.load_test_library()
    lib.ddcmi_debug_reduce_jobs.argtypes = [ctypes.c_int, c_int_p, c_int_p, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    lib.ddcmi_debug_reduce_hist.argtypes = [ctypes.c_int, c_int_p, ctypes.c_int, ctypes.c_longlong, c_double_p, c_double_p, c_double_p]
    lib.ddcmi_debug_reduce_gather.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]
    lib.ddcmi_debug_reduce_gather_hist.argtypes = [ctypes.c_int, c_int_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]
    lib.ddcmi_debug_block_reduce.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_double_p]
    lib.ddcmi_debug_census_final.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.ddcmi_debug_kinetic_finish.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]
    lib.ddcmi_debug_mol_sum.argtypes = [ctypes.c_int, c_double_p, c_double_p]
    for f in (lib.ddcmi_debug_reduce_jobs, lib.ddcmi_debug_reduce_hist, lib.ddcmi_debug_reduce_gather, lib.ddcmi_debug_reduce_gather_hist,
              lib.ddcmi_debug_block_reduce, lib.ddcmi_debug_census_final, lib.ddcmi_debug_kinetic_finish, lib.ddcmi_debug_mol_sum):
        f.restype = ctypes.c_int
    return lib


def run_jobs(lib, fronts, rows0, nv0, rows1, nv1, disp_dt=(0.0, 0.0), disp0=(0.0, 0.0)):
    """out[nlaunch][2][8] (poisoned before every launch) and disp[nlaunch][2]"""
    fronts = np.asarray(fronts, dtype=np.int32)
    p0, p1 = np.ascontiguousarray(rows0, dtype=np.float64), np.ascontiguousarray(rows1, dtype=np.float64)
    assert p0.shape[1] == 8 and p1.shape[1] == 8
    nrows, nv = np.array([len(p0), len(p1)], np.int32), np.array([nv0, nv1], np.int32)
    out = np.full((len(fronts), 2, 8), POISON)
    disp = np.full((len(fronts), 2), POISON)
    rc = lib.ddcmi_debug_reduce_jobs(len(fronts), ip(fronts), ip(nrows), ip(nv), dp(p0), dp(p1), dp(np.array(disp_dt, np.float64)), dp(np.array(disp0, np.float64)),
                                     dp(out), dp(disp))
    assert rc == 0, rc
    return out, disp


def with_nan_columns(rows, nv):
    a = np.array(rows)
    a[:, nv:] = np.nan
    return a


def expect_out(rows, nv):
    e = np.full(8, POISON)
    e[:nv] = R.reduce_jobs(rows, nv)
    return e


def assert_bits(got, want, what):
    same = R.same_bits(got, want)
    assert np.all(same), (what, [(int(i), float(np.ravel(got)[i]).hex(), float(np.ravel(want)[i]).hex()) for i in np.nonzero(~np.ravel(same))[0][:6]])


@pytest.mark.parametrize("n", R.ROWS)
def test_reduce_jobs_sums(lib, n):
    """every set as job 0 with all eight columns and as job 1 with nv = 7 and 3 in turn (columns >= nv NaN), through both two-job front ends;
    the one-job front end on job 0.  Words >= nv of out keep their poison."""
    for i, (name, rows) in enumerate(R.make_rows(n)):
        nv1 = (7, 3)[i % 2]
        front = (FRONT_TWO, FRONT_IMAGES)[(i // 2) % 2]
        out, _ = run_jobs(lib, [front, FRONT_ONE], rows, 8, with_nan_columns(rows, nv1), nv1)
        assert_bits(out[0, 0], expect_out(rows, 8), (name, n, "job 0", front))
        assert_bits(out[0, 1], expect_out(rows, nv1), (name, n, "job 1", front, nv1))
        assert_bits(out[1, 0], expect_out(rows, 8), (name, n, "one job"))
        assert np.all(out[1, 1] == POISON), (name, n)
    # the sets did what they are there for
    sets = dict(R.make_rows(n))
    assert np.all(np.isnan(R.reduce_jobs(sets["nan_row"], 8)))
    if n >= 7:
        t = R.reduce_jobs(sets["inf_rows"], 8)
        assert t[0] == np.inf and t[1] == -np.inf and np.isnan(t[2])


@pytest.mark.parametrize("n", R.ROWS)
def test_reduce_gather_sums(lib, n):
    """k_reduce_gather on ten rows of n values at a stride beyond n (what lies between the rows is NaN), filed where finish_energy reads them;
    the words the kernel clears are zero and the two it does not own keep their poison"""
    pstride = n + 5
    for name, rows in R.make_rows(n, ncol=R.GB_NV):
        part = np.full((R.GB_NV, pstride), np.nan)
        part[:, :n] = rows.T
        out = np.full(24, POISON)
        assert lib.ddcmi_debug_reduce_gather(n, pstride, dp(part), dp(out)) == 0
        s = [R.reduce_gather(rows[:, k]) for k in range(R.GB_NV)]
        want = np.array([s[0]] + s[4:10] + [POISON] + [s[1]] + [0.0] * 6 + [POISON] + [s[2], s[3]] + [0.0] * 6)
        assert_bits(out, want, (name, n))


@pytest.mark.parametrize("n", (1, 129, 1024, 1025, 4097, 8193))
def test_column_seven_as_a_maximum(lib, n):
    """The largest |v|^2 in every edge row in turn, a NaN in another row of the column: the displacement word moves by d with
    exact <= d <= exact (1 + 2e-7), exact = disp_dt sqrt(max) -- the lower bound is what the shell-limited walk stands on; the sums of the
    other seven columns are the restatement's; with nv = 0 (the pre-step's job) out is left alone.  Not bit for bit: the compiler may
    contract the last multiply-add.  The NaN drops out of the maximum (fmax)."""
    decimal.getcontext().prec = 60
    rng = np.random.default_rng(n)
    dt, start = (0.0123, 3.5), (0.0, 0.375)
    for r in R.edge_rows(n):
        rows = rng.standard_normal((n, 8))
        rows[:, 7] = rng.uniform(0.0, 4.0, n).astype(np.float32)
        rows[r, 7] = np.float32(4.0 + rng.uniform(0.0, 60.0))
        if n > 1:
            rows[(r + n // 2) % n, 7] = np.nan
        vmax = R.reduce_jobs_max(rows)
        assert vmax == rows[r, 7]
        other = np.array(rows); other[:, :7] = np.nan      # job 1: nv = 0, nothing but the maximum is read
        out, disp = run_jobs(lib, [FRONT_TWO, FRONT_IMAGES, FRONT_ONE], rows, 7, other, 0, disp_dt=dt, disp0=start)
        for l in range(3):
            assert_bits(out[l, 0], expect_out(rows, 7), (n, r, l))
        assert np.all(out[:, 1] == POISON), (n, r)
        before = [decimal.Decimal(start[0]), decimal.Decimal(start[1])]
        for l, jobs in enumerate(((0, 1), (0, 1), (0,))):
            for q in (0, 1):
                now = decimal.Decimal(float(disp[l, q]))
                d = now - before[q]
                if q in jobs:
                    exact = decimal.Decimal(dt[q]) * decimal.Decimal(vmax).sqrt()
                    print("n %d row %d launch %d job %d: d / exact - 1 = %.3e" % (n, r, l, q, float(d / exact - 1)))
                    assert exact <= d <= exact * (1 + decimal.Decimal("2e-7")), (n, r, l, q, float(d), float(exact))
                else:
                    assert d == 0, (n, r, l, q)
                before[q] = now


def test_tickets_repeat_and_interleave(lib):
    """the same jobs three times on one scratch array, then one-job and two-job launches interleaved as a step does it: the same bits every time
    (a ticket left at anything but zero would leave a later launch without a last workgroup, and its out[] poisoned)"""
    a, b = dict(R.make_rows(4097))["spread"], dict(R.make_rows(1025, seed=1))["spread"]
    fronts = [FRONT_TWO] * 3 + [FRONT_ONE, FRONT_TWO, FRONT_ONE, FRONT_IMAGES, FRONT_ONE, FRONT_ONE, FRONT_IMAGES, FRONT_TWO]
    out, _ = run_jobs(lib, fronts, a, 8, with_nan_columns(b, 7), 7)
    for l, f in enumerate(fronts):
        assert_bits(out[l, 0], expect_out(a, 8), (l, f))
        assert_bits(out[l, 1], expect_out(b, 7) if f != FRONT_ONE else np.full(8, POISON), (l, f))


SEQUENCES = ((1,), (32,), (15, 7), (32, 5, 32, 1), (1, 2, 3), (7, 7))


@pytest.mark.parametrize("seq", SEQUENCES, ids=lambda s: "-".join(map(str, s)))
def test_history_sequences(lib, seq):
    """Flushes of seq[i] pending steps on one scratch array: words 0..7 of every step are the pair job's sums and words 8..14 the kinetic job's,
    with the bits k_reduce_jobs forms from the same rows (and the restatement's); word 15 and beyond keep the poison, no other word does.
    With the tickets at tmp + 128 * nsteps (the parent of this commit) a flush of fewer steps than an earlier one found its tickets in that
    one's rows, no workgroup was the last, and its steps kept the poison: (15, 7) and (32, 5, 32, 1) failed so on an MI355X.  (7, 7) and
    (1, 2, 3) passed there too: equal counts share the place, and a longer flush finds its tickets in words no row has reached."""
    nrows, stride = 129, 129 * 8 + 24
    rng = np.random.default_rng(sum(seq) * 100 + len(seq))
    total = sum(seq)
    pair = np.full((total, stride), np.nan)
    kin = np.full((total, stride), np.nan)
    steps = []
    for q in range(total):
        p = np.ldexp(rng.uniform(1.0, 2.0, (nrows, 8)), rng.integers(-30, 31, (nrows, 8))) * rng.choice([-1.0, 1.0], (nrows, 8))
        k = with_nan_columns(np.ldexp(rng.uniform(1.0, 2.0, (nrows, 8)), rng.integers(-30, 31, (nrows, 8))), 7)
        pair[q, :nrows * 8] = p.ravel(); kin[q, :nrows * 8] = k.ravel()
        steps.append((p, k))
    hist = np.full((total, R.LEAN_HW), POISON)
    ns = np.array(seq, np.int32)
    assert lib.ddcmi_debug_reduce_hist(len(seq), ip(ns), nrows, stride, dp(pair), dp(kin), dp(hist)) == 0
    want = np.full((total, R.LEAN_HW), POISON)
    for q, (p, k) in enumerate(steps):
        want[q, 0:8] = R.reduce_jobs(p, 8)
        want[q, 8:15] = R.reduce_jobs(k, 7)
    stale = [q for q in range(total) if np.any(hist[q, :15] == POISON)]
    assert not stale, ("steps left poisoned", seq, stale)
    assert_bits(hist, want, seq)
    # ... and the per-step launch itself on the first and the last step
    for q in (0, total - 1):
        out, _ = run_jobs(lib, [FRONT_TWO], steps[q][0], 8, steps[q][1], 7)
        assert_bits(hist[q, 0:8], out[0, 0], (seq, q)); assert_bits(hist[q, 8:15], out[0, 1, :7], (seq, q))


@pytest.mark.parametrize("seq", SEQUENCES, ids=lambda s: "-".join(map(str, s)))
def test_gather_history_sequences(lib, seq):
    """k_reduce_gather_hist: words 16..25 of every step of every flush are the bits k_reduce_gather forms from the same rows"""
    n, pstride = 129, 131      # (the row counts are test_reduce_gather_sums's; this is about the steps and the flushes)
    total = sum(seq)
    rng = np.random.default_rng(sum(seq) * 100 + len(seq) + 1)
    part = np.full((total, R.GB_NV, pstride), np.nan)
    part[:, :, :n] = np.ldexp(rng.uniform(1.0, 2.0, (total, R.GB_NV, n)), rng.integers(-30, 31, (total, R.GB_NV, n))) * rng.choice([-1.0, 1.0], (total, R.GB_NV, n))
    hist = np.full((total, R.LEAN_HW), POISON)
    assert lib.ddcmi_debug_reduce_gather_hist(len(seq), ip(np.array(seq, np.int32)), n, pstride, dp(part), dp(hist)) == 0
    want = np.full((total, R.LEAN_HW), POISON)
    for q in range(total):
        want[q, 16:26] = [R.reduce_gather(part[q, k, :n]) for k in range(R.GB_NV)]
    assert_bits(hist, want, seq)
    for q in (0, total - 1):
        out = np.full(24, POISON)
        assert lib.ddcmi_debug_reduce_gather(n, pstride, dp(np.ascontiguousarray(part[q])), dp(out)) == 0
        assert_bits(np.concatenate([out[[0, 8, 16, 17]], out[1:7]]), hist[q, 16:26], (seq, q))


@pytest.mark.parametrize("which,nv", [(0, 7), (1, 3), (2, 12)])
def test_block_reduce_store(lib, which, nv):
    """block_reduce_store<NV, 4>: every wave in the order of wave_sum (shuffle down by 32 ... 1; not tree64, the order of the DPP butterfly
    wave_sum_dpp, which this routine does not use: test_reductions_host shows that the two orders differ), then the waves in wave order.  One block per set; words >= NV of a block's 16 keep the poison."""
    sets = R.make_rows(R.BLOCK, ncol=nv)
    inp = np.ascontiguousarray(np.stack([rows for _, rows in sets]))
    out = np.full((len(sets), 16), POISON)
    assert lib.ddcmi_debug_block_reduce(which, len(sets), inp.ctypes.data_as(ctypes.c_void_p), dp(out)) == 0
    want = np.full((len(sets), 16), POISON)
    for i, (_, rows) in enumerate(sets):
        want[i, :nv] = R.block_reduce(rows)
    assert_bits(out, want, [name for name, _ in sets])


@pytest.mark.parametrize("which", (3, 4))
def test_block_vmax_store(lib, which):
    """block_vmax_store: the exact maximum of 256 non-negative floats in word 7 -- the largest in every lane of a wave edge in turn, in the
    last lane of the last wave, an all-zero block, +inf, subnormal floats -- and no other word written"""
    rng = np.random.default_rng(which)
    blocks = []
    for lane in (0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 191, 192, 254, 255):
        a = rng.uniform(0.0, 1.0, R.BLOCK).astype(np.float32)
        a[lane] = np.float32(1.0 + lane)
        blocks.append(a)
    blocks.append(np.zeros(R.BLOCK, np.float32))
    a = rng.uniform(0.0, 1.0, R.BLOCK).astype(np.float32); a[200] = np.inf
    blocks.append(a)
    blocks.append((rng.integers(0, 2 ** 20, R.BLOCK) * np.float32(1e-45).astype(np.float64)).astype(np.float32))
    a = rng.uniform(0.0, 1.0, R.BLOCK).astype(np.float32); a[77] = np.nextafter(np.float32(1.0), np.float32(2.0)); a[78] = 1.0
    blocks.append(a)
    inp = np.ascontiguousarray(np.stack(blocks), dtype=np.float32)
    out = np.full((len(blocks), 16), POISON)
    assert lib.ddcmi_debug_block_reduce(which, len(blocks), inp.ctypes.data_as(ctypes.c_void_p), dp(out)) == 0
    want = np.full((len(blocks), 16), POISON)
    want[:, 7] = inp.max(axis=1).astype(np.float64)
    assert_bits(out, want, which)
    assert out[-4, 7] == 0.0 and out[-3, 7] == np.inf and 0.0 < out[-2, 7] < 2.0 ** -126


@pytest.mark.parametrize("nwg", (1, 2, 1023, 1024))
def test_census_final(lib, nwg):
    """k_census_final: the workgroups' rows in workgroup order starting from row 0, all three instantiations; the minimum and maximum columns of
    RowsSumMinMax exact; every count 0xffffffff: the 64-bit total exact (as an integer, and as the double the zdensity pass asks for)"""
    nd, nc = 66, 5      # (two workgroups of the finisher, the second partly filled)
    cnt = np.full((nwg, nc), 0xffffffff, np.uint32)
    cnt[:, 1] = np.arange(nwg)
    for name, rows in R.make_rows(nwg, ncol=nd):
        for which in (0, 1, 2):
            od = np.full(nd, POISON)
            oc = np.full(nc, POISON) if which == 0 else np.full(nc, -7, np.int64)
            assert lib.ddcmi_debug_census_final(which, nwg, nd, dp(rows), dp(od), nc, cnt.ctypes.data_as(ctypes.c_void_p), oc.ctypes.data_as(ctypes.c_void_p)) == 0
            assert_bits(od, R.rows_in_order(rows, False) if which < 2 else R.census_sum_min_max(rows), (name, nwg, which))
            if which == 2 and np.all(np.isfinite(rows)):
                assert np.array_equal(od[1::3], rows[:, 1::3].min(axis=0)) and np.array_equal(od[2::3], rows[:, 2::3].max(axis=0)), name
            tot = [nwg * 0xffffffff, nwg * (nwg - 1) // 2] + [nwg * 0xffffffff] * 3
            assert [int(x) for x in oc] == tot, (name, nwg, which, oc)
    # either part may be empty: the output of the other is left alone
    od, oc = np.full(nd, POISON), np.full(nc, -7, np.int64)
    rows = dict(R.make_rows(nwg, ncol=nd))["spread"]
    assert lib.ddcmi_debug_census_final(1, nwg, nd, dp(rows), dp(od), 0, None, None) == 0
    assert_bits(od, R.rows_in_order(rows, False), nwg)
    assert lib.ddcmi_debug_census_final(1, nwg, 0, None, None, nc, cnt.ctypes.data_as(ctypes.c_void_p), oc.ctypes.data_as(ctypes.c_void_p)) == 0
    assert int(oc[0]) == nwg * 0xffffffff


def test_plain_finishers(lib):
    """k_group_ke_sum on [512][2 n], k_class_kinetic_sum on [512][n][16] (columns 12..15 NaN) and k_mol_sum on [nblk][3]: row order from +0.0"""
    for n in (1, 3, 32):
        for name, rows in R.make_rows(R.GKE_BLOCKS, ncol=2 * n):
            out = np.full(2 * n, POISON)
            assert lib.ddcmi_debug_kinetic_finish(0, n, dp(rows), dp(out)) == 0
            assert_bits(out, R.rows_in_order(rows, True), (name, n))
    for n in (1, 3, 11):
        for name, rows in R.make_rows(R.GKE_BLOCKS, ncol=16 * n):
            rows = rows.reshape(R.GKE_BLOCKS, n, 16).copy()
            rows[:, :, R.KD_NV:] = np.nan
            out = np.full((n, R.KD_NV), POISON)
            assert lib.ddcmi_debug_kinetic_finish(1, n, dp(rows), dp(out)) == 0
            assert_bits(out, R.rows_in_order(rows, True)[:, :R.KD_NV], (name, n))
    for nblk in (1, 2, 63, 64, 65, 1000):
        for name, rows in R.make_rows(nblk, ncol=3):
            out = np.full(3, POISON)
            assert lib.ddcmi_debug_mol_sum(nblk, dp(rows), dp(out)) == 0
            assert_bits(out, R.rows_in_order(rows, True), (name, nblk))


def test_bad_arguments(lib):
    a, o = np.zeros(8 * 64), np.full(64, POISON)
    one, two = np.array([0], np.int32), np.array([4, 4], np.int32)
    zero2 = np.zeros(2)

    def jobs(nlaunch=1, front=0, nrows=(4, 4), nv=(8, 7), dt=(0.0, 0.0), p0=a):
        return lib.ddcmi_debug_reduce_jobs(nlaunch, ip(np.array([front], np.int32)), ip(np.array(nrows, np.int32)), ip(np.array(nv, np.int32)),
                                           dp(p0) if p0 is not None else None, dp(a), dp(np.array(dt, np.float64)), dp(zero2), dp(o), dp(np.zeros(2)))
    assert jobs() == 0
    for kw in (dict(nlaunch=0), dict(nlaunch=65), dict(front=3), dict(front=-1), dict(nrows=(0, 4)), dict(nrows=(4, -1)), dict(nrows=(4, 2 ** 20 + 1)),
               dict(nv=(9, 7)), dict(nv=(8, 5)), dict(nv=(-1, 7)), dict(dt=(-1.0, 0.0)), dict(dt=(0.0, np.nan)), dict(dt=(1.0, 0.0)), dict(p0=None)):
        assert jobs(**kw) == EINVAL, kw
    h = np.full(32 * 64, POISON)
    f = lib.ddcmi_debug_reduce_hist
    assert f(1, ip(one + 1), 4, 32, dp(a), dp(a), dp(h)) == 0
    for args in ((0, ip(one + 1), 4, 32), (17, ip(one + 1), 4, 32), (1, ip(one), 4, 32), (1, ip(one + 33), 4, 32), (1, ip(one + 1), 0, 32), (1, ip(one + 1), 8193, 2 ** 17),
                 (1, ip(one + 1), 4, 31), (1, ip(one + 1), 4, 2 ** 17 + 1), (1, None, 4, 32)):
        assert f(*args, dp(a), dp(a), dp(h)) == EINVAL, args[:1] + args[2:]
    g = lib.ddcmi_debug_reduce_gather
    assert g(4, 8, dp(a), dp(o)) == 0
    for n, ps in ((0, 8), (-1, 8), (9, 8), (4, 2 ** 20 + 1)):
        assert g(n, ps, dp(a), dp(o)) == EINVAL, (n, ps)
    assert g(4, 8, None, dp(o)) == EINVAL
    g = lib.ddcmi_debug_reduce_gather_hist
    assert g(1, ip(one + 1), 4, 8, dp(a), dp(h)) == 0
    for args in ((0, ip(one + 1), 4, 8), (1, ip(one), 4, 8), (1, ip(one + 33), 4, 8), (1, ip(one + 1), 0, 8), (1, ip(one + 1), 9, 8), (1, ip(one + 1), 4, 2 ** 13 + 1)):
        assert g(*args, dp(a), dp(h)) == EINVAL, args[2:]
    b = np.zeros(256 * 12)
    f = lib.ddcmi_debug_block_reduce
    for which, nb in ((-1, 1), (5, 1), (0, 0), (0, 4097)):
        assert f(which, nb, b.ctypes.data_as(ctypes.c_void_p), dp(o)) == EINVAL, (which, nb)
    for bad in (-1.0, np.nan):
        v = np.zeros(256, np.float32); v[100] = bad
        assert f(3, 1, v.ctypes.data_as(ctypes.c_void_p), dp(o)) == EINVAL, bad
    assert f(0, 1, None, dp(o)) == EINVAL
    f = lib.ddcmi_debug_census_final
    c = np.zeros(64, np.uint32)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert f(0, 2, 4, dp(a), dp(o), 4, vp(c), vp(o)) == 0
    for which, nwg, nd, nc in ((3, 2, 4, 4), (-1, 2, 4, 4), (0, 0, 4, 4), (0, 2049, 4, 4), (0, 2, -1, 4), (0, 2, 4, -1), (0, 2, 0, 0), (0, 2, 65537, 0)):
        assert f(which, nwg, nd, dp(a), dp(o), nc, vp(c), vp(o)) == EINVAL, (which, nwg, nd, nc)
    assert f(0, 2, 4, None, dp(o), 0, None, None) == EINVAL and f(0, 2, 0, None, None, 4, vp(c), None) == EINVAL
    f = lib.ddcmi_debug_kinetic_finish
    big = np.zeros(512 * 16)
    for which, n in ((-1, 1), (2, 1), (0, 0), (0, 33), (1, 0), (1, 65)):
        assert f(which, n, dp(big), dp(o)) == EINVAL, (which, n)
    f = lib.ddcmi_debug_mol_sum
    for n in (0, -1, 2 ** 20 + 1):
        assert f(n, dp(a), dp(o)) == EINVAL, n
    assert f(1, None, dp(o)) == EINVAL

"""Plain numpy restatements of the cross-workgroup reductions (the level above the wave), and the row sets the tests feed them.

Each function restates the ORDER of the additions of one device routine, as test_gpu_wave_reduce.tree64 restates the wave's: IEEE double
addition is commutative and numpy adds without contraction, so a restatement is exact -- the device must give its bits -- and not a bound.
tests/test_reductions_host.py holds every restatement against math.fsum; tests/test_gpu_reductions.py holds the device against them.

The constants mirror the device code (ddcmi_integrator.inl, bonded.hip, ddcmi_internal.h); a test that feeds the hooks of include/ddcmi_test.h
arrays shaped by them fails loudly if one of them moves."""
import math

import numpy as np

U = 2.0 ** -53
RED_SPLIT = 8            # workgroups that share a job of reduce_jobs_block
RED_GROUPS = 128         # row groups of one such workgroup (1024 threads / 8 columns)
RG_T = 1024              # threads of reduce_gather_row
GB_NV = 10               # sums of the bonded kernels
LEAN_W, LEAN_HW = 32, 32
GKE_BLOCKS, KD_NV = 512, 12
BLOCK = 256              # DDCMI_BLOCK: four waves
ROWS = (1, 7, 8, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 5121, 8191, 8193)
EDGE_ROWS = (0, 127, 128, 1023, 1024, -1)


def _quiet():
    return np.errstate(invalid="ignore", over="ignore")


def _four_way(x, nthreads):
    """x[n][...]: thread t of nthreads takes elements t, t + nthreads, ...; its m-th element goes to partial sum m % 4 -- the main loop adds four
    per trip, the tail of at most three goes to p[0 ...] -- each partial sum in sequence from +0.0; the thread's sum is (p0 + p1) + (p2 + p3).
    Rows of +0.0 fill the last trip: p + 0.0 is p bit for bit (p is never -0.0: it starts at +0.0 and a sum that cancels is +0.0).
    Returns [nthreads][...]."""
    n = x.shape[0]
    trips = max(1, -(-n // (4 * nthreads)))
    pad = np.zeros((trips * 4 * nthreads,) + x.shape[1:])
    pad[:n] = x
    pad = pad.reshape((trips, 4, nthreads) + x.shape[1:])
    p = np.zeros((4, nthreads) + x.shape[1:])
    with _quiet():
        for t in range(trips):
            p = p + pad[t]
        return (p[0] + p[1]) + (p[2] + p[3])


def _halving_tree(a, first):
    """s[t] += s[t + off] for t < off, off = first, first / 2, ... 1 along axis 0; returns s[0]"""
    a = np.array(a)
    off = first
    with _quiet():
        while off >= 1:
            a[:off] = a[:off] + a[off:2 * off]
            off //= 2
    return a[0]


def reduce_jobs_tmp(rows, nv):
    """the rows the RED_SPLIT workgroups of reduce_jobs_block leave in tmp: [RED_SPLIT][nv].  Workgroup bx, row group g: rows g + 128 bx,
    + 1024, ... four-way; then the LDS tree over the 128 row groups (off = 512 ... 8 in threads is 64 ... 1 in row groups)."""
    rows = np.asarray(rows, dtype=np.float64)[:, :nv]
    a = _four_way(rows, RED_SPLIT * RED_GROUPS).reshape(RED_SPLIT, RED_GROUPS, nv)
    return np.stack([_halving_tree(a[bx], RED_GROUPS // 2) for bx in range(RED_SPLIT)])


def reduce_jobs(rows, nv):
    """out[nv] of reduce_jobs_block: the last workgroup adds the RED_SPLIT rows of tmp in index order, starting from +0.0"""
    tmp = reduce_jobs_tmp(rows, nv)
    t = np.zeros(nv)
    with _quiet():
        for q in range(RED_SPLIT):
            t = t + tmp[q]
    return t


def reduce_jobs_max(rows):
    """column 7 as a maximum: fmax from +0.0 at every level.  fmax returns the other operand where one is NaN, so a NaN row drops out, and
    a maximum does not depend on the order"""
    return float(np.fmax.reduce(np.asarray(rows, dtype=np.float64)[:, 7], initial=0.0))


def reduce_gather(row):
    """reduce_gather_row on row[nblocks]: thread t takes t, t + 1024, ... four-way, then the tree off = 512 ... 1"""
    return float(_halving_tree(_four_way(np.asarray(row, dtype=np.float64), RG_T), RG_T // 2))


def wave_sum_shfl(col):
    """wave_sum (ddcmi.hip) as lane 0 gets it: v += shfl_down(v, off) for off = 32 ... 1.  This is what block_reduce_store reduces a wave with
    -- not the DPP butterfly of wave_sum_dpp, whose order (tree64) differs from it"""
    return _halving_tree(np.asarray(col, dtype=np.float64), 32)


def block_reduce(vals):
    """block_reduce_store<NV, 4> on vals[256][NV]: every wave by wave_sum, then the four waves in wave order starting from wave 0's sum"""
    vals = np.asarray(vals, dtype=np.float64)
    w = [wave_sum_shfl(vals[64 * q:64 * q + 64]) for q in range(vals.shape[0] // 64)]
    a = w[0]
    with _quiet():
        for s in w[1:]:
            a = a + s
    return a


def rows_in_order(rows, from_zero):
    """rows[n][...] added in row order: from +0.0 (k_group_ke_sum, k_class_kinetic_sum, k_mol_sum) or from row 0 (k_census_final)"""
    rows = np.asarray(rows, dtype=np.float64)
    t = np.zeros(rows.shape[1:]) if from_zero else rows[0].copy()
    with _quiet():
        for r in rows[0 if from_zero else 1:]:
            t = t + r
    return t


def census_sum_min_max(rows):
    """k_census_final<RowsSumMinMax>: value k is a sum, a minimum or a maximum by k % 3; the extrema are comparisons o < t ? o : t, which a
    NaN that arrives as o loses"""
    rows = np.asarray(rows, dtype=np.float64)
    t = rows[0].copy()
    q = np.arange(rows.shape[1]) % 3
    with _quiet():
        for o in rows[1:]:
            t = np.where(q == 0, t + o, np.where(q == 1, np.where(o < t, o, t), np.where(o > t, o, t)))
    return t


# how many additions the longest chain from an input to the result passes through: the error of the result is at most
# ((1 + u)^depth - 1) sum |x| <= depth u (1 + depth u) sum |x| (every addition multiplies what passes through it by at most 1 + u)
def depth_reduce_jobs(n):
    """a partial sum takes ceil(ceil(n / 1024) / 4) elements (the first addition, to +0.0, is exact but counted), two more for
    (p0 + p1) + (p2 + p3), seven levels of the tree over 128 row groups, eight additions of the final loop (the first to +0.0)"""
    return -(-(-(-n // 1024)) // 4) + 2 + 7 + 8


def depth_reduce_gather(n):
    """as above with a tree of ten levels over 1024 threads and no final loop"""
    return -(-(-(-n // 1024)) // 4) + 2 + 10


DEPTH_BLOCK_REDUCE = 6 + 3      # six shuffle steps, then three additions over the four waves


def bound(depth, col):
    return depth * U * (1.0 + depth * U) * math.fsum(np.abs(col))


def same_bits(a, b):
    """elementwise: the same 64 bits, or both NaN (a NaN's payload is not compared)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(np.uint64) == b.view(np.uint64)))


def edge_rows(n):
    """the rows of EDGE_ROWS that n rows have: first and last row of a workgroup's share, of a stride, and the last row"""
    return sorted(set((r if r >= 0 else n - 1) for r in EDGE_ROWS if r < n))


def make_rows(n, ncol=8, seed=0):
    """the sets of test_gpu_wave_reduce.make_sets widened to n rows of ncol columns: a list of (name, rows[n][ncol])"""
    rng = np.random.default_rng(20261020 + 7919 * n + 104729 * ncol + seed)
    out = []

    def sign():
        return rng.choice([-1.0, 1.0], (n, ncol))

    out.append(("normal", rng.standard_normal((n, ncol))))
    out.append(("spread", np.ldexp(rng.uniform(1.0, 2.0, (n, ncol)), rng.integers(-60, 61, (n, ncol))) * sign()))
    # exact cancellations: multiples of 2^-10 below 2^30 and their negatives in a random row order -- every partial sum of every order is
    # exact, so every order gives exactly 0
    half = rng.integers(1, 2 ** 40, (n // 2, ncol)).astype(np.float64) * 2.0 ** -10
    a = np.concatenate([half, -half, np.zeros((n % 2, ncol))])
    out.append(("cancel", np.stack([a[rng.permutation(n), k] for k in range(ncol)], axis=1)))
    out.append(("minus_zero", np.full((n, ncol), -0.0)))
    out.append(("mixed_zero", np.where(rng.integers(0, 2, (n, ncol)) == 1, -0.0, 0.0)))
    out.append(("subnormal", rng.integers(-2 ** 36, 2 ** 36, (n, ncol)).astype(np.float64) * 5e-324))
    out.append(("subnormal_edge", np.ldexp(rng.uniform(1.0, 2.0, (n, ncol)), rng.integers(-1074, -1018, (n, ncol))) * sign()))
    a = rng.standard_normal((n, ncol))
    a[(2 * n) // 3] = np.nan
    out.append(("nan_row", a))
    # a +inf row and a -inf row: column k keeps +inf alone if k % 3 == 0, -inf alone if k % 3 == 1 and both otherwise (inf - inf: a NaN the
    # additions make themselves; with one row the -inf row wins)
    a = rng.standard_normal((n, ncol))
    rp, rm = n // 3, (n - 1) - n // 5
    for k in range(ncol):
        if k % 3 != 1: a[rp, k] = np.inf
        if k % 3 != 0: a[rm, k] = -np.inf
    out.append(("inf_rows", a))
    # all rows equal, 24 significant bits: every multiple up to 2^29 of it is exact, so every order gives n c
    c = rng.uniform(1.0, 2.0, ncol).astype(np.float32).astype(np.float64) * np.ldexp(1.0, rng.integers(-30, 31, ncol)) * rng.choice([-1.0, 1.0], ncol)
    out.append(("equal", np.tile(c, (n, 1))))
    for r in edge_rows(n):
        a = np.zeros((n, ncol))
        a[r] = [(k + 1.5) * (-1.0) ** k * math.pi for k in range(ncol)]
        out.append(("one_hot%d" % r, a))
    # one thread's rows alone: rows t, t + 1024, ... are random, every other row is zero, so the result is that thread's sum and nothing
    # rounds its last bits away -- the four partial sums of the thread, which element of the tail goes to which, show bit for bit.  At the
    # row counts of ROWS a tail of two or three rows behind a full trip belongs to one thread alone (5121: thread 0; 8191: thread 1023, the
    # first that has a row fewer than the last row's thread)
    for t in sorted({0, (n - 1) % 1024, n % 1024}) if n > 1024 else ():
        a = np.zeros((n, ncol))
        a[t::1024] = rng.standard_normal((len(range(t, n, 1024)), ncol))
        out.append(("one_thread%d" % t, a))
    return [(name, np.ascontiguousarray(a, dtype=np.float64)) for name, a in out]

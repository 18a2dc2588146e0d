"""wave_sum_multi_dpp<N> (ddcmi.hip) -- N sums over a wave in one transposed pass -- against wave_sum_dpp, bit for bit.

The pair kernel's epilogue forms its seven kinetic sums and its eight energy / virial sums per wave with the transposed routine; the
bit-for-bit tests of the project (fused against split, lean against reduction launch, batched against single steps) stand on it giving
every sum the bits of wave_sum_dpp.  ddcmi_debug_wave_reduce (include/ddcmi_test.h) runs both on the test's own numbers: one 64-thread
workgroup per set of in[64][N].

What is held, for N in {1, 2, 3, 7, 8, 15, 16}, compared as uint64:
  * the two device routines agree on every column of every set (where a sum is NaN both are NaN; a NaN's payload is not compared);
  * both agree with tree64 below, a numpy restatement of the order itself: partner lane ^ 1, lane ^ 2, row_half_mirror (lane ^ 7),
    row_mirror (lane ^ 15) inside the rows of 16, then (r1 + r0) + (r3 + r2) -- IEEE double addition is commutative and numpy adds
    without contraction, so the restatement is exact, not a bound.
Sets: random normals; magnitudes 2^-60 ... 2^60 with mixed signs (association matters: a regrouped sum differs in the last bits, often
in all of them); exact cancellations; -0.0; subnormals; one NaN lane and one +-inf lane; all-equal columns; a column that is non-zero in
exactly one lane, one set for each of the 64 lanes (each column of the set in a lane of its own).

test_tree64_host runs without a GPU: the restatement against math.fsum.  A sum of 64 terms through a tree of depth 6 is off by at most
((1 + u)^6 - 1) sum |x| <= 6 u (1 + 3 u) sum |x|, u = 2^-53 (each level multiplies what passes through it by at most 1 + u), and it is
exact on one-lane columns, exact cancellations and equal columns (64 c: five doublings and one more)."""
import ctypes
import math

import numpy as np
import pytest

NS = (1, 2, 3, 7, 8, 15, 16)
U = 2.0 ** -53


def tree64(col):
    """the reduction order of wave_reduce_dpp<WaveSum> on one column of 64 doubles"""
    lane = np.arange(64)
    v = np.array(col, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in (1, 2, 7, 15):
            v = v + v[lane ^ x]
        return (v[0] + v[16]) + (v[32] + v[48])


def make_sets(n):
    """[nsets][64][n] doubles and the names of the sets"""
    rng = np.random.default_rng(20261019 + n)
    sets, names = [], []

    def add(name, a):
        sets.append(np.ascontiguousarray(a, dtype=np.float64).reshape(64, n))
        names.append(name)

    for r in range(2):
        add("normal%d" % r, rng.standard_normal((64, n)))
    for r in range(2):
        add("spread%d" % r, np.ldexp(rng.uniform(1.0, 2.0, (64, n)), rng.integers(-60, 61, (64, n))) * rng.choice([-1.0, 1.0], (64, n)))
    # exact cancellations: 32 values and their negatives in a random lane order (the exact sum is 0; the tree's is whatever the tree gives),
    # and partner lanes that cancel in the first step
    half = np.ldexp(rng.uniform(1.0, 2.0, (32, n)), rng.integers(-40, 41, (32, n)))
    a = np.concatenate([half, -half])
    add("cancel_shuffled", np.stack([a[rng.permutation(64), k] for k in range(n)], axis=1))
    a = np.empty((64, n)); a[0::2] = half; a[1::2] = -half
    add("cancel_pairs", a)
    add("minus_zero", np.full((64, n), -0.0))
    add("mixed_zero", np.where(rng.integers(0, 2, (64, n)) == 1, -0.0, 0.0))
    add("subnormal", rng.integers(-2 ** 40, 2 ** 40, (64, n)).astype(np.float64) * 5e-324)
    add("subnormal_edge", np.ldexp(rng.uniform(1.0, 2.0, (64, n)), rng.integers(-1074, -1018, (64, n))) * rng.choice([-1.0, 1.0], (64, n)))
    # one NaN lane and one inf lane: column k has its NaN in lane (3 k + 1) % 64 if k % 3 == 0, +inf in lane (5 k + 2) % 64 if k % 3 == 1, -inf there
    # if k % 3 == 2; the second set gives every column +inf and -inf in two lanes (a NaN the additions make themselves)
    a = rng.standard_normal((64, n))
    for k in range(n):
        if k % 3 == 0: a[(3 * k + 1) % 64, k] = np.nan
        elif k % 3 == 1: a[(5 * k + 2) % 64, k] = np.inf
        else: a[(5 * k + 2) % 64, k] = -np.inf
    add("nan_inf", a)
    a = rng.standard_normal((64, n))
    for k in range(n):
        a[(7 * k + 3) % 64, k] = np.inf
        a[(7 * k + 36) % 64, k] = -np.inf
    add("inf_minus_inf", a)
    add("equal", np.tile(np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-30, 31, n)) * rng.choice([-1.0, 1.0], n), (64, 1)))
    for l in range(64):
        a = np.zeros((64, n))
        for k in range(n):
            a[(l + 5 * k) % 64, k] = (k + 1.5) * (-1.0) ** k * math.pi
        add("one_lane%d" % l, a)
    return np.stack(sets), names


@pytest.mark.parametrize("n", NS)
def test_tree64_host(n):
    sets, names = make_sets(n)
    for s, name in zip(sets, names):
        for k in range(n):
            col = s[:, k]
            t = tree64(col)
            if not np.all(np.isfinite(col)):
                assert np.isnan(t) or np.isinf(t), (name, k)
                continue
            exact = math.fsum(col)
            bound = 6.0 * U * (1.0 + 3.0 * U) * math.fsum(np.abs(col))
            assert abs(t - exact) <= bound, (name, k, t, exact, bound)
            if name.startswith("one_lane") or name == "cancel_pairs":
                assert t == exact, (name, k, t, exact)
            if name == "equal":
                assert t == 64.0 * col[0], (name, k)
            if name == "minus_zero":
                assert t == 0.0 and math.copysign(1.0, t) < 0.0, (name, k)
    # the order is the tree's and no other: on the spread sets the lane-order sum differs from it somewhere
    spread = sets[names.index("spread0")]
    if n >= 2:
        assert any(float(np.cumsum(spread[:, k])[-1]) != float(tree64(spread[:, k])) for k in range(n))


def _run_device(n, sets):
    import ddcmd_amd._lib as L
    lib = L.load_test_library()
    f = lib.ddcmi_debug_wave_reduce
    f.restype = ctypes.c_int
    dp = ctypes.POINTER(ctypes.c_double)
    f.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp]
    nsets = sets.shape[0]
    inp = np.ascontiguousarray(sets, dtype=np.float64)
    single = np.full((nsets, n), 12345.0)
    multi = np.full((nsets, n), 54321.0)
    rc = f(n, nsets, inp.ctypes.data_as(dp), single.ctypes.data_as(dp), multi.ctypes.data_as(dp))
    assert rc == 0, rc
    return single, multi


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_multi_matches_single_and_tree(built, n):
    sets, names = make_sets(n)
    single, multi = _run_device(n, sets)
    ref = np.array([[tree64(s[:, k]) for k in range(n)] for s in sets])
    bad = []
    for what, a, b in (("multi vs single", multi, single), ("single vs tree64", single, ref), ("multi vs tree64", multi, ref)):
        na, nb = np.isnan(a), np.isnan(b)
        same = (na & nb) | (~na & ~nb & (a.view(np.uint64) == b.view(np.uint64)))
        for i, k in zip(*np.nonzero(~same)):
            bad.append((what, names[i], int(k), float(a[i, k]).hex(), float(b[i, k]).hex()))
    assert not bad, bad[:8]
    # the sets did what they are there for: a NaN from the NaN lane and one made of inf - inf, infinities of both signs, -0.0
    assert np.isnan(single[names.index("nan_inf"), 0]) and np.all(np.isnan(single[names.index("inf_minus_inf")]))
    if n >= 3:
        assert single[names.index("nan_inf"), 1] == np.inf and single[names.index("nan_inf"), 2] == -np.inf
    assert np.all(np.signbit(multi[names.index("minus_zero")]))


@pytest.mark.gpu
def test_bad_arguments(built):
    import ddcmd_amd._lib as L
    lib = L.load_test_library()
    f = lib.ddcmi_debug_wave_reduce
    f.restype = ctypes.c_int
    dp = ctypes.POINTER(ctypes.c_double)
    f.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp]
    a = np.zeros(64 * 17)
    o = np.zeros(17)
    for n, nsets in ((0, 1), (17, 1), (8, 0)):
        assert f(n, nsets, a.ctypes.data_as(dp), o.ctypes.data_as(dp), o.ctypes.data_as(dp)) == -2

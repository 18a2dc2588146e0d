"""GPU tests (-m gpu) of the device primitives every kernel shares, each run by itself through the hooks of include/ddcmi_test.h
(ddcmd_amd/csrc/hip/ddcmi_debug_primitives.inl: the very __device__ functions and kernels of the product) and held against the plain
references of tests/device_primitives.py: exact rational error counts for the reciprocals, numpy restatements for the rest.

The reciprocals.  Inputs: 262 values in each binade 2^-20 ... 2^40 and four in every binade of the doubles (device_primitives.recip_inputs).
  * rsqrt_f64 / rcp_f64 (single-precision seed, two Newton steps; the bonded kernels'): at most 2 ulp of the true result wherever the seed
    instruction works on normal floats; outside that the values are pinned at named points.  The tests' docstrings have what an MI355X gave.
  * rsqrt_f64_pair / rcp_f64_pair (double-precision seed, one Newton step; the pair kernel's), x and the result normal: with e0 the largest
    relative error of the bare seed over the inputs and u = 2^-53, the relative error is at most e0^2 + 2 u (reciprocal: the step squares the
    seed's error; the two fma round once each and the residual's rounding is worth less than a third u) and 1.5 e0^2 (1 + e0) + 2 u (root).
    Derived, not tuned; the test's docstring has the figures.
The wave operations equal numpy on every lane of every set, row_sum_dpp and lean_effective bit for bit.  The scan equals the shifted cumsum
at every size around its tile (2048) and around the 256 tiles at which its second kernel's loop makes a second trip, out of place and in
place, with and without the total, one context shrinking and growing through all of them.  The in-cell sorts equal Python's sort by
(gid as unsigned, shift code, index) on cells of 0 ... 300 entries with ties and gids at and above 2^63.  The census frame's
compaction equals numpy.flatnonzero at every size around a wave, a block and a workgroup's range, and leaves what lies behind nrec alone;
its gid search equals numpy.searchsorted over whole lists of the lengths at which FORCE_AVERAGE's pivot stride changes (the call with int
indices over [0, n): cholAnalysis'), over the sub-ranges behind a pivot as k_track_accumulate forms them, and with 64-bit indices as subsetWrite
calls it.  The pivot search of k_track_accumulate itself, an upper bound in LDS, is not run by these hooks: tests/test_gpu_track.py has it.

docs/primitive_variants.md lists the one-line mutations of the device code that these tests were run against."""
import ctypes

import numpy as np
import pytest

import device_primitives as D
from test_gpu_wave_reduce import make_sets

pytestmark = pytest.mark.gpu
U = D.U
EINVAL = -2
RSQRT_F64, RCP_F64, RSQRT_PAIR, RCP_PAIR, SEED_RSQ, SEED_RCP = range(6)

c_int_p = ctypes.POINTER(ctypes.c_int)
c_double_p = ctypes.POINTER(ctypes.c_double)
c_u64_p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def lib(built):
    import ddcmd_amd._lib as L
    lib = L.load_test_library()
    lib.ddcmi_debug_recip.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]
    lib.ddcmi_debug_wave_ops.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.ddcmi_debug_scan.argtypes = [ctypes.c_void_p, ctypes.c_int, c_int_p, c_int_p, c_int_p, ctypes.c_int]
    lib.ddcmi_debug_sort_cells.argtypes = [ctypes.c_int, c_int_p, c_int_p, ctypes.c_int, c_int_p, c_u64_p, c_int_p]
    lib.ddcmi_debug_compact.argtypes = [ctypes.c_int, c_int_p, ctypes.c_int, ctypes.c_int, c_int_p, c_int_p]
    lib.ddcmi_debug_gid_find.argtypes = [ctypes.c_int, c_u64_p, ctypes.c_int, c_u64_p, c_int_p]
    lib.ddcmi_debug_gid_find_in.argtypes = [ctypes.c_int, c_u64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_u64_p, c_int_p]
    lib.ddcmi_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    lib.ddcmi_destroy.argtypes = [ctypes.c_void_p]
    lib.ddcmi_destroy.restype = None
    for f in (lib.ddcmi_debug_recip, lib.ddcmi_debug_wave_ops, lib.ddcmi_debug_scan, lib.ddcmi_debug_sort_cells, lib.ddcmi_debug_compact, lib.ddcmi_debug_gid_find, lib.ddcmi_debug_gid_find_in,
              lib.ddcmi_create):
        f.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def ctx(lib):
    """a context that holds no beads"""
    c = ctypes.c_void_p()
    assert lib.ddcmi_create(ctypes.byref(c), 0) == 0
    yield c
    lib.ddcmi_destroy(c)


# ---------------------------------------------------------------------------------------------------------------------------------
_recip_out = {}


def recip(lib, which, x=None):
    """the routine on x (default: all inputs, computed once per routine)"""
    if x is None:
        if which not in _recip_out:
            _recip_out[which] = recip(lib, which, np.concatenate(D.recip_inputs()))
        return _recip_out[which]
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full(len(x), 12345.0)
    assert lib.ddcmi_debug_recip(which, len(x), x.ctypes.data_as(c_double_p), y.ctypes.data_as(c_double_p)) == 0
    return y


def worst(e, x):
    i = int(np.argmax(np.abs(e)))
    return float(e[i]), float(x[i])


# the seed instructions work on normal floats: v_rsq_f32 needs a normal argument, v_rcp_f32 a normal argument AND a normal result
F32_DOMAIN = {RSQRT_F64: (D.FLT_MIN, D.FLT_MAX), RCP_F64: (D.FLT_MIN, 2.0 ** 126)}


@pytest.mark.parametrize("which,name,err", [(RSQRT_F64, "rsqrt_f64", D.ulp_error_rsqrt), (RCP_F64, "rcp_f64", D.ulp_error_rcp)])
def test_f32_seeded_reciprocals_within_two_ulp(lib, which, name, err):
    """The domain is the float's normal range for the root.  For the reciprocal it ends at 2^126: above, the single-precision 1/x is subnormal,
    v_rcp_f32 returns 0 for it and two Newton steps leave 0 -- the six inputs of the set in (2^126, FLT_MAX] all give 0.0, which this test pins
    (no caller comes near: ddcmi_internal.h).  Measured on an MI355X (gfx950, ROCm 7.2) with the library of this commit, parent 4b59ac3:
        rsqrt_f64   0.9516 ulp at x = 0x1.0c7011256c167p+40   over 16997 inputs in [2^-126, FLT_MAX]
        rcp_f64     0.5000 ulp at x = 0x1.fffffffffffffp-20   over 16991 inputs in [2^-126, 2^126]"""
    x = np.concatenate(D.recip_inputs())
    y = recip(lib, which)
    lo, hi = F32_DOMAIN[which]
    m = (x >= lo) & (x <= hi)
    assert m.sum() > 16000 and np.all(np.isfinite(y[m]))
    e = err(x[m], y[m])
    w = worst(e, x[m])
    print("%s: largest error %.4f ulp at x = %s over %d inputs in [%s, %s]" % (name, w[0], w[1].hex(), m.sum(), lo.hex(), hi.hex()))
    assert abs(w[0]) <= 2.0, (name, w[0], w[1].hex())
    # the rest of the float's normal range (reciprocal: arguments above 2^126, whose single-precision reciprocal is subnormal)
    rest = (x >= D.FLT_MIN) & (x <= D.FLT_MAX) & ~m
    assert rest.sum() == (6 if which == RCP_F64 else 0) and np.all(y[rest] == 0.0), (name, [v.hex() for v in x[rest]], [v.hex() for v in y[rest]])


def test_f32_seeded_reciprocals_outside_their_domain(lib):
    """what comes back outside the domain, pinned at named points; the comment above rsqrt_f64 in ddcmi_internal.h says the same.  On an
    MI355X (gfx950, ROCm 7.2), this commit:
        x           2^130   2^-130   0     +inf   NaN   -1    2^127       2^126    2^-126   2^-127
        rsqrt_f64   0       NaN      NaN   NaN    NaN   NaN   2^-63.5 ok  2^-63    2^63     NaN
        rcp_f64     0       NaN      NaN   NaN    NaN   -1    0           2^-126   2^126    NaN
    Above the range the float argument is inf, the seed 0, and 0 is a fixed point of both Newton steps: a finite wrong answer.  Below it the
    instructions take a subnormal float for 0: the seed is inf and the first step forms 0 x inf."""
    pts = np.array([2.0 ** 130, 2.0 ** -130, 0.0, np.inf, np.nan, -1.0, 2.0 ** 127, 2.0 ** 126, 2.0 ** -126, 2.0 ** -127])
    rs, rc = recip(lib, RSQRT_F64, pts), recip(lib, RCP_F64, pts)
    print("x         ", [float(v).hex() for v in pts])
    print("rsqrt_f64 ", [float(v).hex() for v in rs])
    print("rcp_f64   ", [float(v).hex() for v in rc])
    assert rs[0] == 0.0 and rc[0] == 0.0 and not np.signbit(rs[0]) and not np.signbit(rc[0])      # not 2^-65 / 2^-130
    assert np.all(np.isnan(rs[1:6]))                      # 2^-130, 0, +inf, NaN, -1
    assert np.all(np.isnan(rc[1:5])) and rc[5] == -1.0    # the reciprocal takes negative arguments
    assert rc[6] == 0.0 and abs(D.ulp_error_rsqrt(pts[6], rs[6])) <= 2.0                           # 2^127: a normal float whose reciprocal is none
    assert rs[7] == 2.0 ** -63 and rs[8] == 2.0 ** 63 and rc[8] == 2.0 ** 126 and rc[7] == 2.0 ** -126      # the ends of the domain, exact
    assert np.isnan(rs[9]) and np.isnan(rc[9])           # 2^-127: the largest subnormal float's binade


@pytest.mark.parametrize("which,seed,name,rel,ulp", [(RSQRT_PAIR, SEED_RSQ, "rsqrt_f64_pair", D.rel_error_rsqrt, D.ulp_error_rsqrt),
                                                     (RCP_PAIR, SEED_RCP, "rcp_f64_pair", D.rel_error_rcp, D.ulp_error_rcp)])
def test_f64_seeded_reciprocals_within_the_newton_bound(lib, which, seed, name, rel, ulp):
    """Measured on an MI355X (gfx950, ROCm 7.2) with the library of this commit, parent 4b59ac3, over the 24166 inputs (the reciprocal: the
    24158 with a normal result), u = 2^-53:
                         bare seed, largest relative error e0                          one Newton step, largest error                       bound
        rsqrt_f64_pair   5.024e-08 = 2^-24.25 (2.4e8 ulp) at 0x1.d7cb918758772p+473    34.19 u, 17.81 ulp at 0x1.d7cb918758772p+473         36.10 u
        rcp_f64_pair     4.479e-08 = 2^-24.41 (2.5e8 ulp) at 0x1.fffcb881a2a61p+22     18.26 u at 0x1.fffcb881a2a61p+22,                    20.07 u
                                                                                       9.80 ulp at 0x1.7fdcc4a762342p+34
    Both errors are the squared seed error almost alone (1.5 e0^2 = 34.1 u, e0^2 = 18.07 u): the seeds are single-precision good, not more,
    and the step's own roundings add a fraction of a u.  This accounts for the 56 u that tests/test_gpu_pair_split.py measured through the
    forces of its uncharged box: the force's leading term near contact is 48 eps sigma^12 ir2^7, which carries seven times ir2's relative
    error -- up to 128 u for a single pair at the worst argument, 56 u after the sum over a bead's pairs, next to a few u of ordinary rounding."""
    x = np.concatenate(D.recip_inputs())
    m = x <= 2.0 ** 1022 if which == RCP_PAIR else np.ones(len(x), bool)      # x is normal throughout; the result too
    x = x[m]
    y0, y = recip(lib, seed)[m], recip(lib, which)[m]
    assert len(x) > 24000 and np.all(np.isfinite(y0)) and np.all(np.isfinite(y)) and np.all(y >= 2.0 ** -1022)
    d0 = rel(x, y0)
    e0, at0 = worst(d0, x)
    e0 = abs(e0)
    bound = e0 * e0 + 2 * U if which == RCP_PAIR else 1.5 * e0 * e0 * (1 + e0) + 2 * U
    d = rel(x, y)
    w = worst(d, x)
    wu = worst(ulp(x, y), x)
    print("%s: seed e0 = %.4g = 2^%.2f at x = %s (%.4g ulp); one step: relative error %.4f u at x = %s, %.4f ulp at x = %s; bound %.4f u"
          % (name, e0, np.log2(e0), at0.hex(), worst(ulp(x, y0), x)[0], w[0] / U, w[1].hex(), wu[0], wu[1].hex(), bound / U))
    assert 2.0 ** -40 < e0 < 2.0 ** -20      # (a seed, not a result)
    assert abs(w[0]) <= bound, (name, w[0] / U, w[1].hex(), bound / U)


# ---------------------------------------------------------------------------------------------------------------------------------
def wave_ops(lib, which, sets):
    a = np.ascontiguousarray(sets)
    out = np.empty_like(a)
    out.view(np.uint8)[...] = 0xA5
    assert lib.ddcmi_debug_wave_ops(which, a.shape[0], a.ctypes.data, out.ctypes.data) == 0
    return out


def test_wave_scan(lib):
    sets, names = D.scan_sets()
    got, want = wave_ops(lib, 0, sets), D.wave_scan_ref(sets)
    bad = [(names[i], int(l), int(got[i, l]), int(want[i, l])) for i, l in zip(*np.nonzero(got != want))]
    assert not bad, bad[:8]


def test_wave_max(lib):
    sets, names = D.max_sets()
    got, want = wave_ops(lib, 1, sets), D.wave_max_ref(sets)
    bad = [(names[i], int(l), int(got[i, l]), int(want[i, l])) for i, l in zip(*np.nonzero(got != want))]
    assert not bad, bad[:8]


def test_row_sum(lib):
    s3, names = make_sets(3)
    sets = np.ascontiguousarray(np.concatenate([s3[:, :, k] for k in range(3)]))      # every column of the wave-reduction sets is a set here
    names = ["%s.%d" % (n, k) for k in range(3) for n in names]
    got = wave_ops(lib, 2, sets)
    want = np.stack([D.row_sum_ref(s) for s in sets])
    na, nb = np.isnan(got), np.isnan(want)
    same = (na & nb) | (~na & ~nb & (got.view(np.uint64) == want.view(np.uint64)))      # (a NaN's payload is not compared)
    bad = [(names[i], int(l), float(got[i, l]).hex(), float(want[i, l]).hex()) for i, l in zip(*np.nonzero(~same))]
    assert not bad, bad[:8]
    assert na.any() and np.signbit(got[names.index("minus_zero.0")]).all()
    # the sum of a row and no other lane's: the one-lane sets give zero in the other three rows
    i = names.index("one_lane20.0")
    assert np.all(got[i, 16:32] != 0) and np.all(got[i, :16] == 0) and np.all(got[i, 32:] == 0)


def test_lean_effective(lib):
    sets, names = D.lean_sets()
    got = wave_ops(lib, 3, sets)
    want = np.stack([D.lean_effective_ref(s) for s in sets])
    same = got.view(np.uint32) == want.view(np.uint32)
    bad = [(names[i], int(l), float(got[i, l]).hex(), float(want[i, l]).hex()) for i, l in zip(*np.nonzero(~same))]
    assert not bad, bad[:8]


# ---------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A
_scan_ref = {}


def scan_reference(kind, n):
    if (kind, n) not in _scan_ref:
        _scan_ref[(kind, n)] = D.scan_ref(D.scan_values(kind, n))
    return _scan_ref[(kind, n)]


def check_scan(lib, ctx, kind, n, in_place, with_total):
    a = D.scan_values(kind, max(n, 0))
    want, want_total = scan_reference(kind, max(n, 0))
    out = np.full(max(n, 0) + D.SCAN_GUARD, SENTINEL, np.int32)
    total = ctypes.c_int(-77)
    rc = lib.ddcmi_debug_scan(ctx, n, a.ctypes.data_as(c_int_p), out.ctypes.data_as(c_int_p), ctypes.byref(total) if with_total else None, int(in_place))
    what = (kind, n, "in place" if in_place else "out of place", "total" if with_total else "no total")
    assert rc == 0, what
    if n > 0:
        wrong = np.nonzero(out[:n] != want)[0]
        assert wrong.size == 0, what + ("first wrong element %d (tile %d): %d, not %d" % (wrong[0], wrong[0] // D.SCAN_TILE, out[wrong[0]], want[wrong[0]]),)
    assert np.all(out[max(n, 0):] == SENTINEL), what + ("elements behind n were written",)
    if with_total:
        assert total.value == want_total, what + ("total %d, not %d" % (total.value, want_total),)


@pytest.mark.parametrize("kind", D.SCAN_VALUES)
def test_scan(lib, ctx, kind):
    for n in D.SCAN_SIZES:
        for in_place in (False, True):
            for with_total in (True, False):
                check_scan(lib, ctx, kind, n, in_place, with_total)


def test_scan_of_nothing(lib, ctx):
    for n in (0, -1, -(2 ** 31)):
        for in_place in (False, True):
            check_scan(lib, ctx, "ones", n, in_place, True)      # total 0, all of out[] untouched
            check_scan(lib, ctx, "ones", n, in_place, False)


def test_scan_on_a_context_that_shrinks_and_grows(lib):
    """one fresh context through the sizes in descending, then ascending order: the scratch array grows in the middle of the second pass,
    and the tile sums a larger call left in it lie behind the ones a smaller call writes"""
    c = ctypes.c_void_p()
    assert lib.ddcmi_create(ctypes.byref(c), 0) == 0
    try:
        check_scan(lib, c, "ones", 9, False, True)               # the scratch array starts small
        for n in sorted(D.SCAN_SIZES, reverse=True):
            check_scan(lib, c, "random", n, n % 2 == 0, True)
        for n in sorted(D.SCAN_SIZES):
            check_scan(lib, c, "tile_first", n, n % 2 == 1, True)
    finally:
        lib.ddcmi_destroy(c)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ("index", "gid", "gid_shift"))
@pytest.mark.parametrize("arrival", D.CELL_ORDERS)
def test_sort_cells(lib, arrival, keys):
    start, cnt, order, key, key2 = D.sort_case(arrival)
    if keys == "index":
        key = key2 = None
    elif keys == "gid":
        key2 = None
    want = D.sort_cells_ref(start, cnt, order, key, key2)
    got = order.copy()
    rc = lib.ddcmi_debug_sort_cells(len(start), start.ctypes.data_as(c_int_p), cnt.ctypes.data_as(c_int_p), len(got), got.ctypes.data_as(c_int_p),
                                    key.ctypes.data_as(c_u64_p) if key is not None else None, key2.ctypes.data_as(c_int_p) if key2 is not None else None)
    assert rc == 0
    inside = np.zeros(len(got), bool)
    for c, (s, n) in enumerate(zip(start, cnt)):
        inside[s:s + n] = True
        assert np.array_equal(got[s:s + n], want[s:s + n]), ("cell %d of %d entries at %d" % (c, n, s), got[s:s + n][:12], want[s:s + n][:12])
    assert (~inside).sum() > 10 and np.array_equal(got[~inside], order[~inside])      # what lies between the cells is left alone


def test_bad_arguments(lib, ctx):
    d = np.ones(64 * 4)
    i = np.zeros(64 * 4 + D.SCAN_GUARD, np.int32)
    dp, ip = d.ctypes.data_as(c_double_p), i.ctypes.data_as(c_int_p)
    for which, n, a, b in ((-1, 4, dp, dp), (6, 4, dp, dp), (0, 0, dp, dp), (0, -3, dp, dp), (0, 2 ** 24 + 1, dp, dp), (0, 4, None, dp), (0, 4, dp, None)):
        assert lib.ddcmi_debug_recip(which, n, a, b) == EINVAL
    for which, n, a, b in ((-1, 1, d.ctypes.data, d.ctypes.data), (4, 1, d.ctypes.data, d.ctypes.data), (0, 0, d.ctypes.data, d.ctypes.data),
                           (0, 65536, d.ctypes.data, d.ctypes.data), (2, 1, None, d.ctypes.data), (2, 1, d.ctypes.data, None)):
        assert lib.ddcmi_debug_wave_ops(which, n, a, b) == EINVAL
    t = ctypes.c_int(0)
    assert lib.ddcmi_debug_scan(None, 4, ip, ip, ctypes.byref(t), 0) == EINVAL
    for n, a, b in ((4, None, ip), (4, ip, None), (0, ip, None), (2 ** 28 + 1, ip, ip)):
        assert lib.ddcmi_debug_scan(ctx, n, a, b, ctypes.byref(t), 0) == EINVAL
    check_scan(lib, ctx, "ones", 9, False, True)      # the context still works
    start, cnt = np.array([0, 8], np.int32), np.array([4, 4], np.int32)
    order = np.arange(12, dtype=np.int32)[::-1].copy()
    key = np.arange(12, dtype=np.uint64)
    sp, cp, op, kp = start.ctypes.data_as(c_int_p), cnt.ctypes.data_as(c_int_p), order.ctypes.data_as(c_int_p), key.ctypes.data_as(c_u64_p)
    f = lib.ddcmi_debug_sort_cells
    assert f(0, sp, cp, 12, op, kp, None) == EINVAL and f(2, None, cp, 12, op, kp, None) == EINVAL and f(2, sp, None, 12, op, kp, None) == EINVAL
    assert f(2, sp, cp, 0, op, kp, None) == EINVAL and f(2, sp, cp, 12, None, kp, None) == EINVAL
    assert f(2, sp, cp, 12, op, None, order.ctypes.data_as(c_int_p)) == EINVAL      # a shift code without a gid
    assert f(2, sp, cp, 11, op, kp, None) == EINVAL                                   # the second cell ends behind order[]
    assert f(2, sp, cp, 11, op, None, None) == EINVAL
    bad = np.array([0, -1], np.int32)
    assert f(2, bad.ctypes.data_as(c_int_p), cp, 12, op, kp, None) == EINVAL and f(2, sp, bad.ctypes.data_as(c_int_p), 12, op, kp, None) == EINVAL
    o2 = order.copy(); o2[1] = 12
    assert f(2, sp, cp, 12, o2.ctypes.data_as(c_int_p), kp, None) == EINVAL           # an entry that names no key
    o2[1] = -1
    assert f(2, sp, cp, 12, o2.ctypes.data_as(c_int_p), kp, None) == EINVAL
    assert np.array_equal(order, np.arange(12)[::-1])                                 # refused calls wrote nothing
    assert f(2, sp, cp, 12, op, kp, None) == 0 and list(order) == [8, 9, 10, 11, 7, 6, 5, 4, 0, 1, 2, 3]


# ---- the census frame's compaction and gid search (ddcmi_census_frame.inl) ---------------------------------------------------
COMPACT_GUARD = 64           # DDCMI_DEBUG_COMPACT_GUARD
COMPACT_MAX_WG = 2048        # census_split(n, 2048) gives ranges of 256 slots up to n = 2^19: the last size spans four workgroups
COMPACT_SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 3 * 256 + 1)
COMPACT_PATTERNS = ("zeros", "ones", "first", "last", "every64", "half")
POISON = -559038737


def compact_flags(pattern, n):
    f = np.zeros(n, np.int32)
    if pattern == "ones":
        f[:] = 1
    elif pattern == "first":
        f[0] = 1
    elif pattern == "last":
        f[-1] = 1
    elif pattern == "every64":
        f[::64] = 1
    elif pattern == "half":
        f[:] = np.random.RandomState(20261021 + n).randint(0, 2, n)
    return f


def compact(lib, flags, nrec, max_wg=COMPACT_MAX_WG):
    places = np.full(nrec + COMPACT_GUARD, POISON, np.int32)
    total = ctypes.c_int(-1)
    assert lib.ddcmi_debug_compact(len(flags), flags.ctypes.data_as(c_int_p), max_wg, nrec, places.ctypes.data_as(c_int_p), ctypes.byref(total)) == 0
    return places, total.value


@pytest.mark.parametrize("pattern", COMPACT_PATTERNS)
def test_compact_equals_flatnonzero(lib, pattern):
    for n in COMPACT_SIZES:
        flags = compact_flags(pattern, n)
        want = np.flatnonzero(flags).astype(np.int32)
        places, total = compact(lib, flags, len(want))
        assert total == len(want), (pattern, n)
        assert np.array_equal(places[:len(want)], want), (pattern, n)
        assert np.all(places[len(want):] == POISON), (pattern, n)


@pytest.mark.parametrize("max_wg,n", [(1, 3 * 256 + 1), (2, 3 * 256 + 1), (1, 8 * 256), (3, 7 * 256 + 65)])
def test_compact_workgroups_of_several_blocks(lib, max_wg, n):
    """few workgroups, so that each walks several blocks of 256 slots (census_split(769, 1): one workgroup of four blocks, the last with one
    slot; (769, 2): two of two; (2048, 1): eight full blocks; (1857, 3): three of three, the last short): the pack kernel's two alternating rows
    of wave counts and the carry of a block's total into the next block's places"""
    for pattern in COMPACT_PATTERNS:
        flags = compact_flags(pattern, n)
        want = np.flatnonzero(flags).astype(np.int32)
        places, total = compact(lib, flags, len(want), max_wg)
        assert total == len(want), (pattern, n)
        assert np.array_equal(places[:len(want)], want) and np.all(places[len(want):] == POISON), (pattern, n)
    flags = compact_flags("half", n)
    want = np.flatnonzero(flags).astype(np.int32)
    places, total = compact(lib, flags, len(want) - 1, max_wg)      # nrec one below the total
    assert total == len(want) and np.array_equal(places[:len(want) - 1], want[:-1]) and np.all(places[len(want) - 1:] == POISON)


def test_compact_stops_at_nrec(lib):
    """nrec one below the total: the last kept slot has no place, and the guard behind nrec stays as it was"""
    for pattern in ("ones", "half", "every64"):
        flags = compact_flags(pattern, 3 * 256 + 1)
        want = np.flatnonzero(flags).astype(np.int32)
        places, total = compact(lib, flags, len(want) - 1)
        assert total == len(want)
        assert np.array_equal(places[:len(want) - 1], want[:-1]) and np.all(places[len(want) - 1:] == POISON), pattern


def gid_lists():
    """ascending 64-bit ids of the lengths around FORCE_AVERAGE's pivot strides, with ids above 2^32 and the largest value"""
    for n in (1, 2, 1024, 1025, 2049):
        rng = np.random.RandomState(n)
        gaps = rng.randint(2, 1 << 20, n).astype(np.uint64)      # at least 2: a value strictly between any two neighbours
        ids = np.cumsum(gaps, dtype=np.uint64) + np.uint64(5)
        ids[n // 2:] += np.uint64(1) << np.uint64(33)            # the upper half above 2^32 (n = 1: the one id)
        ids[-1] = np.uint64(2 ** 64 - 1)
        yield ids


def test_gid_find_equals_searchsorted(lib):
    for ids in gid_lists():
        n = len(ids)
        between = ids[:-1] + np.uint64(1)
        q = np.concatenate([[ids[0] - np.uint64(1), np.uint64(0)], [ids[-1]], [ids[0]], between, ids, ids[:1] + np.uint64(1)]).astype(np.uint64)
        if n > 1:
            q = np.concatenate([q, [ids[-2] + np.uint64(1)]]).astype(np.uint64)      # above every id but the largest value itself
        at = np.searchsorted(ids, q, side="left")
        hit = (at < n) & (ids[np.minimum(at, n - 1)] == q)
        want = np.where(hit, at, -1).astype(np.int32)
        assert hit.sum() >= n + 2 and (~hit).sum() >= 2
        got = np.full(len(q), 12345, np.int32)
        assert lib.ddcmi_debug_gid_find(n, ids.ctypes.data_as(c_u64_p), len(q), q.ctypes.data_as(c_u64_p), got.ctypes.data_as(c_int_p)) == 0
        assert np.array_equal(got, want), n
    # a list whose greatest id is not the largest value: a query above it
    ids = np.array([7, 1 << 40, (1 << 63) + 5], np.uint64)
    q = np.array([(1 << 63) + 6, 2 ** 64 - 1, 6, 7, 1 << 40], np.uint64)
    got = np.full(len(q), 12345, np.int32)
    assert lib.ddcmi_debug_gid_find(3, ids.ctypes.data_as(c_u64_p), len(q), q.ctypes.data_as(c_u64_p), got.ctypes.data_as(c_int_p)) == 0
    assert got.tolist() == [-1, -1, -1, 0, 1]


@pytest.mark.parametrize("wide", [0, 1])
def test_gid_find_in_a_sub_range(lib, wide):
    """the ranges k_track_accumulate searches, ids[u << l, min(n, (u + 1) << l)) behind pivot u for the strides 2 and 4 of lists of 1025 and
    2049 gids, and a few others (empty, one entry, the tail): the queries are the range's gids, their neighbours in the list on either side
    (listed, but outside the range: a miss), values between entries, below and above everything.  int and 64-bit indices."""
    for ids in gid_lists():
        n = len(ids)
        ranges = [(0, 0), (n, n), (0, 1), (n - 1, n), (n // 3, n), (0, n)]
        for l in (1, 2):
            ranges += [(u << l, min(n, (u + 1) << l)) for u in (0, 1, (n - 1) >> l, ((n - 1) >> l) - 1) if u >= 0 and (u << l) < n]
        for lo, hi in ranges:
            around = ids[max(lo - 2, 0):min(hi + 2, n)]
            q = np.concatenate([around, around + np.uint64(1), [np.uint64(0), np.uint64(2 ** 64 - 1)]]).astype(np.uint64)
            at = lo + np.searchsorted(ids[lo:hi], q, side="left")
            hit = (at < hi) & (ids[np.minimum(at, n - 1)] == q)
            want = np.where(hit, at, -1).astype(np.int32)
            got = np.full(len(q), 12345, np.int32)
            assert lib.ddcmi_debug_gid_find_in(n, ids.ctypes.data_as(c_u64_p), lo, hi, wide, len(q), q.ctypes.data_as(c_u64_p), got.ctypes.data_as(c_int_p)) == 0
            assert np.array_equal(got, want), (n, lo, hi, wide)
    ids = np.arange(8, dtype=np.uint64)
    q, got = ids.copy(), np.zeros(8, np.int32)
    for lo, hi in ((-1, 4), (5, 4), (0, 9)):
        assert lib.ddcmi_debug_gid_find_in(8, ids.ctypes.data_as(c_u64_p), lo, hi, wide, 8, q.ctypes.data_as(c_u64_p), got.ctypes.data_as(c_int_p)) == EINVAL


def test_compact_and_gid_find_bad_arguments(lib):
    f = np.ones(8, np.int32)
    p = np.zeros(8 + COMPACT_GUARD, np.int32)
    t = ctypes.c_int(0)
    fp, pp = f.ctypes.data_as(c_int_p), p.ctypes.data_as(c_int_p)
    for n, a, wg, nrec, b, c in ((0, fp, 4, 8, pp, ctypes.byref(t)), (8, None, 4, 8, pp, ctypes.byref(t)), (8, fp, 0, 8, pp, ctypes.byref(t)),
                                 (8, fp, 2049, 8, pp, ctypes.byref(t)), (8, fp, 4, -1, pp, ctypes.byref(t)), (8, fp, 4, 8, None, ctypes.byref(t)), (8, fp, 4, 8, pp, None)):
        assert lib.ddcmi_debug_compact(n, a, wg, nrec, b, c) == EINVAL
    ids, q, idx = np.array([3, 2], np.uint64), np.array([2], np.uint64), np.zeros(1, np.int32)
    ip, qp, xp = ids.ctypes.data_as(c_u64_p), q.ctypes.data_as(c_u64_p), idx.ctypes.data_as(c_int_p)
    assert lib.ddcmi_debug_gid_find(2, ip, 1, qp, xp) == EINVAL      # not ascending
    assert lib.ddcmi_debug_gid_find(0, ip, 1, qp, xp) == EINVAL and lib.ddcmi_debug_gid_find(1, None, 1, qp, xp) == EINVAL
    assert lib.ddcmi_debug_gid_find(1, ip, 0, qp, xp) == EINVAL and lib.ddcmi_debug_gid_find(1, ip, 1, None, xp) == EINVAL and lib.ddcmi_debug_gid_find(1, ip, 1, qp, None) == EINVAL

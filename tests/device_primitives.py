"""Plain references and input sets for the device primitives every kernel shares (tests/test_gpu_device_primitives.py runs them on the
device through the hooks of include/ddcmi_test.h; tests/test_device_primitives_host.py checks this module without one).  No device code
and no oracle here: exact rational arithmetic, numpy and Python's sort.

  * ulp_error_rcp / ulp_error_rsqrt: the error of a computed y ~ 1/x or y ~ 1/sqrt(x) in units of one ulp of the TRUE result, exact.  The
    doubles are taken apart into integer mantissa and exponent, r = x y - 1 (or x y^2 - 1) is formed as a rational, and the true result is
    y / (1 + d) with d the relative error of y: d = r for the reciprocal; for the root 1 + r = (1 + d)^2, d = r / 2 - r^2 / 8 + O(r^3) --
    the third-order term is 2^-47 of d for a single-precision seed (r ~ 2^-22) and less for everything better.  No longdouble and no libm.
  * the input sets of the reciprocals, the wave operations, the scan and the in-cell sort;
  * numpy restatements of the wave operations (the row sum and lean_effective operation for operation, so bit for bit), of the scan and
    of the sort."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
FLT_MIN = 2.0 ** -126                          # the smallest normal float
FLT_MAX = (2.0 - 2.0 ** -23) * 2.0 ** 127
LEAN_C = np.float32(0.81)                      # ddcmi_nonbond.inl
LEAN_W = 32                                    # ddcmi_internal.h
SCAN_TILE = 2048                               # scan.hip
SCAN_GUARD = 2048                              # DDCMI_DEBUG_SCAN_GUARD (include/ddcmi_test.h)
INT_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# exact errors of reciprocals
def _split(v):
    """v = n 2^k with integers n, k (exact; v finite)"""
    m, e = math.frexp(v)
    return int(math.ldexp(m, 53)), e - 53


def _dyadic(n, k):
    return Fraction(n << k, 1) if k >= 0 else Fraction(n, 1 << -k)


def _ulp_exponent_rcp(x):
    """e - 52 with 2^e <= 1/x < 2^(e+1), not below the subnormals' spacing"""
    m, ex = math.frexp(x)                      # x = m 2^ex, 1/2 <= m < 1: 1/x = (1/m) 2^-ex, 1 < 1/m <= 2
    e = 1 - ex if m == 0.5 else -ex
    return max(e, -1022) - 52


def _ulp_exponent_rsqrt(x):
    """e - 52 with 2^e <= 1/sqrt(x) < 2^(e+1)"""
    m, ex = math.frexp(x)
    if ex % 2 == 0:                            # 1 < m^-1/2 <= sqrt 2
        e = -ex // 2
    else:                                      # x = (2m) 2^(ex-1), 1 <= 2m < 2: 1/sqrt 2 < (2m)^-1/2 <= 1
        e = -(ex - 1) // 2 - (0 if m == 0.5 else 1)
    return e - 52


def _rel_rcp(x, y):
    nx, kx = _split(x)
    ny, ky = _split(y)
    return _dyadic(nx * ny, kx + ky) - 1       # x y - 1 = d, exactly


def _rel_rsqrt(x, y):
    nx, kx = _split(x)
    ny, ky = _split(y)
    r = _dyadic(nx * ny * ny, kx + 2 * ky) - 1
    return r / 2 - r * r / 8


def _err(x, y, rel, ulp_exponent, in_ulp):
    x, y = float(x), float(y)
    if not (math.isfinite(x) and math.isfinite(y)) or x <= 0.0:
        raise ValueError("ulp_error: x = %r, y = %r" % (x, y))
    d = rel(x, y)
    if not in_ulp:
        return float(d)
    ny, ky = _split(y)
    return float(d / (1 + d) * _dyadic(ny, ky - ulp_exponent(x)))      # y - true = true d = y d / (1 + d)


def _vector(x, y, *a):
    if np.ndim(x) == 0:
        return _err(x, y, *a)
    return np.array([_err(p, q, *a) for p, q in zip(np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel())]).reshape(np.shape(x))


def ulp_error_rcp(x, y):
    """(y - 1/x) / ulp(1/x), signed, exact up to the final rounding to a double; x > 0 and y finite (scalars or arrays)"""
    return _vector(x, y, _rel_rcp, _ulp_exponent_rcp, True)


def ulp_error_rsqrt(x, y):
    """(y - 1/sqrt x) / ulp(1/sqrt x), signed (module docstring)"""
    return _vector(x, y, _rel_rsqrt, _ulp_exponent_rsqrt, True)


def rel_error_rcp(x, y):
    """y x - 1: the relative error of y as a reciprocal of x, signed"""
    return _vector(x, y, _rel_rcp, _ulp_exponent_rcp, False)


def rel_error_rsqrt(x, y):
    """d with y = (1 + d) / sqrt x, signed"""
    return _vector(x, y, _rel_rsqrt, _ulp_exponent_rsqrt, False)


def sqrt2_neighbours():
    """the two doubles next to sqrt 2, below and above"""
    s = math.sqrt(2.0)
    if Fraction(s) ** 2 > 2:
        return math.nextafter(s, 0.0), s
    return s, math.nextafter(s, 2.0)


BINADES = range(-20, 41)                       # every r^2, g1, g2 and 1 - cos^2 of a Martini deck in the library's length unit (bohr)
EDGES = (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 1.5) + sqrt2_neighbours()
_recip = None


def recip_inputs():
    """the inputs of the reciprocal tests: (dense, sparse), positive normal doubles.  dense: per binade 2^-20 ... 2^40, 256 random mantissas
    and the six EDGES.  sparse: every exponent -1022 ... 1023 with the mantissas 1, 2 - 2^-52 and two random ones.  Computed once; do not
    write to them."""
    global _recip
    if _recip is None:
        rng = np.random.default_rng(20261020)
        dense = np.concatenate([np.ldexp(np.concatenate([1.0 + rng.integers(0, 2 ** 52, 256) * 2.0 ** -52, EDGES]), e) for e in BINADES])
        ex = np.arange(-1022, 1024)
        sparse = np.ldexp(np.stack([np.ones(ex.size), np.full(ex.size, 2.0 - 2.0 ** -52), 1.0 + rng.integers(0, 2 ** 52, ex.size) * 2.0 ** -52,
                                    1.0 + rng.integers(0, 2 ** 52, ex.size) * 2.0 ** -52], 1), ex[:, None]).ravel()
        dense.setflags(write=False)
        sparse.setflags(write=False)
        _recip = (dense, sparse)
    return _recip


# ---------------------------------------------------------------------------------------------------------------------------------
# the wave operations
def scan_sets():
    """[nsets][64] int32 and their names: the sets of the wave scan (and of the wave maximum)"""
    rng = np.random.default_rng(20261021)
    sets, names = [], []
    for l in range(64):
        a = np.zeros(64, np.int32)
        a[l] = 1 + 37 * l
        sets.append(a); names.append("one_hot%d" % l)
    sets.append(np.ones(64, np.int32)); names.append("ones")
    sets.append(np.full(64, 4095, np.int32)); names.append("equal")
    for r in range(4):
        sets.append(rng.integers(0, 4097, 64).astype(np.int32)); names.append("random%d" % r)
    sets.append(np.zeros(64, np.int32)); names.append("zeros")
    # (one lane short of INT_MAX / 64 everywhere: the largest sums the scan can hold)
    sets.append(np.full(64, INT_MAX // 64, np.int32)); names.append("large")
    return np.stack(sets), names


def max_sets():
    """the scan's sets, INT_MAX in one lane (a lane of each row and the lanes at the row boundaries), and bit patterns of non-negative
    floats -- what block_vmax_store (ddcmi_integrator.inl) hands wave_max_dpp"""
    rng = np.random.default_rng(20261022)
    s, names = scan_sets()
    sets = list(s)
    for l in (0, 15, 16, 31, 32, 47, 48, 63, 5, 26, 41, 58):
        a = rng.integers(0, 4097, 64).astype(np.int32)
        a[l] = INT_MAX
        sets.append(a); names.append("int_max%d" % l)
    for r in range(3):
        f = np.ldexp(rng.uniform(1.0, 2.0, 64), rng.integers(-30, 31, 64)).astype(np.float32)
        sets.append(f.view(np.int32)); names.append("float_bits%d" % r)
    f = np.zeros(64, np.float32); f[37] = np.float32(1e-30); f[2] = np.float32(np.inf)
    sets.append(f.view(np.int32)); names.append("float_bits_inf")
    # all-different values in descending and ascending lane order: every lane holds the maximum of some group of lanes
    sets.append(np.arange(64, 0, -1, dtype=np.int32) * 1000); names.append("descending")
    sets.append(np.arange(1, 65, dtype=np.int32) * 1000); names.append("ascending")
    return np.stack(sets), names


def lean_sets():
    """[nsets][64] float32 and their names: the ring's LEAN_W words in lanes 0 ... 31, zeros behind them as k_nonbond loads them"""
    rng = np.random.default_rng(20261023)
    sets, names = [], []

    def add(name, w):
        a = np.zeros(64, np.float32)
        a[:len(w)] = np.asarray(w, dtype=np.float32)
        sets.append(a); names.append(name)

    s = np.arange(LEAN_W)
    add("zeros", np.zeros(LEAN_W))
    for l in range(LEAN_W):
        w = np.zeros(LEAN_W); w[l] = 3.0 + 0.37 * l
        add("one_word%d" % l, w)
    add("rising", 1.0 + 0.173 * s)
    add("falling_fast", 7.3 * 0.7 ** s)          # faster than 0.81 per step: every E_s is the decayed first word
    add("falling_slow", 7.3 * 0.9 ** s)          # slower: every E_s is its own word
    for r in range(4):
        add("random%d" % r, rng.uniform(0.0, 10.0, LEAN_W))
    add("sparse", np.where(rng.integers(0, 4, LEAN_W) == 0, rng.uniform(0.0, 10.0, LEAN_W), 0.0))
    add("equal", np.full(LEAN_W, 2.718))
    sets.append(rng.uniform(0.0, 10.0, 64).astype(np.float32)); names.append("random_all_lanes")
    return np.stack(sets), names


def wave_scan_ref(sets):
    return np.cumsum(sets.astype(np.int64), axis=1).astype(np.int32)


def wave_max_ref(sets):
    return np.repeat(sets.max(axis=1)[:, None], 64, axis=1)


def row_sum_ref(col):
    """row_sum_dpp on 64 doubles: partner lane ^ 1, ^ 2, ^ 7, ^ 15 (the first four steps of test_gpu_wave_reduce.tree64)"""
    lane = np.arange(64)
    v = np.array(col, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in (1, 2, 7, 15):
            v = v + v[lane ^ x]
    return v


def lean_effective_ref(w):
    """lean_effective (ddcmi_nonbond.inl) on the 64 lanes of a wave, operation for operation in float32"""
    e = np.array(w, dtype=np.float32)
    lane = np.arange(64)
    c = LEAN_C
    i = 1
    while i < LEAN_W:
        t = np.concatenate([e[:i], e[:-i]])      # __shfl_up by i (a lane below i gets its own value back and keeps its own anyway)
        e = np.where(lane >= i, np.maximum(e, (t * c).astype(np.float32)), e).astype(np.float32)
        c = np.float32(c * c)
        i <<= 1
    return e


# ---------------------------------------------------------------------------------------------------------------------------------
# the scan
T = SCAN_TILE
SCAN_SIZES = (0, 1, 7, 8, 9, T - 1, T, T + 1, 2 * T, 2 * T + 1, 255 * T + 5, 256 * T - 1, 256 * T, 256 * T + 1, 257 * T + 5, 512 * T, 513 * T + 1)
SCAN_VALUES = ("ones", "random", "tile_last", "tile_first", "int_max")
_scan_cache = {}


def scan_values(kind, n):
    """the int32 input of a scan test.  ones: the result is the index.  random: 0 ... 7.  tile_last / tile_first: zero but for the last /
    first element of every tile (and the very last element), tile b's holding b + 1.  int_max: a total of exactly 2^31 - 1."""
    key = (kind, n)
    if key in _scan_cache:
        return _scan_cache[key]
    if kind == "ones":
        a = np.ones(n, np.int32)
    elif kind == "random":
        a = np.random.default_rng(20261024 + n).integers(0, 8, n).astype(np.int32)
    elif kind in ("tile_last", "tile_first"):
        a = np.zeros(n, np.int32)
        if kind == "tile_last":
            a[T - 1::T] = 1 + np.arange(len(a[T - 1::T]))
            if n:
                a[-1] = 1 + (n - 1) // T
        else:
            a[0::T] = 1 + np.arange(len(a[0::T]))
    elif kind == "int_max":
        q, r = divmod(INT_MAX, max(n, 1))
        a = np.full(n, q, np.int32)
        a[n - r:] += 1                           # (n > 0: the remainder over the last elements, so every prefix stays below the total)
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    _scan_cache[key] = a
    return a


def scan_ref(a):
    """(the exclusive prefix sums, the total) of int32 a: np.cumsum shifted"""
    c = np.cumsum(a, dtype=np.int64)
    out = np.zeros(len(a), np.int64)
    out[1:] = c[:-1]
    total = int(c[-1]) if len(a) else 0
    assert total <= INT_MAX
    return out.astype(np.int32), total


# ---------------------------------------------------------------------------------------------------------------------------------
# the in-cell sort
CELL_SIZES = (0, 1, 2, 64, 300)
CELL_ORDERS = ("reversed", "sorted", "random")
BIG = 1 << 63


def sort_case(arrival, seed=0):
    """cells of CELL_SIZES entries (one of each size and kind of key, shuffled) with gaps of 0 ... 5 untouched entries between them, over norder = the
    number of beads: (start, cnt, order, key, key2).  The entries of the cells are a permutation of part of range(norder); the gaps hold
    entries too (the sort must leave them).  key: 64-bit gids in four kinds of cell -- all different; every gid twice or more (key2 decides);
    gid and key2 equal in runs (the index decides); gids at and above 2^63 next to small ones.  arrival: the order of a cell's entries
    before the sort, by the sorted order -- reversed, sorted, random."""
    rng = np.random.default_rng(20261025 + seed)
    cells = rng.permutation([(n, kind) for n in CELL_SIZES for kind in range(4)])
    sizes, kinds = cells[:, 0], cells[:, 1]
    gaps = rng.integers(0, 6, len(sizes) + 1)
    norder = int(sizes.sum() + gaps.sum())
    perm = rng.permutation(norder).astype(np.int32)          # which bead sits where
    start = (gaps[0] + np.concatenate([[0], np.cumsum(sizes + gaps[1:])[:-1]])).astype(np.int32)
    cnt = sizes.astype(np.int32)
    key = rng.integers(0, 1 << 40, norder).astype(np.uint64)
    key2 = rng.integers(0, 27, norder).astype(np.int32)
    for c, (s, n) in enumerate(zip(start, cnt)):
        idx = perm[s:s + n]
        kind = kinds[c]
        if kind == 1:                           # every gid several times, different shift codes
            key[idx] = rng.integers(0, max(n // 3, 1), n).astype(np.uint64) + np.uint64(1000)
        elif kind == 2:                          # ties in both: the index decides
            key[idx] = rng.integers(0, max(n // 8, 1), n).astype(np.uint64) + np.uint64(7)
            key2[idx] = rng.integers(0, 2, n)
        elif kind == 3:                          # the top bit: 2^63, 2^63 + small, 2^64 - 1 next to 0, 1, 2^63 - 1
            pool = np.array([BIG, BIG + 1, BIG + 5, (1 << 64) - 1, (1 << 64) - 2, 0, 1, BIG - 1, BIG - 2, 1 << 62], dtype=np.uint64)
            key[idx] = pool[rng.integers(0, len(pool), n)]
    order = perm.copy()
    for s, n in zip(start, cnt):
        want = sort_ref(order[s:s + n], key, key2)
        if arrival == "reversed":
            order[s:s + n] = want[::-1]
        elif arrival == "sorted":
            order[s:s + n] = want
        else:
            order[s:s + n] = rng.permutation(want)
    return start, cnt, order, key, key2


def sort_ref(entries, key=None, key2=None):
    """Python's sort of a cell's entries by (key, key2, entry); without a key by the entry"""
    if key is None:
        return np.array(sorted(int(i) for i in entries), dtype=np.int32)
    return np.array(sorted((int(i) for i in entries), key=lambda i: (int(key[i]), int(key2[i]) if key2 is not None else 0, i)), dtype=np.int32)


def sort_cells_ref(start, cnt, order, key=None, key2=None):
    out = order.copy()
    for s, n in zip(start, cnt):
        out[s:s + n] = sort_ref(order[s:s + n], key, key2)
    return out

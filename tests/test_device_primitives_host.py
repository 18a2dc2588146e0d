"""tests/device_primitives.py checked without a GPU: the exact ulp functions against numpy's correctly rounded operations and against
perturbations made by hand, the restatement of lean_effective against the properties its comment in ddcmi_nonbond.inl states, and the input
sets against the sizes and edge values the device tests rely on."""
import math
from fractions import Fraction

import numpy as np

import device_primitives as D


def _sample():
    dense, sparse = D.recip_inputs()
    return np.concatenate([dense[::7], sparse[::5]])


def test_ulp_functions_on_correctly_rounded_results():
    x = _sample()
    e = D.ulp_error_rcp(x[x <= 2.0 ** 1022], 1.0 / x[x <= 2.0 ** 1022])        # (normal results)
    assert np.abs(e).max() <= 0.5 and np.abs(e).max() > 0.4
    e = D.ulp_error_rsqrt(x, 1.0 / np.sqrt(x))       # sqrt: 1/2 ulp of the root, at most one of the result; the division: 1/2 more
    assert np.abs(e).max() <= 1.5 and np.abs(e).max() > 0.5
    # exact results: powers of two, and of four under the root
    p = np.ldexp(1.0, np.arange(-1000, 1001, 2))
    assert np.all(D.ulp_error_rcp(p, 1.0 / p) == 0.0) and np.all(D.ulp_error_rsqrt(p, np.ldexp(1.0, -np.arange(-1000, 1001, 2) // 2)) == 0.0)


def test_ulp_functions_report_a_perturbation_made_by_hand():
    x = _sample()
    x = x[(x >= 2.0 ** -1000) & (x <= 2.0 ** 1000)]
    for name, f, y0, tol in (("rcp", D.ulp_error_rcp, 1.0 / x, 0.5), ("rsqrt", D.ulp_error_rsqrt, 1.0 / np.sqrt(x), 1.5)):
        base = f(x, y0)
        for k in (1, 7, 100):
            for sign in (1, -1):
                # y0 moved by k of its own ulps, which are the true result's where y0, y and the true result lie in one binade
                y = (y0.view(np.int64) + sign * k).view(np.float64)
                ok = (np.frexp(y)[1] == np.frexp(y0)[1]) & (_exp_true(name, x) == np.frexp(y0)[1] - 1)
                e = f(x, y)
                assert ok.sum() > 0.7 * len(x)      # (the rest: results at a power of two, which half of the sparse inputs give)
                assert np.all(np.abs(e[ok] - base[ok] - sign * k) <= 1e-12), (name, k, sign)      # (each exact to 2^-53 of a value below 2^7)
                assert np.all(np.abs(e[ok] - sign * k) <= tol)


def _exp_true(name, x):
    return np.array([(D._ulp_exponent_rcp(v) if name == "rcp" else D._ulp_exponent_rsqrt(v)) + 52 for v in x])


def test_ulp_functions_report_a_relative_error_of_a_single_precision_seed():
    """y = true (1 + 2^-23): the relative error comes back to three digits (the root's second-order term is 2^-25 of it: without it the
    first-order (x y^2 - 1) / 2 would still pass; to six digits it would not), and the ulp count is that times the true mantissa"""
    rng = np.random.default_rng(5)
    d = 2.0 ** -23
    for x in np.ldexp(rng.uniform(1.0, 2.0, 200), rng.integers(-100, 100, 200)):
        X = Fraction(float(x))
        y_r = float(Fraction(1) / X * (1 + Fraction(d)))                       # correctly rounded: Fraction -> float
        assert abs(D.rel_error_rcp(x, y_r) / d - 1.0) < 1e-6
        root = Fraction(math.isqrt(int((1 / X) * (1 << 400)))) / (1 << 200)    # 1/sqrt x to 2^-190
        y_s = float(root * (1 + Fraction(d)))
        assert abs(D.rel_error_rsqrt(x, y_s) / d - 1.0) < 1e-6
        first_order = float((X * Fraction(y_s) ** 2 - 1) / 2)
        assert abs(first_order / d - 1.0) > 1e-8 and abs(first_order / d - 1.0) < 1e-3
        mant = float(root) / 2.0 ** (D._ulp_exponent_rsqrt(x) + 52)
        assert 1.0 <= mant < 2.0 and abs(D.ulp_error_rsqrt(x, y_s) / (d * mant * 2.0 ** 52) - 1.0) < 1e-3
        mant = float(1 / X) / 2.0 ** (D._ulp_exponent_rcp(x) + 52)
        assert 1.0 <= mant < 2.0 and abs(D.ulp_error_rcp(x, y_r) / (d * mant * 2.0 ** 52) - 1.0) < 1e-3


def test_lean_effective_restatement():
    sets, names = D.lean_sets()
    c = float(D.LEAN_C)
    eps = 2.0 ** -23
    for w, name in zip(sets, names):
        e = D.lean_effective_ref(w)
        assert e.dtype == np.float32
        assert np.all(e >= w), name                                            # E_s >= W_s
        # E_s >= 0.81 E_(s-1) over the ring's 32 words (a lane looks 31 back), up to the roundings of the at most five products behind either side
        assert np.all(e[1:32].astype(np.float64) >= c * e[:31].astype(np.float64) * (1 - 12 * eps)), name
        # E_s = max_j 0.81^(s-j) W_j over the window of 32 (1 + 2 + 4 + 8 + 16 = 31 steps back); LEAN_C^k by squaring: at most 5 products
        # and 4 squarings of the constant in float
        s = np.arange(64)
        k = s[:, None] - s[None, :]
        decay = np.where((k >= 0) & (k < D.LEAN_W), c ** np.clip(k, 0, None), 0.0)
        exact = (decay * w.astype(np.float64)[None, :]).max(axis=1)
        assert np.all(np.abs(e - exact) <= 40 * eps * exact), (name, np.abs(e - exact).max())
    i = names.index("falling_fast")
    assert np.all(D.lean_effective_ref(sets[i])[1:32] > sets[i][1:32])           # the decayed first word
    i = names.index("falling_slow")
    assert np.all(D.lean_effective_ref(sets[i])[:32] == sets[i][:32])            # its own word
    i = names.index("one_word5")
    assert np.all(D.lean_effective_ref(sets[i])[:5] == 0) and np.all(np.diff(D.lean_effective_ref(sets[i])[5:37]) < 0) and D.lean_effective_ref(sets[i])[37] == 0


def test_input_sets():
    dense, sparse = D.recip_inputs()
    assert len(dense) == 61 * 262 and len(sparse) == 2046 * 4 and 24000 < len(dense) + len(sparse) < 26000
    assert dense.min() == 2.0 ** -20 and dense.max() == (2.0 - 2.0 ** -52) * 2.0 ** 40
    lo, hi = D.sqrt2_neighbours()
    assert Fraction(lo) ** 2 < 2 < Fraction(hi) ** 2 and math.nextafter(lo, 2.0) == hi
    for e in D.BINADES:
        b = dense[(dense >= 2.0 ** e) & (dense < 2.0 ** (e + 1))]
        assert len(b) == 262 and all(math.ldexp(v, e) in b for v in D.EDGES)
    assert sparse.min() == 2.0 ** -1022 and sparse.max() == np.finfo(np.float64).max and np.all(np.isfinite(sparse))
    assert np.array_equal(np.unique(np.frexp(sparse)[1]), np.arange(-1021, 1025))
    s, names = D.scan_sets()
    assert s.shape == (len(names), 64) and s.dtype == np.int32 and sum(n.startswith("one_hot") for n in names) == 64
    assert np.all(s >= 0) and np.all(s.astype(np.int64).sum(axis=1) < 2 ** 31) and {"ones", "equal", "zeros", "random0"} <= set(names)
    m, names = D.max_sets()
    assert np.all(m >= 0) and (m == D.INT_MAX).any(axis=1).sum() == 12 and sum(n.startswith("float_bits") for n in names) == 4
    l, names = D.lean_sets()
    assert l.dtype == np.float32 and sum(n.startswith("one_word") for n in names) == 32 and np.all(l[:-1, 32:] == 0) and np.all(l >= 0)
    assert {"zeros", "rising", "falling_fast", "falling_slow", "random0", "equal"} <= set(names)
    r = l[names.index("falling_fast")][:32]; assert np.all(r[1:] < 0.81 * r[:-1])
    r = l[names.index("falling_slow")][:32]; assert np.all(r[1:] > 0.81 * r[:-1]) and np.all(r[1:] < r[:-1])
    T = D.SCAN_TILE
    assert T == 2048 and len(D.SCAN_SIZES) == 17 and max(D.SCAN_SIZES) == 513 * T + 1 and {0, T, 256 * T, 256 * T + 1, 257 * T + 5} <= set(D.SCAN_SIZES)
    for n in (0, 1, 9, T + 1, 257 * T + 5):
        for kind in D.SCAN_VALUES:
            a = D.scan_values(kind, n)
            out, total = D.scan_ref(a)
            assert a.dtype == np.int32 and len(a) == n and len(out) == n and total == int(a.astype(np.int64).sum()) and np.all(a >= 0)
            if kind == "ones":
                assert np.array_equal(out, np.arange(n))
            if kind == "int_max" and n:
                assert total == D.INT_MAX
            if kind == "tile_last" and n:
                assert np.count_nonzero(a) == (n + T - 1) // T and a[-1] != 0 and (n < T or a[T - 1] == 1)
            if kind == "tile_first" and n:
                assert np.count_nonzero(a) == (n + T - 1) // T and a[0] == 1
            assert not a.flags.writeable
    for arrival in D.CELL_ORDERS:
        start, cnt, order, key, key2 = D.sort_case(arrival)
        assert sorted(cnt) == sorted(list(D.CELL_SIZES) * 4) and np.all(start[1:] >= start[:-1] + cnt[:-1]) and start[-1] + cnt[-1] <= len(order)
        assert (start[1:] > start[:-1] + cnt[:-1]).any() and np.array_equal(np.sort(order), np.arange(len(order)))
        assert key.dtype == np.uint64 and (key >= np.uint64(D.BIG)).any() and (key == np.uint64(D.BIG)).any() and (key == np.uint64(2 ** 64 - 1)).any()
        want = D.sort_cells_ref(start, cnt, order, key, key2)
        ties_key = ties_both = 0
        for s, n in zip(start, cnt):
            c = want[s:s + n]
            k = [(int(key[i]), int(key2[i]), int(i)) for i in c]
            assert k == sorted(k)
            ties_key += sum(a[0] == b[0] and a[1] != b[1] for a, b in zip(k, k[1:]))
            ties_both += sum(a[:2] == b[:2] for a, b in zip(k, k[1:]))
        assert ties_key > 50 and ties_both > 50
        if arrival == "sorted":
            assert np.array_equal(want, order)
        else:
            assert not np.array_equal(want, order)
        assert not np.array_equal(D.sort_cells_ref(start, cnt, order), want) and not np.array_equal(D.sort_cells_ref(start, cnt, order, key), want)

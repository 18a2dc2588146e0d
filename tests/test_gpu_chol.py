"""cholAnalysis on the device (ddcmi_chol_offsets, Martini*.chol_offsets) on the planted systems of chol_systems.py: both histograms
against the longdouble reference away from the bin edges (the derived bound q_bound; tests/test_chol_host.py holds the share of
molecules inside it at 1 %), the planted edge cases by hand, extremes bitwise a single molecule's, the sums within nmol eps max|d|,
the run untouched, brick grids with molecules split over domains, and every refusal."""
import ctypes

import numpy as np
import pytest

import chol_systems as C
from chol_systems import LD

pytestmark = pytest.mark.gpu
ARGS = (C.RMIN, C.DELTA, C.NBINS)


def _single(s):
    from ddcmd_amd.martini import MartiniHIP
    m = MartiniHIP(s)
    m.eval_forces()
    return m


def _host_lane(m, s, pbc):
    from ddcmd_amd import martini
    return np.array([martini.chol_molecule(m.lib, r, C.box_of(s), pbc, *ARGS) for r in s.mol_r])


@pytest.mark.parametrize("pbc", [7, 3])
@pytest.mark.parametrize("nmol", C.SIZES)
def test_against_the_reference(nmol, pbc):
    s = C.made("system", nmol, pbc)
    L = C.box_of(s)
    m = _single(s)
    counts, stats, n = m.chol_offsets(s.gid7, *ARGS)
    again = m.chol_offsets(s.gid7, *ARGS)
    lane = _host_lane(m, s, pbc)
    m.close()
    assert n == nmol
    assert counts.tobytes() == again[0].tobytes() and stats.tobytes() == again[1].tobytes() and again[2] == n
    d = C.reference(s.mol_r, L, pbc)
    qb = C.q_bound(L.max())
    dmax = max(float(np.nanmax(np.abs(x))) for x in d)
    for k in range(2):
        b, q = C.bins_of(d[k])
        with np.errstate(invalid="ignore"):
            near = np.abs(q - np.rint(q)) <= qb
        got = counts[k * C.NBINS:(k + 1) * C.NBINS]
        assert got.sum() == nmol
        # the molecules away from an edge are where the reference has them; one near an edge sits in the reference's bin or the
        # neighbouring one -- the bin the lane's arithmetic gives it -- and the histogram is exactly the sum of the two
        near_bins = lane[near, 2 + k].astype(np.int64)
        assert (np.abs(near_bins - b[near]) <= 1).all()
        assert (got == np.bincount(b[~near], minlength=C.NBINS) + np.bincount(near_bins, minlength=C.NBINS)).all()
        fin = ~np.isnan(d[k].astype(float))
        vals = lane[fin, k]
        print("nmol %d pbc %d dR%d: sum %.17g reference %.17g bound %.3g; min %.17g max %.17g" % (
            nmol, pbc, (1, 5)[k], stats[3 * k], float(np.sum(d[k][fin])), nmol * C.EPS * dmax, stats[3 * k + 1], stats[3 * k + 2]))
        # the extremes: bitwise one molecule's value -- the lane's arithmetic restated on the host gives every molecule's
        assert stats[3 * k + 1] == vals.min() and stats[3 * k + 2] == vals.max()
        if fin.all():
            assert abs(LD(stats[3 * k]) - np.sum(d[k])) <= nmol * C.EPS * dmax
        else:
            assert np.isnan(stats[3 * k])      # the collinear molecule joins the sum
    if s.nedge:
        exp = C.expected_edge_bins()
        assert [(int(a), int(b)) for a, b in lane[:s.nedge, 2:]] == exp


def test_edge_cases_alone():
    """the planted molecules by themselves: exact offsets, bins by hand; the list in descending gid order gives the same histograms"""
    s = C.made("system", 1025, 7)
    m = _single(s)
    ne = s.nedge
    counts, stats, n = m.chol_offsets(s.gid7[:ne], *ARGS)
    exp = np.zeros(2 * C.NBINS, np.int64)
    for b1, b5 in C.expected_edge_bins():
        exp[b1] += 1
        exp[C.NBINS + b5] += 1
    assert n == ne and (counts == exp).all()
    assert np.isnan(stats[0]) and stats[1] == C.RMIN - 1.0 and stats[2] == 3.9375       # the NaN joins the sum and neither extreme
    assert stats[3] == -0.25 + C.RMAX + (C.RMAX + 0.5) + 1.125 - 4.0 and stats[4] == -4.0 and stats[5] == C.RMAX + 0.5
    full = m.chol_offsets(s.gid7, *ARGS)
    order = np.argsort(s.gid7[:, 0])[::-1]
    desc = m.chol_offsets(s.gid7[order], *ARGS)
    assert (desc[0] == full[0]).all() and desc[2] == full[2] and (desc[1][[1, 2, 4, 5]] == full[1][[1, 2, 4, 5]]).all()
    # one bin, and the cap
    one = m.chol_offsets(s.gid7, C.RMIN, 8.0, 1)
    assert one[0].tolist() == [1025, 1025]
    from ddcmd_amd.martini import DdcmiError
    cap = 8167
    big = m.chol_offsets(s.gid7, C.RMIN, 8.0 / cap, cap)
    assert big[0][:cap].sum() == 1025 and big[0][cap:].sum() == 1025 and (big[1][[1, 2, 4, 5]] == full[1][[1, 2, 4, 5]]).all()
    with pytest.raises(DdcmiError, match="LDS"):
        m.chol_offsets(s.gid7, C.RMIN, 8.0 / cap, cap + 1)
    assert m.chol_offsets(s.gid7, *ARGS)[0].tobytes() == full[0].tobytes()
    m.close()


def test_the_run_is_untouched():
    s = C.made("system", 257, 7)
    rng = np.random.RandomState(3)
    import copy
    s = copy.copy(s)
    v = rng.normal(size=(s.natoms, 3)) * 2e-4
    s.vx, s.vy, s.vz = (np.ascontiguousarray(v[:, c]) for c in range(3))
    out, res = [], []
    for calls in (True, False):
        m = _single(s)
        for _ in range(4):
            m.step(10)
            if calls:
                res.append(m.chol_offsets(s.gid7, *ARGS))
        st = m.download()
        out.append(b"".join(a.tobytes() for k in ("r", "v", "f") for a in st[k]))
        m.close()
    assert out[0] == out[1]
    assert res[0][2] == 257 and any(res[0][0].tobytes() != r[0].tobytes() for r in res[1:])      # (the beads do move)


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2)])
def test_decomposed(grid):
    from ddcmd_amd.martini import DdcmiError, MartiniGroup, CHOL_FRAGMENT, _lp
    s = C.made("split_system")
    nmol = len(s.gid7)
    m = _single(s)
    one = m.chol_offsets(s.gid7, *ARGS)
    m.close()
    assert one[2] == nmol
    g = MartiniGroup(s, grid)
    g.eval_forces()
    counts, ndone, stats, frag, nfrag = g.chol_offsets(s.gid7, *ARGS, per_rank=True)
    merged = g.chol_offsets(s.gid7, *ARGS)
    nsplit = len(np.unique(frag["mol"]))
    expect = len(set(k for a in range(3) if grid[a] == 2 for k in range(nmol)
                     if (s.mol_r[k, :, a] < 0).any() and (s.mol_r[k, :, a] > 0).any()))
    assert nsplit == expect and nsplit >= 4
    assert int(ndone.sum()) + nsplit == nmol and merged[2] == nmol
    assert len(frag) == 7 * nsplit and nfrag.sum() == len(frag)
    off = np.concatenate([[0], np.cumsum(nfrag)])
    for r in range(g.n):      # (mol, role) order within a rank
        key = frag["mol"][off[r]:off[r + 1]].astype(np.int64) * 7 + frag["role"][off[r]:off[r + 1]]
        assert (np.diff(key) > 0).all()
    if grid == (2, 2, 2):
        corner = 9
        owners = [r for r in range(8) if (frag["mol"][off[r]:off[r + 1]] == corner).any()]
        assert len(owners) == 7 and nfrag[7] == 0 and ndone[7] == 0      # a bead in seven bricks; the eighth owns nothing
    # merged counts and extremes are bit for bit the single domain's
    assert merged[0].tobytes() == one[0].tobytes()
    assert (merged[1][[1, 2, 4, 5]] == one[1][[1, 2, 4, 5]]).all()
    assert np.allclose(merged[1][[0, 3]], one[1][[0, 3]], rtol=0, atol=nmol * C.EPS * 6.0)
    # too small a room: the count comes back, the buffer stays as it was
    buf = np.zeros(len(frag), CHOL_FRAGMENT)
    buf["mol"] = -7
    with pytest.raises(DdcmiError, match="capacity"):
        g.chol_offsets(s.gid7, *ARGS, per_rank=True, cap=len(frag) - 1, out=buf)
    assert (buf["mol"] == -7).all()
    r0 = next(r for r in range(g.n) if nfrag[r] > 0)      # the packed fragments of one rank once more, and a room that is too small
    one_n = np.zeros(1, np.int64)
    assert g.lib.ddcmi_chol_fragments(g.ranks[r0].ctx, int(nfrag[r0]) - 1, buf.ctypes.data_as(ctypes.c_void_p), one_n.ctypes.data_as(_lp)) != 0
    assert one_n[0] == nfrag[r0] and (buf["mol"] == -7).all()
    assert g.lib.ddcmi_chol_fragments(g.ranks[r0].ctx, int(nfrag[r0]), buf.ctypes.data_as(ctypes.c_void_p), one_n.ctypes.data_as(_lp)) == 0
    assert buf[:int(nfrag[r0])].tobytes() == frag[off[r0]:off[r0 + 1]].tobytes()
    # a listed gid no rank owns, in a split molecule: named
    bad = s.gid7.copy()
    mol = int(frag["mol"][0])
    bad[mol, 6] = np.uint64(0x7ffffffe) << np.uint64(16)
    with pytest.raises(DdcmiError, match=r"molecule %d: gid %d \(role 6\) is owned by no rank" % (mol, int(bad[mol, 6]))):
        g.chol_offsets(bad, *ARGS)
    assert g.chol_offsets(s.gid7, *ARGS)[0].tobytes() == one[0].tobytes()
    g.close() if hasattr(g, "close") else None


def test_wrong_arguments_leave_the_context_usable():
    from ddcmd_amd.martini import DdcmiError, _lp, _up, _d
    s = C.made("system", 63, 7)
    m = _single(s)
    good = m.chol_offsets(s.gid7, *ARGS)
    dup = s.gid7.copy()
    dup[5, 2] = dup[40, 0]
    for args, pat in (((s.gid7, C.RMIN, C.DELTA, 0), "nbins"), ((s.gid7, C.RMIN, 0.0, 4), "delta"), ((s.gid7, C.RMIN, -1.0, 4), "delta"),
                      ((s.gid7, C.RMIN, float("inf"), 4), "delta"), ((s.gid7, C.RMIN, float("nan"), 4), "delta"),
                      ((s.gid7, float("nan"), C.DELTA, 4), "rmin"), ((s.gid7, float("inf"), C.DELTA, 4), "rmin"),
                      ((dup, C.RMIN, C.DELTA, 4), "gid %d is listed twice" % int(dup[40, 0]))):
        with pytest.raises(DdcmiError, match=pat):
            m.chol_offsets(*args)
    gid = np.ascontiguousarray(s.gid7.reshape(-1))
    counts, ndone, stats, nfrag = np.zeros(2 * C.NBINS, np.int64), np.zeros(1, np.int64), np.zeros(6), np.zeros(1, np.int64)
    tail = (C.RMIN, C.DELTA, C.NBINS, counts.ctypes.data_as(_lp), ndone.ctypes.data_as(_lp), _d(stats), 0, None, nfrag.ctypes.data_as(_lp))
    f = m.lib.ddcmi_chol_offsets
    assert f(m.ctx, -1, gid.ctypes.data_as(_up), *tail) != 0
    assert f(m.ctx, 63, None, *tail) != 0
    assert f(m.ctx, 63, gid.ctypes.data_as(_up), C.RMIN, C.DELTA, C.NBINS, None, ndone.ctypes.data_as(_lp), _d(stats), 0, None, nfrag.ctypes.data_as(_lp)) != 0
    assert not counts.any() and not stats.any()
    assert f(m.ctx, 0, None, C.RMIN, C.DELTA, C.NBINS, None, None, None, 0, None, None) == 0      # nmol = 0 is valid and touches nothing
    again = m.chol_offsets(s.gid7, *ARGS)
    assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
    m.close()


def test_no_state_is_refused():
    from ddcmd_amd import _lib, martini
    lib = _lib.load_library()
    martini._declare(lib)
    ctx = ctypes.c_void_p()
    assert lib.ddcmi_create(ctypes.byref(ctx), 0) == 0
    gid = np.arange(7, dtype=np.uint64)
    counts, ndone, stats, nfrag = np.zeros(8, np.int64), np.zeros(1, np.int64), np.zeros(6), np.zeros(1, np.int64)
    rc = lib.ddcmi_chol_offsets(ctx, 1, gid.ctypes.data_as(martini._up), 0.0, 1.0, 4, counts.ctypes.data_as(martini._lp), ndone.ctypes.data_as(martini._lp),
                                martini._d(stats), 0, None, nfrag.ctypes.data_as(martini._lp))
    assert rc != 0 and b"uploaded state" in lib.ddcmi_last_error(ctx)
    lib.ddcmi_destroy(ctx)

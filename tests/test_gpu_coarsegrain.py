"""GPU tests (-m gpu) of the COARSEGRAIN analysis on the device: ddcmi_coarsegrain and the in-process group's twin against the
numpy.longdouble restatement of coarsegrain_eval (tests/coarsegrain_systems.py), entry by entry.

Structure: the set of (label, species) keys is the reference's, in ascending order; an unsmeared n is the exact integer.  Every other
value lies within (n_terms + 8) 2^-53 sum |term| of the reference's sum, with the reference's sum |term|: the first-order bound of a sum
of n_terms products in any order, each with at most 4 roundings (coarsegrain_systems.bound; the device's terms have at most 3).  No
tolerance is measured.

Shapes, the smallest at which each stage can go wrong: 3 species on 3 x 2 x 5 with 2000 beads (segments straddle waves and workgroups
of the sort); 1 x 1 x 1 with 5000 beads, smeared (three segments of 8000 to 16 000 contributions: many workgroups of the sort, a long
segment of the reduction); 17 x 13 x 11 with 4 species and 300 beads (nearly every key empty, segments of one or two items, two
passes); 41^3 with one species (68 921 keys: a third pass); 2 x 2 x 2 with 64, 65, 256, 257 beads and with one.  Smearing radii:
0.125 internal units (lSmearHalf = 0.125 grid units clamps delta, the weights become exactly 0 and 1 and the reference skips those
corners), 3 A (below half of every cell) and 20 A (above every cell: lSmear is the cell)."""
import ctypes

import numpy as np
import pytest

import coarsegrain_systems as cgs
from coarsegrain_systems import ANG, gas, place, box_of, reference, check_against

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -2, -4
SMEARS = [(0.0, "impulse"), (0.125, "impulse"), (0.125, "hat"), (3.0 * ANG, "impulse"), (3.0 * ANG, "hat"), (20.0 * ANG, "impulse"), (20.0 * ANG, "hat")]


def particles(m):
    from ddcmd_amd.martini import DomainMixin
    return DomainMixin.download_particles(m)


def ref_of(m, s, grid, sr, method, p=None):
    return reference(particles(m) if p is None else p, s.mass, box_of(s), s.pbc, grid[0], grid[1], grid[2], s.nspecies, sr, method)


def hold(m, s, grid, sr=0.0, method="impulse"):
    """one evaluation against the reference; a second call returns the same bytes; the count alone agrees"""
    rec = m.coarsegrain(*grid, smear_radius=sr, smear_method=method)
    ref = ref_of(m, s, grid, sr, method)
    worst = check_against(rec, ref, exact_n=not sr > 0.0)
    assert rec.dtype.itemsize == 80
    assert m.coarsegrain(*grid, smear_radius=sr, smear_method=method).tobytes() == rec.tobytes()
    assert m.coarsegrain(*grid, smear_radius=sr, smear_method=method, count_only=True) == len(ref)
    return rec, ref, worst


def open_ctx(s):
    from ddcmd_amd.martini import MartiniHIP
    return MartiniHIP(s, test_api=True)


@pytest.mark.parametrize("sr,method", SMEARS)
def test_three_species_on_a_small_grid(sr, method):
    s = gas(2000, 3)
    m = open_ctx(s)
    rec, ref, worst = hold(m, s, (3, 2, 5), sr, method)
    print(sr, method, len(rec), "entries, worst error / bound", worst)
    assert len(rec) == 3 * 2 * 5 * 3      # every key is occupied: segments of 20 to 200 contributions or more
    total = rec["n"].sum()
    # a bead's eight weights add up to 1 within 3 roundings; their 16 000 terms to the bound of the sums
    assert total == 2000.0 if not sr > 0.0 else abs(total - 2000.0) <= (8 * 2000 + 8) * cgs.U * 2000.0
    m.close()


def test_the_skip_of_light_corners_changes_the_count():
    """with lSmearHalf = 0.125 grid units most beads have a weight of exactly 0 on some axis: those corners are no contributions, and on a
    sparse grid their cells are no entries"""
    s = gas(300, 4)
    m = open_ctx(s)
    grid = (17, 13, 11)
    p = particles(m)
    key, w, _ = cgs.contributions(p, s.mass, box_of(s), s.pbc, *grid, s.nspecies, 0.125, "impulse")
    assert len(key) < 8 * 300 and (w == 1.0).any()      # corners were skipped, and some bead kept one corner of weight 1
    rec, ref, _ = hold(m, s, grid, 0.125, "impulse")
    wide = m.coarsegrain(*grid, smear_radius=3.0 * ANG)
    assert len(rec) == len(np.unique(key)) < len(wide)
    m.close()


@pytest.mark.parametrize("method", ["impulse", "hat"])
def test_one_cell_with_long_segments(method):
    s = gas(5000, 3)
    m = open_ctx(s)
    rec, ref, worst = hold(m, s, (1, 1, 1), 3.0 * ANG, method)
    print(method, "worst error / bound", worst, [e.n_terms for e in ref.values()])
    assert len(rec) == 3 and min(e.n_terms for e in ref.values()) >= 8000
    rec0, _, _ = hold(m, s, (1, 1, 1))
    assert rec0["n"].tolist() == np.bincount(s.species, minlength=3).astype(float).tolist()
    m.close()


@pytest.mark.parametrize("sr,method", [(0.0, "impulse"), (3.0 * ANG, "hat"), (20.0 * ANG, "impulse")])
def test_a_sparse_grid_of_four_species_takes_two_passes(sr, method):
    s = gas(300, 4)
    m = open_ctx(s)
    rec, ref, worst = hold(m, s, (17, 13, 11), sr, method)
    print(sr, method, len(rec), "entries of up to", max(e.n_terms for e in ref.values()), "terms")
    assert 17 * 13 * 11 * 4 > 256 and max(e.n_terms for e in ref.values()) <= 8 and len(rec) >= 280
    assert rec["label"].max() > 255      # a key beyond the first digit
    m.close()


@pytest.mark.parametrize("sr", [0.0, 3.0 * ANG])
def test_one_species_on_41_cubed_takes_three_passes(sr):
    s = gas(500, 1)
    m = open_ctx(s)
    rec, ref, _ = hold(m, s, (41, 41, 41), sr, "impulse")
    assert 41 ** 3 > 65536 and rec["label"].max() > 65535 and not rec["species"].any()
    m.close()


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257])
def test_block_edges(n):
    s = gas(n, 2)
    m = open_ctx(s)
    for sr, method in SMEARS[:1] + SMEARS[3:5]:
        rec, ref, _ = hold(m, s, (2, 2, 2), sr, method)
        assert sum(e.n_terms for e in ref.values()) == (8 * n if sr > 0.0 else n)
    m.close()


def test_a_species_the_system_lacks():
    i = np.arange(700)
    s = gas(700, 3, species=np.where(i % 3 == 1, 2, 0))
    m = open_ctx(s)
    for sr in (0.0, 3.0 * ANG):
        rec, _, _ = hold(m, s, (4, 3, 2), sr)
        assert set(rec["species"].tolist()) == {0, 2}
    m.close()


def _geometry(pbc):
    """beads exactly on cell faces, on the box's lower and upper faces and at +-L/2, and smeared beads in the first and the last layer"""
    s = gas(40, 2, pbc=pbc, seed=3)
    L = np.array(cgs.BOX_A)
    cell = L / np.array([3.0, 2.0, 5.0])
    k = 0
    for a in range(3):
        for where in (-0.5 * L[a], 0.5 * L[a], -0.5 * L[a] + cell[a], -0.5 * L[a] + 2 * cell[a] if a != 1 else 0.0,
                      -0.5 * L[a] + 0.1 * cell[a], 0.5 * L[a] - 0.1 * cell[a], -0.5 * L[a] + 0.6 * cell[a], 0.5 * L[a] - 0.6 * cell[a]):
            r = [1.0, -2.0, 3.0]
            r[a] = where
            place(s, k, r)
            k += 1
    assert k <= 40
    return s


@pytest.mark.parametrize("pbc", [7, 3, 0])
def test_faces_layers_and_open_axes(pbc):
    s = _geometry(pbc)
    m = open_ctx(s)
    p = particles(m)
    L = box_of(s)
    print("beads exactly on a face of the box:", [int((np.abs(p["r"][a]) == 0.5 * L[a]).sum()) for a in range(3)])
    for sr, method in SMEARS:
        rec, ref, _ = hold(m, s, (3, 2, 5), sr, method)
    if pbc == 3:
        # z is open: the bead 0.1 cells above the lower face still gives weight to the top layer, as in the reference
        z = p["r"][2]
        low = np.flatnonzero(np.abs(z - (-0.5 * L[2] + 0.1 * L[2] / 5)) < 1e-9)
        assert len(low) == 1
        one = {"gid": p["gid"][low], "species": p["species"][low], "r": [a[low] for a in p["r"]], "v": [a[low] for a in p["v"]]}
        ref1 = reference(one, s.mass, L, pbc, 3, 2, 5, s.nspecies, 20.0 * ANG, "impulse")
        assert {k[0] % 5 for k in ref1} == {0, 4}
    m.close()


def test_a_nan_coordinate_goes_to_cell_zero():
    s = gas(70, 2)
    s.rx[5] = np.nan
    s.rz[9] = np.nan
    m = open_ctx(s)
    rec, ref, _ = hold(m, s, (3, 2, 5))
    p = particles(m)
    i5 = int(np.flatnonzero(np.isnan(p["r"][0]))[0])
    key, _, bead = cgs.contributions(p, s.mass, box_of(s), s.pbc, 3, 2, 5, 2, 0.0, "impulse")
    assert (key[bead == i5][0] // 2) // (5 * 2) == 0      # igx = 0
    m.close()


def test_beads_that_left_the_box_between_two_rebuilds_are_wrapped():
    s = gas(2000, 3, update_rate=20)
    m = open_ctx(s)
    m.eval_forces()
    m.step(15)
    L = box_of(s)
    flown = [np.asarray(getattr(s, "r" + c)) + 15 * s.dt * np.asarray(getattr(s, "v" + c)) for c in "xyz"]      # no force acts
    out = sum(int((np.abs(f) > 0.5 * L[a]).sum()) for a, f in enumerate(flown))
    assert out >= 5
    p = particles(m)
    assert all((np.abs(p["r"][a]) <= 0.5 * L[a]).all() for a in range(3))
    for sr, method in ((0.0, "impulse"), (3.0 * ANG, "hat")):
        hold(m, s, (3, 2, 5), sr, method)
    m.close()


def _state(m):
    d = m.download()
    return np.concatenate(d["r"] + d["v"] + d["f"]).tobytes()


def test_the_call_reads_and_the_run_does_not_notice():
    s = gas(2000, 3)
    outs = []
    for calls in (False, True):
        m = open_ctx(s)
        m.eval_forces()
        for k in range(8):
            m.step(5)
            if calls:
                before = _state(m)
                a = m.coarsegrain(6, 5, 4, smear_radius=3.0 * ANG, smear_method="hat")
                b = m.coarsegrain(6, 5, 4)
                assert _state(m) == before and len(a) > 0 and len(b) > 0
        e, vir, rk, t = m.energies()
        outs.append((sorted(e.items()), vir.tobytes(), rk, t.tobytes(), _state(m)))
        m.close()
    assert outs[0] == outs[1]


def test_cap_and_count_protocol():
    from ddcmd_amd.martini import DdcmiError, CG_RECORD
    s = gas(300, 2)
    m = open_ctx(s)
    want = m.coarsegrain(5, 4, 3)
    n = len(want)
    assert n > 10
    out = np.zeros(n, CG_RECORD)
    out["label"], out["n"] = 77, 7.0
    before = out.tobytes()
    with pytest.raises(DdcmiError, match="capacity %d < %d" % (n - 1, n)):
        m.coarsegrain(5, 4, 3, cap=n - 1, out=out)
    assert out.tobytes() == before
    cnt = np.full(1, -5, np.int64)
    lp = ctypes.POINTER(ctypes.c_int64)
    assert m.lib.ddcmi_coarsegrain(m.ctx, 5, 4, 3, 2, 0.0, 0, n - 1, out.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(lp)) == EINVAL
    assert cnt[0] == n and out.tobytes() == before
    cnt[0] = -5
    assert m.lib.ddcmi_coarsegrain(m.ctx, 5, 4, 3, 2, 0.0, 0, 0, None, cnt.ctypes.data_as(lp)) == 0 and cnt[0] == n      # rec = NULL counts
    assert m.coarsegrain(5, 4, 3, cap=n, out=out).tobytes() == want.tobytes()
    m.close()


def test_refusals_leave_their_code_a_message_and_a_usable_context():
    from ddcmd_amd.martini import MartiniHIP, DdcmiError
    s = gas(100, 2)
    m = open_ctx(s)
    want = m.coarsegrain(3, 3, 3)
    cnt = np.zeros(1, np.int64)
    lp = cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    call = lambda *a: m.lib.ddcmi_coarsegrain(m.ctx, *a, 0, None, lp)
    for args, code, word in (((0, 3, 3, 2, 0.0, 0), EINVAL, "nx = 0"), ((3, -1, 3, 2, 0.0, 0), EINVAL, "ny = -1"), ((3, 3, 0, 2, 0.0, 0), EINVAL, "nz = 0"),
                             ((3, 3, 3, 3, 0.0, 0), EINVAL, "nspecies = 3"), ((3, 3, 3, 2, 0.0, 2), EINVAL, "smear_method = 2"),
                             ((3, 3, 3, 2, float("nan"), 0), EINVAL, "smear_radius = nan"), ((3, 3, 3, 2, float("inf"), 0), EINVAL, "smear_radius = inf"),
                             ((1024, 1024, 256, 2, 0.0, 0), EUNSUPPORTED, "at most 268435456"), ((1 << 14, 1 << 14, 1, 2, 0.0, 0), EUNSUPPORTED, "keys")):
        assert call(*args) == code, args
        assert word in m.lib.ddcmi_last_error(m.ctx).decode(), (args, m.lib.ddcmi_last_error(m.ctx).decode())
        assert m.coarsegrain(3, 3, 3).tobytes() == want.tobytes()
    assert call(1024, 1024, 128, 2, 0.0, 0) == 0 and cnt[0] == len(m.coarsegrain(1024, 1024, 128))      # 2^28 keys: the largest grid
    assert m.lib.ddcmi_coarsegrain(m.ctx, 3, 3, 3, 2, 0.0, 0, 0, None, None) == EINVAL
    m.close()
    e = MartiniHIP(s, upload=False)
    with pytest.raises(DdcmiError, match="needs an uploaded state"):
        e.coarsegrain(3, 3, 3)
    e.close()
    t = gas(100, 2)
    t.h = t.h.copy()
    t.h[1] = 0.5 * ANG
    try:
        tri = MartiniHIP(t)
    except DdcmiError:
        return      # (a context that takes no triclinic box has nothing to refuse)
    with pytest.raises(DdcmiError, match="orthorhombic"):
        tri.coarsegrain(3, 3, 3)
    tri.close()


@pytest.mark.parametrize("grid,empty", [((2, 1, 1), True), ((2, 2, 2), False)])
def test_in_process_domains_merge_to_the_one_domain_reference(grid, empty):
    from ddcmd_amd.analysis import merge_cg_records
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP, DdcmiError
    s = gas(1021, 3, seed=5)
    if empty:      # nobody lives in the first domain
        s.rx = np.abs(s.rx) + 0.01 * ANG
    one = MartiniHIP(s)
    g = MartiniGroup(s, grid)
    p1 = particles(one)
    for sr, method in ((0.0, "impulse"), (3.0 * ANG, "hat"), (0.125, "impulse")):
        rec, cnt = g.coarsegrain(6, 5, 4, smear_radius=sr, smear_method=method, per_rank=True)
        assert cnt.shape == (g.n,) and cnt.sum() == len(rec)
        if empty:
            assert cnt[0] == 0 and cnt[1] > 0
        off = np.concatenate([[0], np.cumsum(cnt)])
        blocks, refs = [rec[off[r]:off[r + 1]] for r in range(g.n)], []
        for r, rk in enumerate(g.ranks):      # every domain's block: its own beads
            pr = rk.download_particles()
            refs.append(ref_of(rk, s, (6, 5, 4), sr, method, p=pr))
            check_against(blocks[r], refs[-1], exact_n=not sr > 0.0)
        merged = merge_cg_records(blocks)
        ref = ref_of(one, s, (6, 5, 4), sr, method, p=p1)
        assert sorted(cgs.merge_reference(refs)) == sorted(ref)
        check_against(merged, ref, exact_n=not sr > 0.0)      # n_terms of the merged entry
        assert g.coarsegrain(6, 5, 4, smear_radius=sr, smear_method=method).tobytes() == merged.tobytes()
        total = sum(float(b["n"].sum()) for b in blocks)
        if not sr > 0.0:
            assert total == 1021.0
        else:
            assert abs(total - 1021.0) <= (8 * 1021 + 8) * cgs.U * 1021.0
    tot = int(g.coarsegrain(6, 5, 4, per_rank=True)[1].sum())
    out = np.full(80 * tot, 9, np.uint8)
    before = out.tobytes()
    with pytest.raises(DdcmiError, match="capacity"):
        g.coarsegrain(6, 5, 4, cap=tot - 1, out=out.view(rec.dtype))
    assert out.tobytes() == before
    with pytest.raises(DdcmiError, match="ddcmi_group_coarsegrain"):
        g.ranks[0].coarsegrain(6, 5, 4)
    g.close()
    one.close()

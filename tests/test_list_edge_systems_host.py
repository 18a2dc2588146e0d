"""Host tests of tests/list_edge_systems.py: what tests/test_gpu_list_edge.py takes for granted about its inputs is asserted here --
the references agree, no pair is ambiguous, the pairs sit where the list search decides in single precision, and the band of the exact
test covers the error of the staged arithmetic (the claim of the comment in k_tile_build).

Measured worst |r2_f32 - r2_exact| / rl2 against band / 4 of the pair's tile (emulated on the host, every system): 0.44 of band / 4 -- a pair
of "sweep" (error 3.0e-7, band / 4 6.8e-7); 0.25 for the pairs 1000 A outside the open box (error 6.8e-6, band / 4 2.7e-5), for the outer
ring of a tile ("place") and for the nudged water box (error 3.7e-7, band / 4 1.5e-6).  docs/list_edge_variants.md has the table."""
import numpy as np
import pytest

import list_edge_systems as E

GAS_CASES = [(n, "one_type") for n in E.GAS] + [("sweep", "types20"), ("sweep", "mol"), ("crowded", "one_type")]
ALL_CASES = GAS_CASES + [("nudged_water", "one_type")]


def both_ways(s):
    return np.concatenate([s.pair_i, s.pair_j]), np.concatenate([s.pair_j, s.pair_i])


@pytest.mark.parametrize("name,variant", ALL_CASES)
def test_references_agree_and_no_pair_is_ambiguous(name, variant):
    """the float64 list equals the longdouble list (the water box: on every pair within 2e-3 of the list radius, the only ones the two could
    tell apart), and no pair lies within 2^-45 of the list radius: nothing is excluded from any comparison"""
    s = E.system(name, variant)
    I, J, x = E.near_pairs(s)
    assert E.ambiguous(x) == 0, (name, float(np.abs(x).min()))
    f64 = E.reference_list(s, np.float64) if name != "nudged_water" else E.exact_list(name, variant)
    near_in = set(zip(I[x < 0].tolist(), J[x < 0].tolist())) - set((i, i) for i in range(s.natoms))
    near_all = set(zip(I.tolist(), J.tolist()))
    assert {p for p in f64 if p in near_all} == near_in
    if name != "nudged_water" and variant != "mol":
        assert f64 == E.exact_list(name, variant)
    if variant == "mol":          # every molecule's own pair is inside the list radius and leaves the list
        assert len(f64) - len(E.exact_list(name, variant)) == 2 * E.excluded_pairs(s) == s.natoms
    labelled = set(zip(*[a.tolist() for a in both_ways(s)]))
    assert labelled <= near_all or name != "nudged_water"
    print("%s %s: %d beads, %d ordered pairs in the list, %d within 2e-3 of the list radius, nearest |d2/rl2 - 1| = %.2e" % (
        name, variant, s.natoms, len(f64), len(I), float(np.abs(x).min())))


@pytest.mark.parametrize("name,variant", GAS_CASES)
def test_no_foreign_bead_near_a_probe(name, variant):
    s = E.system(name, variant)
    d = E.foreign_distance(s)
    assert d > E.rlist_of(s) + E.MARGIN_A * E.ANG, (name, d / E.ANG)


def test_every_e_value_on_both_sides():
    s = E.system("sweep")
    sw = s.pair_family == "sweep"
    for e in E.E_VALUES:
        for sign in (1, -1):
            assert (sw & (s.pair_e == sign * e)).sum() == len(E.DIRECTIONS)
    I, J = s.pair_i[sw], s.pair_j[sw]
    r = E.positions(s)
    d = np.asarray(r[I], np.longdouble) - np.asarray(r[J], np.longdouble)
    x = np.sqrt((d * d).sum(axis=1)) / np.longdouble(E.rlist_of(s)) - 1
    # the distances realised in double positions: the sign of every e, and its size to 2e-15 (an ulp of a 300 A coordinate against 30 A)
    assert np.array_equal(np.sign(x), np.sign(s.pair_e[sw]))
    assert np.abs(np.asarray(x, np.float64) - s.pair_e[sw]).max() < 4e-15


@pytest.mark.parametrize("variant", E.VARIANTS)
def test_sweep_straddles_the_band(variant):
    """with the emulated single-precision r^2 and the band of the first bead's tile: pairs below rl2_lo (taken unseen), above rl2_hi (rejected
    unseen) and inside on both sides of the list radius; the band pairs land on the intended side of the band's edges"""
    s = E.system("sweep", variant)
    err, quarter, slack, r2, lo, hi = E.staged_error(s, s.pair_i, s.pair_j)
    inside = s.pair_e < 0
    assert (r2 < lo).sum() > 20 and (r2 > hi).sum() > 20
    assert ((r2 > lo) & (r2 < hi) & inside).sum() > 20 and ((r2 > lo) & (r2 < hi) & ~inside).sum() > 20
    # the searched pairs: single precision puts at least one of them (two for one_type and types20, one for mol) on the wrong side of the list radius, further out than a band of a
    # quarter of the error bound (band / 16) would re-test
    adv = s.pair_family == "adverse"
    wrong = -np.sign(s.pair_e) * (r2.astype(np.float64) / E.rl2_of(s) - 1.0)
    print("adverse pairs beyond band / 16 on the wrong side: %d of %d" % (int((adv & (wrong > quarter / 4.0)).sum()), int(adv.sum())))
    assert (adv & (wrong > quarter / 4.0)).sum() >= 1
    band = s.pair_family == "band"
    for tag, want in (("lo*1.1", r2 < lo), ("lo*0.9", (r2 > lo) & (r2 < hi)), ("hi*0.9", (r2 > lo) & (r2 < hi)), ("hi*1.1", r2 > hi)):
        q = band & (s.pair_tag == tag)
        assert q.sum() == len(E.DIRECTIONS) and want[q].all(), (tag, r2[q], lo[q], hi[q])


@pytest.mark.parametrize("name", ["prune_exact", "prune_eps", "prune_fold", "noncubic"])
def test_prune_pairs_sit_at_faces_with_partners_two_cells_away(name):
    s = E.system(name)
    g = E.grid_of(s)
    r = E.positions(s)
    off = E.cell_offsets(s, g)
    pr = np.flatnonzero(s.pair_family == "prune")
    assert (s.pair_e[pr] < 0).all()
    if name == "prune_fold":
        assert all(g.folded)
    if name in ("prune_exact", "prune_eps"):
        assert list(g.n) == [50, 50, 50]
        width = 1.0 / g.cinv / (0.5 * g.rlist) - 1.0
        assert (np.abs(width) < 1e-15).all() if name == "prune_exact" else (np.abs(width - 1e-12) < 1e-15).all()
    faces = [q for q in pr if s.pair_tag[q] != "corner"]
    assert len(faces) == 36
    for k in range(0, 36, 3):          # the three nudges of one (axis, face, direction)
        trio = faces[k:k + 3]
        a = "xyz".index(str(s.pair_dir[trio[0]])[1])
        for q, nudge in zip(trio, (-1, 0, 1)):
            # on the face = the first double of the cell above it; one ulp below = across; one ulp above = still in that cell
            assert str(s.pair_tag[q]).endswith("%+d ulp" % nudge)
            x = r[s.pair_i[q], a]
            c = int(g.raw_cell(r[s.pair_i[q]])[a])
            at = {-1: np.nextafter(x, np.inf), 0: x, 1: np.nextafter(x, -np.inf)}[nudge]
            assert at == g.face(a, c + (1 if nudge < 0 else 0)), (name, k, nudge)
        o = sorted(abs(int(off[q][a])) for q in trio)
        assert o[0] >= 1 and o[-1] == 2, (name, k, o)
        for q in trio:
            assert all(off[q][b] == 0 for b in range(3) if b != a)
    corners = [q for q in pr if s.pair_tag[q] == "corner"]
    assert len(corners) == 24
    seen = set()
    for q in corners:
        o = tuple(int(v) for v in off[q])
        assert sorted(abs(v) for v in o) == [1, 1, 2], (name, s.pair_dir[q], o)
        seen.add(o)
    assert len(seen) == 24          # (+-2, +-1, +-1) in every order and sign


def test_place_pairs_reach_the_outer_ring():
    s = E.system("place")
    g = E.grid_of(s)
    r = E.positions(s)
    loc = g.owned_cell(r[s.pair_i]) + g.m - TCt(g, r[s.pair_i])
    off = E.cell_offsets(s, g)
    assert {tuple(l) for l in loc.tolist()} == {(0, 0, 0), (7, 0, 0), (0, 3, 0), (7, 3, 0), (0, 0, 3), (7, 0, 3), (0, 3, 3), (7, 3, 3), (4, 2, 2)}
    ploc = loc + off
    outside = ((ploc < 0) | (ploc >= E.TC)).any(axis=1)
    ring = ((ploc == -2) | (ploc == E.TC + 1)).any(axis=1)
    corner = (loc != E.TC // 2).any(axis=1)
    assert outside[corner].all() and ring[corner].all()
    am = E.tile_amax(s, g)
    amax = np.array([am[tuple(t)] for t in g.tile_of(r[s.pair_i]).tolist()]) / E.ANG
    print("largest staged coordinate per tile: %.1f - %.1f A" % (amax.min(), amax.max()))
    xout = corner & (np.abs(off[:, 0]) == 2)
    assert xout.sum() >= 16 and amax[xout].min() > 5.0 * 8.0 and amax[corner].min() > 3.9 * 8.0 and amax.max() < 6.0 * 8.1


def TCt(g, r):
    return E.TC * g.tile_of(r)


def test_images_and_domain_faces():
    """face pairs straddle a periodic face, domain pairs a mid plane; "on" partners lie exactly on the plane or 1e-13 off it"""
    s = E.system("sweep")
    r, L = E.positions(s), E.box_of(s)
    for q in np.flatnonzero(s.pair_family == "face"):
        a = int(str(s.pair_tag[q]).split()[1])
        xi, xj = r[s.pair_i[q], a], r[s.pair_j[q], a]
        assert xi * xj < 0 and abs(xi - xj) > 0.5 * L[a]
    nd = 0
    for q in np.flatnonzero(s.pair_family == "domain"):
        w = str(s.pair_tag[q]).split()
        a = int(w[1])
        xi, xj = r[s.pair_i[q], a], r[s.pair_j[q], a]
        if len(w) > 2:
            assert xi == float(w[3]) and xj < 0
        else:
            assert xi < 0 < xj
        nd += 1
    assert nd == 24
    for name in ("open", "mixed"):
        s = E.system(name)
        r, L = E.positions(s), E.box_of(s)
        out = s.pair_family == "outside"
        far = np.abs(r[s.pair_i[out]]).max(axis=1) - 0.5 * L.max()
        assert (far > 2.4 * E.rlist_of(s)).all() and (far > 990 * E.ANG).sum() == (4 * 3 if name == "open" else 4)


@pytest.mark.parametrize("pgrid", [(1, 1, 1), (2, 1, 1), (2, 2, 2)])
def test_face_cell_images_land_in_an_owned_cell_without_the_side_forcing(pgrid):
    """"face_cell": the image (one domain) or the received copy (a 2-way split) of the first bead lies exactly on the high face of the domain
    that stages it, `floor((r - lo) * cinv)` alone files it in the last interior cell n - 1, and that cell holds an owned bead of the same
    site, the third one: halo_cell's side forcing is all that keeps the image out of an owned cell.  The partner is inside the list radius"""
    s = E.system("face_cell")
    r, L = E.positions(s), E.box_of(s)
    fc = np.flatnonzero(s.pair_family == "facecell")
    assert len(fc) == 6 and len(s.face_third) == 6 and (s.pair_e[fc] < 0).all()
    seen = 0
    for q, third in zip(fc, s.face_third):
        kind, _, a = str(s.pair_tag[q]).split()
        a = int(a)
        i = s.pair_i[q]
        assert r[i, a] == (-0.5 * L[a] if kind == "periodic" else 0.0)
        if kind == "mid" and pgrid[a] == 1:
            continue          # a mid-plane bead of an unsplit axis is an interior bead
        img = r[i].copy()
        if kind == "periodic":
            img[a] += L[a]
        # the domain that owns the third bead: the highest along a for the image beyond the box face, the low one at the mid plane
        pcoord = [0 if pgrid[b] == 1 or r[third, b] < 0 else 1 for b in range(3)]
        assert pcoord[a] == (pgrid[a] - 1 if kind == "periodic" else 0)
        g = E.grid_of(s, pgrid, pcoord)
        assert img[a] == g.lo[a] + L[a] / pgrid[a]                       # exactly on the domain's high face
        assert g.raw_cell(img)[a] == g.n[a] - 1                          # and yet filed inside without the forcing
        assert np.array_equal(g.raw_cell(img), g.raw_cell(r[third]))     # in the cell of an owned bead
        assert (g.raw_cell(r[third]) >= 0).all() and (g.raw_cell(r[third]) < g.n).all()
        seen += 1
    assert seen == 3 + sum(p == 2 for p in pgrid), seen


@pytest.mark.parametrize("name,variant", ALL_CASES)
def test_float_error_is_below_a_quarter_of_the_band(name, variant):
    """the comment's own claim, on the emulated staged arithmetic of every labelled pair both ways round and (water) every pair within 2e-3
    of the list radius: |r2_f32 - r2_exact| / rl2 < band / 4 of the tile, with one float32 ulp of slack for the emulation's double rounding"""
    s = E.system(name, variant)
    if name == "nudged_water":
        I, J, _ = E.near_pairs(s)
    else:
        I, J = both_ways(s)
        far = np.isin(s.pair_family, ["inner"])
        keep = np.concatenate([~far, ~far])
        I, J = I[keep], J[keep]
    err, quarter, slack, r2, lo, hi = E.staged_error(s, I, J)
    k = int(np.argmax(err / quarter))
    print("%s %s: worst |r2_f32 - r2| / rl2 = %.3e against band / 4 = %.3e (ratio %.3f) over %d ordered pairs; slack %.1e" % (
        name, variant, err[k], quarter[k], err[k] / quarter[k], len(I), slack))
    assert (err < quarter - slack).all(), (name, err[k], quarter[k])

"""The builders and the reference of tests/migration_systems.py held to their claims on the CPU, so that tests/test_gpu_migration.py
cannot pass vacuously."""
from fractions import Fraction

import numpy as np
import pytest

import migration_systems as M
from ddcmd_amd.martini import domain_of

NSTEPS = 20
IDS = ["%d%d%d-pbc%d" % (g + (p,)) for g, p in M.GRIDS]
THREES = [(g, p) for g, p in M.GRIDS if max(g) >= 3]


def _codes_of(planted_key, grid):
    """the direction code k_mig_classify gives a bead that leaves `rank` along the physical direction d"""
    rank, d, _ = planted_key
    pc = (rank % grid[0], (rank // grid[0]) % grid[1], rank // (grid[0] * grid[1]))
    dd = []
    for a in range(3):
        if d[a] == 0 or grid[a] > 2:
            dd.append(d[a])
        else:
            dd.append(1 if pc[a] == 0 else -1)        # P = 2: the other brick, through whichever face
    return (dd[0] + 1) + 3 * (dd[1] + 1) + 9 * (dd[2] + 1)


def test_fma64_is_the_correctly_rounded_fma():
    rng = np.random.RandomState(1)
    a, x, p = rng.normal(size=4000), rng.normal(size=4000), rng.normal(size=4000) * 100
    # products that end exactly half-way between two doubles of the sum, and a hair off it
    p[:100] = 1.0
    a[:100] = 2.0 ** -53
    x[:100] = 1.0 + rng.randint(0, 3, 100) * 2.0 ** -52
    want = np.array([float(Fraction(float(ai)) * Fraction(float(xi)) + Fraction(float(pi))) for ai, xi, pi in zip(a, x, p)])
    assert (M.fma64(a, x, p) == want).all()


def test_owner_exact_is_the_rational_statement():
    box = np.array(M.BOX_A) * M.ANG
    rng = np.random.RandomState(2)
    r = rng.uniform(-0.7, 0.7, (300, 3)) * box
    for grid, pbc in (((3, 2, 1), 7), ((4, 1, 1), 6), ((1, 3, 1), 5)):
        got = M.coords_exact(r, box, grid, pbc)
        for i in range(len(r)):
            for a in range(3):
                assert got[i, a] == M.brick_exact(r[i, a], box[a], grid[a], M.per_axis(pbc)[a])
    # the edges of the statement: +L/2 is not wrapped and clamps to the last brick, -L/2 is brick 0, an open axis clamps
    L = box[0]
    assert M.brick_exact(0.5 * L, L, 3, True) == 2 and M.brick_exact(-0.5 * L, L, 3, True) == 0
    assert M.brick_exact(np.nextafter(0.5 * L, np.inf), L, 3, True) == 0 and M.brick_exact(np.nextafter(-0.5 * L, -np.inf), L, 3, True) == 2
    assert M.brick_exact(0.9 * L, L, 3, False) == 2 and M.brick_exact(-0.9 * L, L, 3, False) == 0


@pytest.mark.parametrize("grid,pbc", M.GRIDS, ids=IDS)
def test_crossers_take_every_direction(grid, pbc):
    s = M.system("crossers", grid, pbc)
    assert 1000 <= s.natoms <= 4000
    snaps = M.snapshots(s, NSTEPS)
    census = M.direction_census(s, grid, snaps)
    box = M.box_of(s)
    total = census[1][0] + census[2][0]
    want = np.zeros(27, int)
    for key, idx in s.planted.items():
        want[_codes_of(key, grid)] += len(idx)
    assert (total == want).all(), (total, want)
    codes = {_codes_of(k, grid) for k in s.planted}
    assert codes == set(M.possible_codes(grid, pbc))
    for c in codes:
        assert census[1][0][c] >= 8 and census[2][0][c] >= 4, (c, census[1][0][c], census[2][0][c])
    assert census[1][2] == 0 and census[2][2] == 0
    # every planted bead changes brick in its own period, to the brick its direction names, and nobody else moves
    for (rank, d, wave), idx in s.planted.items():
        own = [M.owner_exact(snaps[k][idx], box, grid, pbc) for k in range(3)]
        assert (own[0] == rank).all() and (own[wave] != rank).all() and (own[wave - 1] == rank).all()
        assert (own[2] == own[wave]).all()
    bg = np.setdiff1d(np.arange(s.natoms), s.planted_all)
    assert (M.owner_exact(snaps[0][bg], box, grid, pbc) == M.owner_exact(snaps[2][bg], box, grid, pbc)).all()
    # nobody is near a face at a rebuild: no owner is left open, and the margins hold against the passengers' perturbation
    for r in snaps:
        assert not M.near_face(r, box, grid, pbc).any()
        assert M.min_face_distance(r, s).min() >= M.MARGIN_A
    assert M.perturbation_bound(M.system("crossers", grid, pbc, passengers=True), 30) < 0.01 * M.MARGIN_A


@pytest.mark.parametrize("grid,pbc", M.GRIDS, ids=IDS)
def test_face_sitters_are_the_only_open_cases(grid, pbc):
    s = M.system("face_sitters", grid, pbc)
    assert 1000 <= s.natoms <= 4000
    box = M.box_of(s)
    snaps = M.snapshots(s, NSTEPS)
    nf = M.near_face(M.positions(s), box, grid, pbc)
    assert nf.sum() == len(s.planted["face"]) and nf[s.planted["face"]].all()            # the cap on the open cases; no unplanted bead among them
    for r in snaps:
        now = M.near_face(r, box, grid, pbc)
        assert not now[np.setdiff1d(np.arange(s.natoms), s.planted["face"])].any()
        assert now[s.planted["face"]][s.at_rest[s.planted["face"]]].all()
    # every k in -2 ... 2 stands on both sides of the rational face or on it: the planted set straddles every plane
    c0 = M.coords_exact(M.positions(s)[s.planted["face"]], box, grid, pbc)
    for a in range(3):
        if grid[a] > 1:
            assert len(np.unique(c0[:, a])) == grid[a]
    # outside the box on an open axis: the edge brick
    per = M.per_axis(pbc)
    out = s.planted["outside"]
    assert (len(out) > 0) == any(grid[a] > 1 and not per[a] for a in range(3))
    if len(out):
        r = M.positions(s)[out]
        c = M.coords_exact(r, box, grid, pbc)
        beyond = np.abs(r) > 0.5 * box
        assert beyond.any(axis=1).all() and (np.abs(r) / box).max() > 0.9
        for a in range(3):
            b = beyond[:, a]
            assert (c[b, a] == np.where(r[b, a] > 0, grid[a] - 1, 0)).all()
    ps = M.system("face_sitters", grid, pbc, passengers=True)
    assert ps.nrest > 0 and (np.asarray(ps.group)[ps.planted_all] == 3).any()
    # a restrained sitter feels nothing along the axis of its face
    nfa = M.near_face_axes(M.positions(ps)[ps.rest_bead], box, grid, pbc)
    assert nfa.any(axis=1).all() and (np.asarray(ps.rest_fc)[nfa] == 0).all()


@pytest.mark.parametrize("grid,pbc", M.GRIDS, ids=IDS)
def test_bricks_are_a_list_radius_wide(grid, pbc):
    W = np.array(M.BOX_A) / np.array(grid)
    assert (W[np.array(grid) > 1] >= M.RLIST_A).all()
    # along x and y, the axes that are divided in three, neither L / 3 nor a plane k L / 3 - L / 2 is a double
    L = M.box_of(M.system("crossers", grid, pbc))
    for a in (0, 1):
        assert Fraction(float(L[a])) / 3 != Fraction(float(L[a]) / 3)
        for f in M.faces_exact(L[a], 3)[1:3]:
            assert Fraction(float(f)) != f


@pytest.mark.parametrize("grid,pbc", THREES, ids=["%d%d%d-pbc%d" % (g + (p,)) for g, p in THREES])
def test_two_hops_land_two_bricks_away(grid, pbc):
    s = M.system("two_hops", grid, pbc)
    box = M.box_of(s)
    snaps = M.snapshots(s, M.UPDATE)
    a = s.axis
    far = 2 if M.per_axis(pbc)[a] else grid[a] - 1
    c0, c1 = M.coords_exact(snaps[0], box, grid, pbc), M.coords_exact(snaps[1], box, grid, pbc)
    assert (c0[s.planted["out"], a] == 0).all() and (c1[s.planted["out"], a] == far).all()
    assert (c0[s.planted["back"], a] == far).all() and (c1[s.planted["back"], a] == 0).all()
    assert far >= 2
    cnt, nloc, nfar = M.direction_census(s, grid, snaps)[1]
    assert s.legal == (M.per_axis(pbc)[a] and grid[a] == 3)
    assert nfar == (0 if s.legal else 16) and cnt.sum() == (16 if s.legal else 0)
    assert M.min_face_distance(snaps[1], s).min() >= M.MARGIN_A and not M.near_face(snaps[1], box, grid, pbc).any()


@pytest.mark.parametrize("variant", ["face", "corner"])
def test_crowd_exceeds_the_first_capacity(variant):
    s = M.system("crowd", variant)
    snaps = M.snapshots(s, M.UPDATE)
    cnt, nloc, nfar = M.direction_census(s, s.grid, snaps)[1]
    first_cap = max(1024, int(M.direction_census(s, s.grid, snaps)[0][1][0]) // 16)
    assert first_cap == 1024 and cnt[s.code] == M.NCROWD > first_cap and cnt.sum() == M.NCROWD and nfar == 0
    assert s.natoms <= 4000 and M.min_face_distance(snaps[1][s.planted_all], s).min() >= M.MARGIN_A


def test_passengers_deal_every_kind_into_every_planted_set():
    s = M.system("crossers", (2, 2, 2), 7, passengers=True)
    for key, idx in s.planted.items():
        assert set(np.asarray(s.group)[idx]) == {0, 1, 2} and set(np.asarray(s.species)[idx]) == {0, 1}
    assert len(set(zip(s.lcg64["prime"].tolist(), s.lcg64["multID"].tolist()))) == s.natoms
    assert s.nrest >= len(s.planted_all) // 5 and (np.asarray(s.gid) & np.uint64(0xffffffff) == 0).all()
    assert len(np.unique(s.gid)) == s.natoms and (np.diff(np.asarray(s.gid).astype(np.int64)) < 0).any()


@pytest.mark.parametrize("grid,pbc", M.GRIDS, ids=IDS)
def test_owner_exact_agrees_with_domain_of_away_from_faces(grid, pbc):
    for name in ("crossers", "face_sitters"):
        s = M.system(name, grid, pbc)
        box = M.box_of(s)
        away = ~M.near_face(M.positions(s), box, grid, pbc)
        assert (domain_of(s, grid)[away] == M.owner_exact(M.positions(s), box, grid, pbc)[away]).all()


def test_returners_cross_and_come_back():
    s = M.system("returners")
    box = M.box_of(s)
    snaps = M.returners_reference(s)
    own = [M.owner_exact(r, box, s.grid, s.pbc) for r in snaps]
    pl = s.planted_all
    assert len(pl) == 4 * M.NRETURN and (own[1][pl] != own[0][pl]).all() and (own[2] == own[0]).all()
    assert (np.delete(own[1], pl) == np.delete(own[0], pl)).all()
    for r in snaps:
        assert M.min_face_distance(r, s).min() >= M.MARGIN_A and not M.near_face(r, box, s.grid, s.pbc).any()
    assert (M.velocities(s)[pl, 0] == np.asarray(s.group_v).reshape(3, 3)[np.asarray(s.group)[pl], 0]).all()


def test_many_species_puts_every_planted_bead_above_255():
    s0 = M.system("crossers", (2, 2, 2), 7, passengers=True)
    s = M.many_species(s0)
    sp = np.asarray(s.species)
    assert (sp[s.planted_all] >= 256).all() and sp.max() < s.nspecies == 300 and (sp % 2 == np.asarray(s0.species)).all()
    m, m0 = np.asarray(s.mass)[sp], np.asarray(s0.mass)[np.asarray(s0.species)]
    assert (m == m0 * np.where(sp >= 256, 1.25, 1.0)).all() and len(s.ljtype) == 300
    assert (np.asarray(s.mass)[sp[s.planted_all] & 0xff] != m[s.planted_all]).all()          # taken for id & 0xff: another mass
    for key, idx in s.planted.items():
        assert len(set((sp[idx] & 0xff).tolist()) ^ set(sp[idx].tolist())) > 0          # the low eight bits alone name other species

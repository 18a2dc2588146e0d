"""CPU tests (-m "not gpu") of tests/constraint_systems.py: the builders ARE what their docstrings say, the longdouble solver is tied to
the oracle's port of velocityConstraintOld on the lipid deck, molecular_virial to orc_barostat_mol's pressure, and the tolerances of
tests/test_gpu_constraints.py are measured here: the one-step and the 40-step constants on every run the GPU tests make, the barostat
run included (the 40-step measurements carry the file's run time: a float64 and a longdouble run of every builder)."""
import os

import numpy as np
import pytest

import pyoracle
import constraint_systems as C
from constraint_systems import LD

IDS = ["-".join(str(x) for x in k) for k in C.CONSTRAINT_SETS]


@pytest.mark.parametrize("key", C.CONSTRAINT_SETS, ids=IDS)
def test_builders_and_one_step_tolerance(key):
    """gids name the molecules, beads are shuffled, three species 1 : 4 : 20, the guard holds; one reference step brings every healthy
    pair home (off_length: from up to 3 % off) and the float64 mirror stays within the committed constants of longdouble"""
    s, t = C.system(*key)
    assert 150 <= s.natoms <= 1600 and len(set(box := tuple(C.box_of(s)))) == 3
    assert np.allclose(np.asarray(s.mass) / s.mass[0], [1, 4, 20])
    from ddcmd_amd.martini import molecule_lists
    nmol, off, atoms = molecule_lists(s)
    assert len(off) - 1 == len(s.groups) and sorted(np.diff(off).tolist()) == sorted(len(g) for g in s.groups)
    assert not np.array_equal(np.argsort(s.gid), np.arange(s.natoms))
    C.assert_guard(s, t)
    skip = getattr(s, "stuck_groups", ())
    r, v, bx, most, bad, nbad = C.step(s, t, 1)
    assert nbad == 2 * len(skip)
    assert np.flatnonzero(bad).tolist() == list(skip)
    res_r, res_v = C.pair_residuals(r, v, t, s.dt, bx, s.pbc)
    ok = np.ones(len(t[1]), bool)
    for g in skip:
        ok[t[0][g]:t[0][g + 1]] = False
    assert res_r[ok].max() <= C.LEN_MULT * C.TOL and res_v[ok].max() <= C.VEL_MULT * C.TOL, (float(res_r[ok].max()), float(res_v[ok].max()))
    dr, dv = C.measure(s, t, 1, skip=skip)
    print("%s: one step |dr| %.3e A |dv| %.3e, %d sweeps" % (s.name, dr / C.ANG, dv, most))
    assert dr <= C.POS_MEASURED and dv <= C.VEL_MEASURED, (dr / C.ANG, dv)
    if key[0] == "slow":
        assert most >= 50
    if key[0] == "off_length":
        r0 = C.pair_residuals(C.positions(s), C.velocities(s), t, s.dt, bx, s.pbc)[0]
        assert 0.05 < r0.max() < 0.0625
    if key[0] == "domains":
        from ddcmd_amd.martini import domain_of
        own = domain_of(s, s.grid)
        assert len(set(own[s.groups[s.corner_group]].tolist())) == int(np.prod(s.grid))
        assert sum(len(set(own[g].tolist())) > 1 for g in s.groups) >= 3 * sum(x == 2 for x in s.grid)


def test_lds_budget_arithmetic():
    assert C.lds_items(C.system("chains", 18)[1]) == 123 and C.lds_items(C.system("rings")[1]) == 126
    assert C.lds_items(C.system("too_large")[1]) == 130 > 128
    assert C.lds_items(C.system("mixed", 129)[1]) == 126


RUNS = [(k, False) for k in C.TRAJ_SETS] + [(("faces", 7), True), (("domains", (2, 1, 1)), True)]


@pytest.mark.parametrize("key,baro", RUNS, ids=["-".join(str(x) for x in k) + ("-barostat" if b else "") for k, b in RUNS])
def test_trajectory_tolerance(key, baro):
    """a fresh measurement of the 40-step constants on every 40-step run of the GPU tests, the barostat run included (and of the
    one-step constants under the barostat); the pairs stay away from half the box over the run"""
    s, t = C.system(*key)
    s = C.with_barostat(s) if baro else s
    skip = getattr(s, "stuck_groups", ())
    dr, dv = C.measure(s, t, C.NSTEPS, dts=C.traj_dts(s, key), barostat=baro, skip=skip)
    print("%s: %d steps |dr| %.3e A |dv| %.3e" % (s.name, C.NSTEPS, dr / C.ANG, dv))
    assert dr <= C.TRAJ_R_MEASURED and dv <= C.TRAJ_V_MEASURED, (dr / C.ANG, dv)
    if baro:
        dr, dv = C.measure(s, t, 1, barostat=True)
        assert dr <= C.POS_MEASURED and dv <= C.VEL_MEASURED, (dr / C.ANG, dv)
        ref = C.step(s, t, 1, barostat=True)
        assert (np.abs(np.asarray(ref[2], float) / C.box_of(s) - 1) > 5e-4).all()
    else:
        ref = C.reference_run(key, C.NSTEPS)
        C.assert_guard(s, t, np.asarray(ref[0], float))
        assert np.isfinite(np.asarray(ref[1], float)).all()


def _lipid():
    from ddcmd_amd.deck import load_deck
    from test_oracle import CONSTRAINT_X
    deck = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lipid_deck")
    return load_deck(os.path.join(deck, "object_nvt.data"), restart_file=os.path.join(deck, "relaxed", "restart"), extra_objects=CONSTRAINT_X)


@pytest.mark.parametrize("front", [True, False], ids=["front", "back"])
def test_solver_agrees_with_the_oracle_on_the_lipid_deck(front):
    """the port of velocityConstraintOld (oracle) against solve() on the lipid deck's CONSTRAINT_X groups: velocities within the measured
    one-step tolerance, the same largest sweep count"""
    from ddcmd_amd.martini import expand_constraints
    s = _lipid()
    t = expand_constraints(s)
    o = pyoracle.Oracle(s, constraints=True)
    most = o.constraint_sweep(0 if front else 1)
    v, sw, bad = C.solve(C.positions(s), C.velocities(s), (LD(1) / np.asarray(s.mass, LD))[s.species], t, s.dt, C.box_of(s), s.pbc, front)
    dv = np.abs(np.stack([o.vx, o.vy, o.vz], 1) - v).max()
    print("lipid deck, %s: |dv| %.3e, sweeps %d / %d" % ("FRONT" if front else "BACK", float(dv), most, sw.max()))
    assert dv <= C.FACTOR * C.VEL_MEASURED and most == sw.max() and not bad.any()


def test_molecular_virial_agrees_with_the_oracle():
    """orc_barostat_mol's pressure on the lipid deck: pmol V - N kT = vir - molv with molv from molecular_virial"""
    import ctypes
    s = _lipid()
    o = pyoracle.Oracle(s)
    o.forces()
    s.mols = C.molecule_table(s)
    r, f = C.positions(s), np.stack([o.fx, o.fy, o.fz], 1)
    vir = o.virial.copy()
    box = C.box_of(s).copy()
    T = C.KT
    o.step_npt(0, T, 0.0, 0.0, 1.0)
    pm = np.zeros(3)
    dp = ctypes.POINTER(ctypes.c_double)
    o.L.orc_barostat_mol(ctypes.byref(o.p), o.n, o.rx.ctypes.data_as(dp), o.ry.ctypes.data_as(dp), o.rz.ctypes.data_as(dp),
                         o.fx.ctypes.data_as(dp), o.fy.ctypes.data_as(dp), o.fz.ctypes.data_as(dp), o.gid.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                         o.species.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), vir.ctypes.data_as(dp), ctypes.c_double(T), ctypes.c_double(0.0),
                         ctypes.c_double(1e-30), ctypes.c_double(1.0), ctypes.c_double(s.dt), pm.ctypes.data_as(dp))
    from ddcmd_amd.martini import molecule_lists
    nkt = molecule_lists(s)[0] * T
    molv, mag, nterm = C.molecular_virial(s, r, f, box)
    lhs = np.asarray(pm, LD) * LD(np.prod(box)) - LD(nkt)
    rhs = np.asarray(vir[:3], LD) - molv
    bound = 4 * nterm * mag * LD(C.U) + 4 * LD(C.U) * (abs(LD(nkt)) + np.abs(np.asarray(vir[:3], LD)) + nterm * mag)
    print("lipid deck: |(pmol V - N kT) - (vir - molv)| / bound", np.asarray(np.abs(lhs - rhs) / bound, float))
    assert (np.abs(lhs - rhs) <= bound).all()


@pytest.mark.parametrize("n", C.MOL_COUNTS)
def test_molecules(n):
    s = C.system("molecules", n)
    assert len(s.mols) == n and max(len(m) for m in s.mols) == 300 and (n == 1 or min(len(m) for m in s.mols) == 2)
    # the first listed atom (k = 0) is anywhere in the molecule: over the molecules of five or more beads it is neither always the
    # bead nearest to the centroid nor always the farthest, and its rank by distance from the centroid takes several values
    r, box = C.positions(s), C.box_of(s)
    ranks = []
    for m in s.mols:
        if len(m) >= 5:
            x = C.min_image(r[m] - r[m[0]], box, s.pbc)
            d = np.sqrt(((x - x.mean(axis=0)) ** 2).sum(axis=1))
            ranks.append(float(np.argsort(np.argsort(d))[0]) / (len(m) - 1))
    if n > 1:
        assert len(ranks) >= 5 and min(ranks) < 0.34 and max(ranks) > 0.66 and len(set(ranks)) >= 3, ranks
    else:
        assert 0.0 < ranks[0] < 1.0
    C.assert_molecules(s)


@pytest.mark.parametrize("grid", C.GRIDS, ids=["2x1x1", "1x1x2", "2x2x2"])
def test_split_molecules(grid):
    s = C.system("molecules_split", grid)
    own, _ = C.owners(s, grid)
    counts = set(len(o) for o in own)
    assert {1, 2} <= counts and (grid != (2, 2, 2) or {4, 8} <= counts) and s.nsplit == sum(len(o) > 1 for o in own) > 0


@pytest.mark.parametrize("pbc", C.PBCS)
def test_molecules_faces(pbc):
    s = C.system("molecules_faces", pbc)
    r, box = C.positions(s), C.box_of(s)
    # a molecule across a periodic face has wrapped beads: raw coordinates further apart than half the side.  Every periodic axis has
    # molecules across its face from the centre placed at - L / 2 and from the one placed at + L / 2; pbc 7: one molecule is across all
    # three (the corner), three across two (the edges); nothing is across an open axis
    span = np.array([np.ptp(r[m], axis=0) for m in s.mols]) > 0.5 * box
    for a in range(3):
        assert span[:, a].sum() >= (2 if (pbc >> a) & 1 else 0) and ((pbc >> a) & 1 or not span[:, a].any()), (pbc, a, span[:, a].sum())
    if pbc == 7:
        assert (span.sum(axis=1) == 3).sum() >= 1 and (span.sum(axis=1) == 2).sum() >= 3
    C.assert_molecules(s)

"""CPU tests (-m "not gpu") of tests/restraint_systems.py: the longdouble reference of the RESTRAINT potential is held against the
finite difference of its own energy, against its virial formed a second way and against the oracle; the builders ARE what their
docstrings say (isolation, counts, the 1e-9 guard, the lipid deck's three bead kinds); the trajectory tolerance of
tests/test_gpu_restraints.py is measured here."""
import copy

import numpy as np
import pytest

import pyoracle
import restraint_systems as R
from restraint_systems import LD, U

SETS = R.STEP0_SETS + [("soft_gas",)]
IDS = ["-".join(str(x) for x in k) for k in SETS]


def _ref(key, **kw):
    s = R.system(*key)
    return s, R.reference(s, R.positions(s), R.box_of(s), s.pbc, **kw)


@pytest.mark.parametrize("key", SETS, ids=IDS)
def test_force_is_the_finite_difference_of_the_energy(key):
    """central differences of every restraint's own energy, h = 1e-8 A (inside the 1e-9 L guard: no image changes); the energy is
    quadratic, so the difference is exact up to longdouble rounding: 1e-7 of kb fc L"""
    s, ref = _ref(key)
    r = R.positions(s).astype(LD)
    h = LD(1e-8) * LD(R.ANG)
    box = R.box_of(s)
    have = ref["bead"] >= 0
    for a in range(3):
        rp, rm = r.copy(), r.copy()
        rp[:, a] += h; rm[:, a] -= h
        ep = R.reference(s, rp, box, s.pbc)["e"]
        em = R.reference(s, rm, box, s.pbc)["e"]
        fd = -(ep - em) / (2 * h)
        scale = np.asarray(s.rest_kb, LD) * np.maximum(np.abs(np.asarray(s.rest_fc)[:, a]), 1) * box[a]
        assert (np.abs(fd - ref["f"][:, a])[have] <= 1e-7 * scale[have]).all(), (key, a)
    assert (ref["f"][~have] == 0).all() and (ref["e"][~have] == 0).all()


@pytest.mark.parametrize("key", SETS, ids=IDS)
def test_virial_formed_a_second_way(key):
    """V_ab = -2 sum kb fc_a fc_b d_a d_b straight from the displacements; the energy is -(V_xx + V_yy + V_zz) / 2 only where every
    fc is 0 or 1 (fc = 2 enters the virial squared): checked there"""
    s, ref = _ref(key)
    fc = np.asarray(s.rest_fc).astype(LD)
    kb = np.asarray(s.rest_kb, LD)
    have = (ref["bead"] >= 0).astype(LD)
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        V = (-2 * kb * have * fc[:, a] * fc[:, b] * ref["d"][:, a] * ref["d"][:, b]).sum()
        assert abs(V - ref["V"][k]) <= (s.nrest + 8) * LD(2) ** -64 * ref["Vabs"][k], (key, k)          # (two longdouble sums of n terms of three roundings each)
    if np.asarray(s.rest_fc).max() <= 1:
        assert abs(ref["E"] + ref["V"][:3].sum() / 2) <= 1e-17 * ref["Eabs"]


@pytest.mark.parametrize("key", SETS, ids=IDS)
def test_reference_agrees_with_the_oracle_and_the_gas_is_isolated(key):
    """the oracle's restatement in double against the reference: forces to the bound the device is held to (R.force_bound), energy and
    virial to (n + 16) u of the sums of absolute terms; the oracle's nonbonded force, energy and virial on the gas -- the forces of a
    copy of the Setup without its restraints -- are == 0.0 in every component"""
    s, ref = _ref(key)
    o = pyoracle.Oracle(s)
    e, vir = o.forces()
    f = np.stack([o.fx, o.fy, o.fz], 1)
    bound = R.force_bound(s, ref, R.box_of(s))
    assert (np.abs(f - ref["F"]) <= bound).all(), key
    eb, vb = R.sum_bound(s, ref)
    assert abs(e["restraint"] - ref["E"]) <= eb and (np.abs(vir - ref["V"]) <= vb).all(), key
    assert e["total"] - e["restraint"] == 0.0
    bare = copy.copy(s)
    bare.nrest = 0
    ob = pyoracle.Oracle(bare)
    e0, v0 = ob.forces()
    assert all((np.asarray(x) == 0.0).all() for x in (ob.fx, ob.fy, ob.fz)) and (v0 == 0.0).all() and all(x == 0.0 for x in e0.values()), key
    # nobody sits on top of anybody (eps = 0 times an overflowed 1 / r^12 would be a NaN, not a zero)
    r = R.positions(s)
    d = R.min_image(r[:, None, :] - r[None, :, :], R.box_of(s))
    d2 = (d * d).sum(axis=2) + np.eye(len(r))
    assert d2.min() > (1e-3 * R.ANG) ** 2


@pytest.mark.parametrize("key", SETS, ids=IDS)
def test_conditional_and_unconditional_image_give_the_same_terms(key):
    """the comment of k_restraint held to account: the reference's rule -- the nearest image of the whole vector, and only when a
    component with fc > 0 exceeds half the box -- and the minimum image of every component give identical c, e, f and virial terms"""
    s, a = _ref(key)
    b = R.reference(s, R.positions(s), R.box_of(s), s.pbc, conditional=False)
    for k in ("c", "e", "f", "vir", "F"):
        assert np.array_equal(a[k], b[k]), (key, k)
    R.assert_guard(s)


def test_builder_invariants():
    for n in R.COUNTS:
        s = R.system("gas", n)
        assert s.nrest == n and len(set(s.rest_gid.tolist())) == n and s.natoms == R.NGAS >= 600 + 100
    for key in SETS:
        s = R.system(*key)
        assert 600 <= s.natoms <= 1000, key
        gid = np.asarray(s.gid)
        assert not np.array_equal(gid, np.sort(gid)), "gids in slot order"
        known = s.rest_gid[s.rest_bead >= 0]
        if s.nrest > 2:
            assert not np.array_equal(known, np.sort(known)), "restraints in gid order"
            assert not np.array_equal(s.rest_bead[s.rest_bead >= 0], np.sort(s.rest_bead[s.rest_bead >= 0])), "restraints in slot order"
        assert len(set(s.rest_bead.tolist())) < s.natoms, "nobody unrestrained"
    s = R.system("faces", 7, 0)
    fc = np.asarray(s.rest_fc)
    assert {tuple(p) for p in fc.tolist()} == set(R.PATTERNS)
    assert s.rest_r0.min() < 0 and s.rest_r0.max() > 1 and any(abs(x + 0.2) < 1e-12 for x in s.rest_r0.ravel()) and any(abs(x - 1.3) < 1e-12 for x in s.rest_r0.ravel())
    ref = R.reference(s, R.positions(s), R.box_of(s), 7)
    L = R.box_of(s)
    near = np.abs(np.abs(ref["d_raw"]) / L - 0.5)
    assert ((near < 1.1e-9) & (fc != 0)).sum() == 12 and R.assert_guard(s) >= R.GUARD
    # across a face: the raw displacement is a box side less an angstrom, the image one angstrom
    wrapped = (np.abs(ref["d_raw"]) > L - 1.0 * R.ANG) & (np.abs(ref["d"]) < 1.0 * R.ANG)
    assert wrapped.any(axis=1).sum() == 3 * 4 * 2          # (the four patterns that restrain the face's axis: the reference wraps for a restrained component only)
    assert (wrapped & (fc != 0)).any(axis=1).sum() == 3 * 4 * 2
    for axis in range(3):          # the force changes sign between 0.5 - 1e-9 and 0.5 + 1e-9
        k = np.flatnonzero((near[:, axis] < 1.1e-9) & (fc[:, axis] != 0))
        assert len(k) == 4 and sorted(np.sign(ref["f"][k, axis]).tolist()) == [-1, -1, 1, 1]
    for pbc in R.PBCS:
        s = R.system("faces", pbc, 0)
        ref = R.reference(s, R.positions(s), R.box_of(s), pbc)
        for axis in range(3):
            if not (pbc >> axis) & 1:
                assert np.array_equal(ref["d"][:, axis], ref["d_raw"][:, axis])
    a, b = R.system("faces", 7, 0), R.system("faces", 7, 1)
    assert np.abs((a.rest_r0 - 0.5) - b.rest_r0).max() < 1e-15 and b.rest_origin == 1
    s = R.system("fc_values")
    assert {tuple(p) for p in np.asarray(s.rest_fc).tolist()} == {(a, b, c) for a in (0, 1, 2) for b in (0, 1, 2) for c in (0, 1, 2)}
    ref = R.reference(s, R.positions(s), R.box_of(s), 7)
    off = np.abs(np.asarray(ref["V"][3:], float))
    assert off.min() > 0 and len(set(off.tolist())) == 3
    s = R.system("duplicates")
    cnt = np.bincount(s.rest_bead[s.rest_bead >= 0], minlength=s.natoms)
    assert cnt[s.dup_beads[0]] == 2 and cnt[s.dup_beads[1]] == 3 and (s.rest_bead < 0).sum() == 1 and R.UNKNOWN_GID not in set(np.asarray(s.gid).tolist())
    for b in s.dup_beads:
        k = np.flatnonzero(s.rest_bead == b)
        assert len({tuple(x) for x in s.rest_fc[k].tolist()}) == len(k) and len(set(s.rest_kb[k].tolist())) == len(k)


def test_oscillators_swing_through_cells_faces_and_domains():
    """periods of 40 to 60 steps, amplitude 7 A > one 5 A cell; along the float64 reference trajectory beads cross the periodic faces and
    the mid planes, the anchor of a "dface" bead lies in another half than the bead at the start; the guard holds at every rebuild
    step and at the end; kinds all present"""
    from ddcmd_amd.martini import domain_of
    s = R.system("oscillators")
    fc = np.asarray(s.rest_fc)
    m = s.mass[s.species[s.rest_bead]]
    w = np.sqrt(2.0 * s.rest_kb[:, None] * fc / m[:, None])
    period = 2.0 * np.pi / w[fc > 0] / s.dt
    assert period.min() >= 40.0 - 1e-9 and period.max() <= 60.0 + 1e-9, (period.min(), period.max())
    assert R.AMPLITUDE_A > 0.5 * (s.rmax + s.deltaR) / R.ANG
    assert set(s.kind.tolist()) == {"bulk", "pface", "dface"}
    run = R.LDReference(s)
    box = R.box_of(s)
    r0 = R.positions(s)
    owner0 = domain_of(s, (2, 2, 2))
    crossed_face = np.zeros(s.natoms, bool)
    changed_domain = np.zeros(s.natoms, bool)
    for n in range(1, 61):
        r, v = run.step()
        crossed_face |= (np.abs(r) > 0.5 * box).any(axis=1)
        if n % 10 == 0:
            sn = copy.copy(s)
            sn.rx, sn.ry, sn.rz = (np.ascontiguousarray(r[:, c]) for c in range(3))
            changed_domain |= domain_of(sn, (2, 2, 2)) != owner0
            R.assert_guard(s, r)
    assert crossed_face[s.rest_bead[s.kind == "pface"]].sum() >= 40
    assert changed_domain[s.rest_bead[s.kind == "dface"]].sum() >= 40
    ref = R.reference(s, r0, box, 7)
    x0 = r0[s.rest_bead] - np.asarray(ref["d"], float)
    k = np.flatnonzero(s.kind == "dface")
    far = (np.sign(x0[k]) != np.sign(r0[s.rest_bead[k]])) & (fc[k] != 0)
    assert far.any(axis=1).all()
    amp = np.abs(np.asarray(ref["d"], float))[fc > 0]
    assert amp.max() <= R.AMPLITUDE_A * R.ANG * (1 + 1e-9)


@pytest.mark.parametrize("no_bead", [False, True])
def test_emptying_leaves_the_first_domain(no_bead):
    from ddcmd_amd.martini import domain_of
    s = R.system("emptying", no_bead)
    owner = domain_of(s, s.grid)
    rb = s.rest_bead
    assert set(np.flatnonzero(owner == 0).tolist()) >= set(s.cluster.tolist()) and (owner[rb] == 0).sum() == len(s.cluster)
    assert ((owner == 0).sum() == len(s.cluster)) == bool(no_bead)
    ref = R.reference(s, R.positions(s), R.box_of(s), 7)
    assert ref["e"][np.isin(rb, s.cluster)].sum() > 0.05 * ref["E"]
    run = R.LDReference(s)
    for n in range(20):
        r, v = run.step()
    sn = copy.copy(s)
    sn.rx, sn.ry, sn.rz = (np.ascontiguousarray(r[:, c]) for c in range(3))
    owner = domain_of(sn, s.grid)
    assert (owner[rb] == 1).all() and ((owner == 0).sum() == 0) == bool(no_bead)
    assert r[s.cluster, 0].min() > 2.0 * R.ANG


def test_lipid_restrains_all_three_bead_kinds():
    s, s0 = R.system("lipid")
    kind = R.bonded_kinds(s)
    cnt = np.bincount(kind[s.rest_bead], minlength=3)
    print("restrained beads without bonded rows / light launch only / heavy launch:", cnt.tolist())
    assert s.nrest > 256 and cnt.min() >= 5 and s0.nrest == 0
    ref = R.reference(s, R.positions(s), R.box_of(s), s.pbc)
    R.assert_guard(s)
    o, o0 = pyoracle.Oracle(s), pyoracle.Oracle(s0)
    e, vir = o.forces()
    e0, vir0 = o0.forces()
    f = np.stack([o.fx - o0.fx, o.fy - o0.fy, o.fz - o0.fz], 1)
    ftot = np.sqrt(o.fx ** 2 + o.fy ** 2 + o.fz ** 2)
    assert (np.abs(f - ref["F"]) <= R.force_bound(s, ref, R.box_of(s)) + 8 * U * ftot[:, None]).all()
    assert abs(e["restraint"] - ref["E"]) <= R.sum_bound(s, ref)[0]


def test_trajectory_tolerance_measured():
    """float64 against longdouble state over the 60 steps of oscillators(), both driven by the reference's forces: a fresh measurement
    stays below the constants of restraint_systems (which the GPU test multiplies by TRAJ_FACTOR = 16)"""
    s = R.system("oscillators")
    dr, dv = R.measure_trajectory_tolerance(s)
    print("largest |r64 - rld| = %.3e A, largest |v64 - vld| = %.3e (largest |v| %.3e)" % (dr / R.ANG, dv, max(np.abs(x).max() for x in (s.vx, s.vy, s.vz))))
    assert 0 < dr <= R.TRAJ_R_MEASURED and 0 < dv <= R.TRAJ_V_MEASURED
    assert dr > 0.1 * R.TRAJ_R_MEASURED and dv > 0.1 * R.TRAJ_V_MEASURED, "the constants are stale: far above what is measured"
    assert R.TRAJ_FACTOR == 16.0

"""Adversarial constraint groups and molecules for k_constrain and the molecular virial (helper module, no tests in here).

The gas of tests/restraint_systems.py (eps = 0, shift = 0, no charges, no bonded terms: every pair term vanishes identically) with
three species of masses 18 : 72 : 360 (1 : 4 : 20), a box of 48 x 56 x 64 A, gids (molecule << 32) | k, beads handed over in a shuffled
order.  The constraint impulse is all that changes a velocity; one NGLFCONSTRAINT step is FRONT solve, drift, BACK solve.

Builders return (Setup, (pair_off, pairI, pairJ, dist)):
  chains(na) na = 2, 3, 17, 18 (18 atoms / 17 pairs: 123 of the 128 LDS items), too_large() the 19-chain (130 items), rings() 18-rings
  (126 items) and rigid tetrahedra K4, mixed(ngroups) 1, 63, 64, 65, 129 groups cycling 2, 18, 3, ring, 2, K4 with pairs shuffled and
  I / J swapped at random, faces(pbc) groups across every periodic face, edge and a corner and -- on open axes -- pairs 0.62 L long
  that must not wrap, slow() nearly collinear 18-chains of alternating heaviest and lightest beads (at least 50 sweeps), stuck() two
  triangles whose dist violate the triangle inequality (500 sweeps) among healthy groups, off_length() lengths off dist by up to 3 %,
  domains(grid) groups across every internal face and the brick corner, some drifting through a face, beyond_halo() a pair 13 A long
  across the internal face of (2, 1, 1).
Molecular virial builders return a Setup whose forces come from the RESTRAINT potential on a subset of every molecule's beads:
  molecules(nmulti) 1, 63, 64, 65, 256, 257, 600; molecules_faces(pbc); molecules_split(grid).

References in numpy.longdouble: solve (nglfconstraint.c:180-264, FRONT and BACK, the caller's pair order, tol, maxit; dtype=float64
is the mirror with the kernel's order of operations), step, molecular_virial (molecularPressure.c:23-56).

Tolerances are measured (tests/test_constraint_systems_host.py re-measures them): *_MEASURED is the largest difference between the
float64 mirror and longdouble, FACTOR = 16 covers the kernel's fused multiply-adds and a different stopping sweep, not method error."""
import copy

import numpy as np

import restraint_systems as R
from ddcmd_amd.deck import Setup, units_convert
from ddcmd_amd.synth import water_forcefield

LD = np.longdouble
ANG = R.ANG
BOX_A = R.BOX_A
U = 2.0 ** -53
TOL, MAXIT = 1.0e-12, 500
MASS_MP = (18.0, 72.0, 360.0)
KT = units_convert(310.0, "K")
GUARD = 0.1                    # every pair vector component on a periodic axis: | |d| / L - 0.5 | >= GUARD
HALO_A = 10.0                  # rmax + deltaR
NSTEPS = 40
CHAIN_SIZES = (2, 3, 17, 18)
MIXED_COUNTS = (1, 63, 64, 65, 129)
PBCS = (7, 3, 5, 6, 0)
GRIDS = ((2, 1, 1), (1, 1, 2), (2, 2, 2))
MOL_COUNTS = (1, 63, 64, 65, 256, 257, 600)
# float64 mirror against longdouble, the largest over every run of the GPU tests (measure(); running this module prints all four); the
# GPU tests allow FACTOR times
VEL_MEASURED = 2.4e-17           # measured 2.34e-17 internal units after one step, off_length() (speeds reach 5e-3)
POS_MEASURED = 9.0e-15 * ANG     # measured 8.97e-15 A after one step, faces(7) under the barostat (5.50e-15 without it)
TRAJ_R_MEASURED = 9.2e-14 * ANG  # measured 9.12e-14 A after 40 steps (faces(7) under the barostat; 7.5e-14 without it)
TRAJ_V_MEASURED = 3.0e-16        # measured 2.96e-16 after 40 steps (faces(7) under the barostat; 7.0e-17 without it)
FACTOR = 16.0
# after a solve: the last sweep saw every |rvab dt| < tol.  A pair solved early in that sweep is perturbed afterwards by every later pair
# that shares an atom with it, by at most that pair's own correction, < tol each: two such pairs in a chain or ring, four in K4.  The
# BACK residual |rab . vab| dt / d^2 IS |rvab dt|: (1 + 4) tol.  The FRONT residual |r|^2 / d^2 - 1 is 2 rvab dt: 2 (1 + 4) tol, and the
# BACK solve moves no position
VEL_MULT = 5.0
LEN_MULT = 10.0


def box_of(s):
    return np.array([s.h[0], s.h[4], s.h[8]])


def positions(s):
    return np.stack([np.asarray(s.rx, float), np.asarray(s.ry, float), np.asarray(s.rz, float)], 1)


def velocities(s):
    return np.stack([np.asarray(s.vx, float), np.asarray(s.vy, float), np.asarray(s.vz, float)], 1)


def masses(s):
    return np.asarray(s.mass, float)[np.asarray(s.species)]


def _forcefield(s, update_rate=10):
    water_forcefield(s, 8.0, 2.0, 20.0, update_rate)
    s.eps = np.zeros_like(s.eps)
    s.shift = np.zeros_like(s.shift)
    s.nspecies = 3
    s.species_name = ["LxL", "MxM", "HxH"]
    s.mass = np.array(MASS_MP) * units_convert(1.0, "M_p")
    s.charge = np.zeros(3)
    s.ljtype = np.array([1, 0, 1], np.int32)
    s.moltype = np.array([0, 1, 2], np.int32)
    s.resitype = np.array([0, 1, 2], np.int32)
    s.atomoffset = np.zeros(3, np.int32)
    s.nmoltype = 3
    s.mol_nspecies = np.ones(3, np.int32)
    s.bpair_off = np.zeros(4, np.int32)
    s.nresi = 3
    s.resi_natoms = np.ones(3, np.int32)
    s.bond_off = np.zeros(4, np.int32)
    s.angle_off = np.zeros(4, np.int32)
    s.tors_off = np.zeros(4, np.int32)
    s.h = np.array([BOX_A[0], 0, 0, 0, BOX_A[1], 0, 0, 0, BOX_A[2]]) * ANG
    s.pbc = 7
    return s


# -- group geometries (A, about their centre) -----------------------------------------------------------------------------------
def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _chain(na):
    k = np.arange(na)
    p = np.stack([1.5 * np.cos(k * np.pi / 3), 1.5 * np.sin(k * np.pi / 3), 0.3 * k], 1)
    return p - p.mean(axis=0), [(a, a + 1) for a in range(na - 1)]


def _ring():
    k = np.arange(18)
    p = np.stack([2.5 * np.cos(2 * np.pi * k / 18), 2.5 * np.sin(2 * np.pi * k / 18), 0.4 * (-1.0) ** k], 1)
    return p, [(a, (a + 1) % 18) for a in range(18)]


def _k4():
    p = 3.0 / np.sqrt(8.0) * np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    return p, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _line(na=18):
    p = np.zeros((na, 3))
    p[:, 0] = 1.5 * (np.arange(na) - 0.5 * (na - 1))
    return p, [(a, a + 1) for a in range(na - 1)]


def _long(a):
    """a pair 0.62 L long along axis a (an open axis: it must not wrap)"""
    p = np.full((2, 3), 0.4)
    p[1] = -0.4
    p[0, a], p[1, a] = -0.31 * BOX_A[a], 0.31 * BOX_A[a]
    return p, [(0, 1)]


def _tri():
    """nearly collinear: sides 1.5008, 1.5008, 3 A (stuck() asks for 1.5, 1.5, 3.01)"""
    return np.array([[-1.5, 0, 0], [0.0, 0.05, 0], [1.5, 0, 0]]), [(0, 1), (1, 2), (0, 2)]


def _far():
    """a pair 13 A long along x, not rotated (beyond_halo)"""
    return np.array([[-1.0, 0, 0], [12.0, 0, 0]]), [(0, 1)]


KINDS = {"tri": _tri, "longfar": _far, "long0": lambda: _long(0), "long1": lambda: _long(1), "long2": lambda: _long(2), "c2": lambda: _chain(2), "c3": lambda: _chain(3), "c17": lambda: _chain(17), "c18": lambda: _chain(18), "c19": lambda: _chain(19),
         "ring": _ring, "k4": _k4, "line": _line}
CYCLE = ("c2", "c18", "c3", "ring", "c2", "k4")


def _centres(n, rng, margin=0.0):
    """n jittered sites of a 6 x 6 x 4 lattice of the box, `margin` A away from the faces"""
    assert n <= 144
    L = np.array(BOX_A) - 2.0 * margin
    k = rng.permutation(144)[:n]
    ijk = np.stack([k % 6, (k // 6) % 6, k // 36], 1)
    return -0.5 * L + (ijk + 0.5) * L / np.array([6, 6, 4]) + rng.uniform(-0.5, 0.5, (n, 3))


def assemble(name, kinds, centres, seed, pbc=7, shuffle_pairs=False, nfree=300, vscale=0.15, drift=None, stretch=None, species=None,
             dist_override=None, jitter=None, update_rate=10, free_margin=0.0):
    """place one group of kinds[g] at centres[g] (A), randomly rotated, add nfree single beads, shuffle the beads.  Returns
    (Setup, tables); the Setup carries groups (bead indices per group, in group-local order of the builder), kinds, tables."""
    rng = np.random.RandomState(seed)
    s = _forcefield(Setup(), update_rate)
    s.pbc = int(pbc)
    L = np.array(BOX_A)
    per = np.array([(int(pbc) >> a) & 1 for a in range(3)], bool)
    pos, spec, vel, mol, kk, groups, pI, pJ, dd, off = [], [], [], [], [], [], [], [], [], [0]
    n = 0
    for g, kind in enumerate(kinds):
        p, pairs = KINDS[kind]()
        if kind == "line":
            p = p[:, [(g + c) % 3 for c in range(3)]]
        elif not kind.startswith("long"):
            p = p @ _rotation(rng).T
        if jitter:
            p = p + rng.uniform(-jitter, jitter, p.shape)
        p_un = p
        if stretch is not None:
            p = p * (1.0 + stretch[g])
        na = len(p)
        sp = np.array([(a + g) % 3 for a in range(na)]) if species is None or species[g] is None else np.asarray(species[g])
        m = np.array(MASS_MP)[sp] * units_convert(1.0, "M_p")
        v = rng.normal(size=(na, 3)) * np.sqrt(KT / m)[:, None] * vscale
        if drift is not None and drift[g] is not None:
            v = v + np.asarray(drift[g]) * ANG / s.dt
        pairs = list(pairs)
        if shuffle_pairs:
            pairs = [pairs[q] for q in rng.permutation(len(pairs))]
            pairs = [(b, a) if rng.uniform() < 0.5 else (a, b) for a, b in pairs]
        for a, b in pairs:
            pI.append(n + a); pJ.append(n + b)
        d0 = np.array([np.sqrt(((p_un[a] - p_un[b]) ** 2).sum()) for a, b in pairs])
        if dist_override and g in dist_override:
            d0 = np.array(dist_override[g], float)
        dd.extend(d0.tolist())
        off.append(off[-1] + len(pairs))
        pos.append(p + np.asarray(centres[g])); spec.append(sp); vel.append(v)
        mol.extend([g] * na); kk.extend(range(na))
        groups.append(np.arange(n, n + na))
        n += na
    ng = len(kinds)
    fr = R._lattice(rng, nfree) if nfree else np.zeros((0, 3))
    if free_margin:
        fr = fr * (1.0 - 2.0 * free_margin / L)
    fsp = np.arange(nfree) % 3
    fm = np.array(MASS_MP)[fsp] * units_convert(1.0, "M_p")
    pos.append(fr); spec.append(fsp); vel.append(rng.normal(size=(nfree, 3)) * np.sqrt(KT / fm)[:, None] * vscale)
    mol.extend(range(ng, ng + nfree)); kk.extend([0] * nfree)
    r = np.concatenate(pos)
    r = np.where(per, r - L * np.rint(r / L), r)
    assert (np.abs(r) <= 0.5 * L + 1e-9).all(), "a bead outside the box on an open axis"
    ntot = len(r)
    perm = rng.permutation(ntot)               # new index of old bead i is where[i]
    where = np.empty(ntot, int)
    where[perm] = np.arange(ntot)
    molnum = rng.permutation(ng + nfree)       # molecule numbers are not in order either
    s.natoms = ntot
    rr, vv = r[perm] * ANG, np.concatenate(vel)[perm]
    s.rx, s.ry, s.rz = (np.ascontiguousarray(rr[:, c]) for c in range(3))
    s.vx, s.vy, s.vz = (np.ascontiguousarray(vv[:, c]) for c in range(3))
    s.species = np.concatenate(spec)[perm].astype(np.int32)
    s.group = np.zeros(ntot, np.int32)
    s.gid = ((molnum[np.array(mol)].astype(np.uint64) << np.uint64(32)) | np.array(kk, np.uint64))[perm]
    tables = (np.array(off, np.int32), where[np.array(pI, int)].astype(np.int32), where[np.array(pJ, int)].astype(np.int32), np.array(dd) * ANG)
    s.groups = [where[g] for g in groups]
    s.kinds = list(kinds)
    s.tables = tables
    s.name = name
    assert_guard(s, tables)
    return s, tables


def assert_guard(s, tables, r=None):
    """every pair vector component on a periodic axis stays GUARD away from half the box side in |d| / L"""
    r = positions(s) if r is None else np.asarray(r, float)
    _, I, J, _ = tables
    t = np.abs((r[I] - r[J]) / box_of(s))
    t = np.abs(t - np.floor(t) - 0.5)
    per = np.array([(int(s.pbc) >> a) & 1 for a in range(3)], bool)
    if len(I) and per.any():
        assert (t[:, per] >= GUARD).all(), ("a pair vector near half the box", float(t[:, per].min()))


def lds_items(tables):
    """4 atoms + 3 pairs of the largest group (the solver's LDS budget is 128)"""
    off, I, J, _ = tables
    na = max(len(set(I[off[g]:off[g + 1]].tolist()) | set(J[off[g]:off[g + 1]].tolist())) for g in range(len(off) - 1))
    return 4 * na + 3 * int(np.diff(off).max())


def chains(na, seed=100):
    rng = np.random.RandomState(seed + na)
    return assemble("chains%d" % na, ["c%d" % na] * 40, _centres(40, rng), seed + na)


def too_large(seed=119):
    rng = np.random.RandomState(seed)
    return assemble("too_large", ["c2", "c19", "c3"], _centres(3, rng), seed, nfree=60)


def rings(seed=120):
    rng = np.random.RandomState(seed)
    return assemble("rings", ["ring", "k4"] * 20, _centres(40, rng), seed)


def mixed(ngroups, seed=200):
    rng = np.random.RandomState(seed + ngroups)
    return assemble("mixed%d" % ngroups, [CYCLE[g % 6] for g in range(ngroups)], _centres(ngroups, rng), seed + ngroups, shuffle_pairs=True)


def _face_centres(planes, rng, corner=True, lo=-0.3, hi=0.3):
    """centres on every plane (axis, coordinate), on every line where two planes of different axes meet and on one point where three
    do; the free coordinates 12 A inside"""
    L = np.array(BOX_A)
    out = []

    def free():
        return rng.uniform(-0.5, 0.5, 3) * (L - 24.0)
    for a, x in planes:
        c = free(); c[a] = x + rng.uniform(lo, hi); out.append(c)
    for i, (a, x) in enumerate(planes):
        for b, y in planes[i + 1:]:
            if a != b:
                c = free(); c[a] = x + rng.uniform(lo, hi); c[b] = y + rng.uniform(lo, hi); out.append(c)
    if corner:
        axes = sorted(set(a for a, _ in planes))
        if len(axes) == 3:
            c = np.array([[x for a, x in planes if a == ax][-1] for ax in range(3)], float) + rng.uniform(lo, hi, 3)
            out.append(c)
    return out


def faces(pbc, seed=300):
    rng = np.random.RandomState(seed + pbc)
    L = np.array(BOX_A)
    per = [a for a in range(3) if (pbc >> a) & 1]
    planes = [(a, sgn * 0.5 * L[a]) for a in per for sgn in (-1.0, 1.0)]
    cen = _face_centres(planes, rng)
    kinds = [CYCLE[(g + 1) % 6] for g in range(len(cen))]
    for a in range(3):
        if a not in per:
            for rep in range(2):
                c = rng.uniform(-0.25, 0.25, 3) * L
                c[a] = 0.0
                cen.append(c); kinds.append("long%d" % a)
    for extra in range(6):
        cen.append(rng.uniform(-0.5, 0.5, 3) * (L - 24.0)); kinds.append(CYCLE[extra])
    return assemble("faces_pbc%d" % pbc, kinds, cen, seed + pbc, pbc=pbc, shuffle_pairs=True, free_margin=0.0 if pbc == 7 else 4.0)


def slow(seed=400):
    rng = np.random.RandomState(seed)
    kinds = ["line"] * 3 + ["c3", "k4", "c2"]
    sp = [np.array([2, 0] * 9)] * 3 + [None] * 3
    cen = [np.array([0.0, -15, -20]), np.array([-12.0, 0, 10]), np.array([14.0, 12, 0])] + list(_centres(3, rng))
    s, t = assemble("slow", kinds, cen, seed, species=sp, jitter=0.4, nfree=100)
    _, sw, _ = solve(positions(s), velocities(s), 1.0 / masses(s), t, s.dt, box_of(s), s.pbc, True)
    assert sw[:3].min() >= 50, sw
    return s, t


def stuck(seed=410):
    rng = np.random.RandomState(seed)
    kinds = ["c3", "tri", "c18", "k4", "tri", "ring", "c2"]
    over = {1: [1.5, 1.5, 3.01], 4: [1.5, 1.5, 3.01]}      # 3.01 > 1.5 + 1.5
    s, t = assemble("stuck", kinds, _centres(7, rng), seed, dist_override=over, nfree=100)
    s.stuck_groups = (1, 4)
    v, sw, bad = solve(positions(s), velocities(s), 1.0 / masses(s), t, s.dt, box_of(s), s.pbc, True)
    assert np.flatnonzero(bad).tolist() == [1, 4] and (sw[[1, 4]] == MAXIT).all() and np.isfinite(v.astype(float)).all(), (sw, bad)
    # (the BACK solve of the same step does not converge on them either: the FRONT sweeps leave the triangles all but collinear, where
    # the three conditions rab . vab = 0 are nearly dependent; the device counts a group once per solve: 4 after one step)
    return s, t


def off_length(seed=420):
    rng = np.random.RandomState(seed)
    kinds = [CYCLE[g % 6] for g in range(24)]
    stretch = rng.uniform(-0.03, 0.03, 24)
    stretch[:4] = (0.03, -0.03, 0.03, -0.03)
    return assemble("off_length", kinds, _centres(24, rng), seed, stretch=stretch, shuffle_pairs=True)


def domains(grid, seed=500):
    rng = np.random.RandomState(seed + sum(g * 10 ** k for k, g in enumerate(grid)))
    L = np.array(BOX_A)
    planes = [(a, 0.0) for a in range(3) if grid[a] == 2] + [(a, 0.5 * L[a]) for a in range(3) if grid[a] == 2]
    cen = _face_centres([(a, x) for a, x in planes if x == 0.0], rng) + _face_centres(planes[len(planes) // 2:], rng, corner=False)
    cen.append(rng.uniform(-0.2, 0.2, 3))            # the corner where the bricks meet (a point of the internal faces on every grid)
    corner = len(cen) - 1
    kinds = [CYCLE[(g + 3) % 6] for g in range(len(cen))]
    kinds[corner] = "ring"
    drift = [None] * len(cen)
    for a, x in planes:                              # groups that swing through a face: 1.2 A away, 0.07 A per step towards it
        for sgn in (-1.0, 1.0):
            c = rng.uniform(-0.5, 0.5, 3) * (L - 24.0)
            c[a] = x + sgn * 4.0
            d = np.zeros(3)
            d[a] = -sgn * 0.07
            cen.append(c); kinds.append(("c18", "ring", "c3", "k4")[len(cen) % 4]); drift.append(d)
    for extra in range(6):
        cen.append(rng.uniform(-0.5, 0.5, 3) * (L - 24.0)); kinds.append(CYCLE[extra]); drift.append(None)
    s, t = assemble("domains_%dx%dx%d" % tuple(grid), kinds, cen, seed, shuffle_pairs=True, drift=drift)
    s.grid, s.corner_group = tuple(grid), corner
    return s, t


def beyond_halo(seed=510):
    """(2, 1, 1): one pair 13 A long across x = 0, its far atom further than rmax + deltaR = 10 A from the face"""
    rng = np.random.RandomState(seed)
    s, t = assemble("beyond_halo", ["c3", "longfar"], [np.array([-10.0, 5, 5]), np.array([0.0, -6, 3])], seed, nfree=100)
    s.grid = (2, 1, 1)
    return s, t


# -- the solver ------------------------------------------------------------------------------------------------------------------
def _wrap(d, L, per):
    """bioVec: x += L * -rint((1 / L) * x) on the periodic axes, in the array's own type"""
    Linv = d.dtype.type(1) / L
    return np.where(per, d + L * -np.rint(Linv * d), d)


def solve(r, v, rm, tables, dt, box, pbc, front, tol=TOL, maxit=MAXIT, dtype=LD):
    """resMoveConsOld (nglfconstraint.c:180-264) on every group: Gauss-Seidel sweeps over the pairs in the caller's order,
    rvab = FRONT ((rab + dt vab)^2 - d^2) / (2 dt) / d^2 | BACK (rab . vab) / d^2, gab = -rvab / (1 / ma + 1 / mb), va += gab / ma rab,
    vb -= gab / mb rab, until max |rvab dt| < tol or maxit sweeps.  Returns (velocities, sweeps per group, groups that hit maxit without
    converging).  dtype float64 carries every operation in the kernel's order (no fused multiply-add)."""
    off, I, J, dist = tables
    T = dtype
    r, v, rm = np.asarray(r, T), np.array(v, T), np.asarray(rm, T)
    dt, L, tol = T(dt), np.asarray(box, T), T(tol)
    per = np.array([(int(pbc) >> a) & 1 for a in range(3)], bool)
    G = len(off) - 1
    npg = np.diff(off)
    maxP = int(npg.max())
    col = np.arange(maxP)
    valid = col[None, :] < npg[:, None]
    idx = np.where(valid, off[:-1, None] + col[None, :], 0)
    A, B = np.asarray(I)[idx], np.asarray(J)[idx]
    rab = _wrap(r[A] - r[B], L, per)
    dd = np.asarray(dist, T)[idx]
    d2 = dd * dd
    sweeps = np.zeros(G, int)
    active = np.arange(G)
    two_dt = 2 * dt

    def plan(active):
        """per pair position: what the sweep needs of the groups still active (gathered once per change of the active set)"""
        out = []
        for ab in range(maxP):
            m = np.flatnonzero(valid[active, ab])
            if not m.size:
                break
            g = active[m]
            a, b = A[g, ab], B[g, ab]
            out.append((m, a, b, rab[g, ab], d2[g, ab], rm[a] + rm[b], rm[a][:, None], rm[b][:, None]))
        return out
    todo = plan(active)
    for it in range(maxit):
        err = np.zeros(len(active), T)
        for m, a, b, x, dd2, rms, rma, rmb in todo:
            w = v[a] - v[b]
            if front:
                p = x + dt * w
                q = p * p
                rvab = (q[:, 0] + q[:, 1] + q[:, 2] - dd2) / two_dt
            else:
                q = x * w
                rvab = q[:, 0] + q[:, 1] + q[:, 2]
            rvab = rvab / dd2
            gab = (-rvab / rms)[:, None]
            err[m] = np.maximum(err[m], np.abs(rvab * dt))
            v[a] += (rma * gab) * x
            v[b] -= (rmb * gab) * x
        sweeps[active] = it + 1
        keep = ~(err < tol)
        if not keep.all():
            active = active[keep]
            if not len(active):
                break
            todo = plan(active)
    bad = np.zeros(G, bool)
    bad[active] = True
    return v, sweeps, bad


def barostat_scale(s, box, dt, dtype=LD):
    """changeVolume on the force-free gas: the virial and the molecular term are zero, p = N kT / V - P0 on every axis"""
    T = dtype
    nmol = len(np.unique(np.asarray(s.gid, np.uint64) >> np.uint64(32)))
    vol = box[0] * box[1] * box[2]
    p = T(nmol) * T(s.npt_T) / vol - T(s.npt_P0)
    lam = np.cbrt(T(1) + p * (T(s.npt_beta) * T(dt) / T(s.npt_tau)))
    return np.array([lam, lam, lam], T)


def step(s, tables, nsteps=1, dts=None, dtype=LD, barostat=False, state=None):
    """NGLFCONSTRAINT steps of the force-free gas: (barostat scaling,) FRONT solve, drift, BACK solve.  dts: one dt per step.  Returns
    (r, v, box, largest sweep count, groups that did not converge in some solve, the number of solves of a group that did not converge
    -- what the device counts); state = (r, v, box) continues a run"""
    T = dtype
    if state is None:
        r, v, box = positions(s).astype(T), velocities(s).astype(T), box_of(s).astype(T)
    else:
        r, v, box = (np.array(x, T) for x in state)
    rm = (T(1) / np.asarray(s.mass, T))[np.asarray(s.species)]
    dts = [s.dt] * nsteps if dts is None else dts
    most, bad, nbad = 0, np.zeros(len(tables[0]) - 1, bool), 0
    for dt in dts:
        if barostat:
            lam = barostat_scale(s, box, dt, T)
            r, box = r * lam, box * lam
        v, sw, b1 = solve(r, v, rm, tables, dt, box, s.pbc, True, dtype=T)
        r = r + T(dt) * v
        v, sw2, b2 = solve(r, v, rm, tables, dt, box, s.pbc, False, dtype=T)
        most, bad, nbad = max(most, int(sw.max()), int(sw2.max())), bad | b1 | b2, nbad + int(b1.sum()) + int(b2.sum())
    return r, v, box, most, bad, nbad


def min_image(d, box, pbc=7):
    per = np.array([(int(pbc) >> a) & 1 for a in range(3)], bool)
    return np.where(per, d - box * np.rint(d / box), d)


def measure(s, tables, nsteps, dts=None, barostat=False, skip=()):
    """largest (|r64 - rld|, |v64 - vld|) after the run, over the beads outside the groups `skip`"""
    ra, va, ba = step(s, tables, nsteps, dts, np.float64, barostat)[:3]
    rb, vb, bb = step(s, tables, nsteps, dts, LD, barostat)[:3]
    keep = np.ones(s.natoms, bool)
    for g in skip:
        keep[s.groups[g]] = False
    dr = np.abs(min_image((ra - rb).astype(float), np.asarray(bb, float), s.pbc))[keep].max()
    return float(dr), float(np.abs(va - vb)[keep].max())


def pair_residuals(r, v, tables, dt, box, pbc):
    """(| |rab|^2 / d^2 - 1 |, |rab . vab| dt / d^2) per pair, longdouble"""
    _, I, J, dist = tables
    per = np.array([(int(pbc) >> a) & 1 for a in range(3)], bool)
    x = _wrap(np.asarray(r, LD)[I] - np.asarray(r, LD)[J], np.asarray(box, LD), per)
    w = np.asarray(v, LD)[I] - np.asarray(v, LD)[J]
    d2 = np.asarray(dist, LD) ** 2
    return np.abs((x * x).sum(axis=1) / d2 - 1), np.abs((x * w).sum(axis=1)) * LD(dt) / d2


def group_momenta(s, v):
    m = masses(s).astype(LD)
    return np.array([(m[g, None] * np.asarray(v, LD)[g]).sum(axis=0) for g in s.groups])


def with_barostat(s, beta_scale=1.0):
    """NGLFCONSTRAINT's barostat at 310 K, P0 = 1 bar; beta so large that the ideal-gas pressure of the gas moves the box by about 1e-3
    per step (beta_scale = 1)"""
    s = copy.copy(s)
    s.npt_T, s.npt_P0, s.npt_tau = KT, units_convert(1.0, "bar"), units_convert(1.0, "ps")
    nmol = len(np.unique(np.asarray(s.gid, np.uint64) >> np.uint64(32)))
    p = nmol * KT / np.prod(box_of(s)) - s.npt_P0
    s.npt_beta = beta_scale * 3.0e-3 * s.npt_tau / (s.dt * p)
    return s


def traj_dts(s, key):
    """mixed(65) halves dt after 20 steps"""
    return [s.dt] * 20 + [0.5 * s.dt] * 20 if key == ("mixed", 65) else [s.dt] * NSTEPS


_runs = {}


def reference_run(key, nsteps, barostat=False):
    """step() of the named system in longdouble, computed once per process and shared by the tests that need it"""
    k = (key, nsteps, barostat)
    if k not in _runs:
        s, t = system(*key)
        s = with_barostat(s) if barostat else s
        _runs[k] = step(s, t, nsteps, dts=traj_dts(s, key) if nsteps == NSTEPS else None, barostat=barostat)
    return _runs[k]


CONSTRAINT_SETS = ([("chains", n) for n in CHAIN_SIZES] + [("rings",)] + [("mixed", n) for n in MIXED_COUNTS] + [("faces", p) for p in PBCS] +
                   [("slow",), ("stuck",), ("off_length",)] + [("domains", g) for g in GRIDS])


# -- molecules -------------------------------------------------------------------------------------------------------------------
def _blob(n, rng):
    rad = min(8.0, 1.5 * n ** (1.0 / 3.0))
    p = rng.normal(size=(n, 3))
    p *= (rad * rng.uniform(0.2, 1.0, n) ** (1.0 / 3.0) / np.sqrt((p * p).sum(axis=1)))[:, None]
    return p


def _molecule_setup(name, sizes, centres, seed, pbc=7, nsingle=None):
    """multi-bead molecules of the given sizes as blobs about the centres, interleaved with single beads; the RESTRAINT potential on about
    half of every molecule's beads (never all, never none) and on no single bead"""
    rng = np.random.RandomState(seed)
    s = _forcefield(Setup())
    s.pbc = int(pbc)
    L = np.array(BOX_A)
    per = np.array([(int(pbc) >> a) & 1 for a in range(3)], bool)
    nm = len(sizes)
    nsingle = max(20, nm // 4) if nsingle is None else nsingle
    pos, mol, kk, rest = [], [], [], []
    n = 0
    for m, (na, c) in enumerate(zip(sizes, centres)):
        pos.append(_blob(na, rng) + c)
        mol.extend([2 * m] * na); kk.extend(rng.permutation(na).tolist())        # the first listed atom (k = 0) is anywhere
        pick = rng.permutation(na)[:max(1, min(na - 1, na // 2))]
        rest.extend((n + pick).tolist())
        n += na
    fr = R._lattice(rng, nsingle) * (1.0 - 8.0 / L)
    pos.append(fr); mol.extend([2 * k + 1 for k in range(nsingle)]); kk.extend([0] * nsingle)
    r = np.concatenate(pos)
    r = np.where(per, r - L * np.rint(r / L), r)
    assert (np.abs(r) <= 0.5 * L + 1e-9).all()
    ntot = len(r)
    perm = rng.permutation(ntot)
    where = np.empty(ntot, int)
    where[perm] = np.arange(ntot)
    s.natoms = ntot
    rr = r[perm] * ANG
    s.rx, s.ry, s.rz = (np.ascontiguousarray(rr[:, c]) for c in range(3))
    s.vx, s.vy, s.vz = (np.zeros(ntot) for _ in range(3))
    s.species = (rng.randint(0, 3, ntot)).astype(np.int32)
    s.group = np.zeros(ntot, np.int32)
    s.gid = ((np.array(mol, np.uint64) << np.uint64(32)) | np.array(kk, np.uint64))[perm]
    bead = where[np.array(rest, int)]
    bead = bead[rng.permutation(len(bead))]
    disp = rng.uniform(1.0, 5.0, (len(bead), 3)) * rng.choice([-1.0, 1.0], (len(bead), 3))
    R._set_restraints(s, bead, np.ones((len(bead), 3), int), r[perm][bead] - disp, rng.uniform(50.0, 500.0, len(bead)))
    s.npt_T, s.npt_P0, s.npt_tau, s.npt_beta = KT, units_convert(1.0, "bar"), units_convert(1.0, "ps"), units_convert(3.0e-10, "1/bar")
    s.name = name
    s.mols = molecule_table(s)
    assert_molecules(s)
    return s


def molecule_table(s):
    """the multi-bead molecules as lists of bead indices in ascending gid (the order of ddcmd_amd.martini.molecule_lists)"""
    from ddcmd_amd.martini import molecule_lists
    _, off, atoms = molecule_lists(s)
    return [atoms[off[m]:off[m + 1]].astype(int) for m in range(len(off) - 1)]


def assert_molecules(s):
    """every extent below 0.45 of the shortest periodic side; a net force of at least 0.1 max |f| on at least 90 % of the molecules"""
    r, box = positions(s), box_of(s)
    per = np.array([(int(s.pbc) >> a) & 1 for a in range(3)], bool)
    f = R.reference(s, r, box, s.pbc)["F"].astype(float)
    short = box[per].min() if per.any() else box.min()
    ok = 0
    for idx in s.mols:
        x = min_image(r[idx] - r[idx[0]], box, s.pbc)
        ext = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)).max()
        assert ext < 0.45 * short, (ext / ANG, short / ANG)
        fm = np.sqrt((f[idx] ** 2).sum(axis=1)).max()
        ok += np.sqrt((f[idx].sum(axis=0) ** 2).sum()) >= 0.1 * fm
    assert ok >= 0.9 * len(s.mols), (ok, len(s.mols))


def _sizes(nmulti):
    return [300 if m == 0 else 17 if m % 100 == 7 else 64 if m == 33 else 3 if m % 10 == 2 else 5 if m % 10 == 5 else 2 for m in range(nmulti)]


def molecules(nmulti, seed=600):
    rng = np.random.RandomState(seed + nmulti)
    L = np.array(BOX_A)
    return _molecule_setup("molecules%d" % nmulti, _sizes(nmulti), rng.uniform(-0.5, 0.5, (nmulti, 3)) * L, seed + nmulti)


def molecules_faces(pbc, seed=700):
    rng = np.random.RandomState(seed + pbc)
    L = np.array(BOX_A)
    planes = [(a, sgn * 0.5 * L[a]) for a in range(3) if (pbc >> a) & 1 for sgn in (-1.0, 1.0)]
    cen = _face_centres(planes, rng) + [rng.uniform(-0.5, 0.5, 3) * (L - 24.0) for _ in range(6)]
    sizes = [(2, 40, 5, 17, 3)[m % 5] for m in range(len(cen))]
    return _molecule_setup("molecules_faces%d" % pbc, sizes, cen, seed + pbc, pbc=pbc)


def owners(s, grid):
    """per multi-bead molecule: the ranks that own one of its beads"""
    from ddcmd_amd.martini import domain_of
    own = domain_of(s, grid)
    return [sorted(set(own[idx].tolist())) for idx in s.mols], own


def molecules_split(grid, seed=800):
    rng = np.random.RandomState(seed + sum(g * 10 ** k for k, g in enumerate(grid)))
    L = np.array(BOX_A)
    planes = [(a, 0.0) for a in range(3) if grid[a] == 2]
    cen = sum((_face_centres(planes, rng, lo=-0.2, hi=0.2) for _ in range(3)), []) + [rng.uniform(-0.5, 0.5, 3) * (L - 24.0) + 0 for _ in range(10)]
    sizes = [(24, 9, 40)[m % 3] for m in range(len(cen))]      # (at most 500 beads within a list radius of the bricks' corner)
    s = _molecule_setup("molecules_split_%dx%dx%d" % tuple(grid), sizes, cen, seed, nsingle=40)
    s.grid = tuple(grid)
    own, per_bead = owners(s, grid)
    counts = sorted(set(len(o) for o in own))
    want = {1: [1], 2: [1, 2], 8: [1, 2, 4, 8]}[int(np.prod(grid))]
    assert set(want) <= set(counts), (counts, want)
    s.nsplit = sum(len(o) > 1 for o in own)
    assert any(len(o) > 1 and per_bead[idx[0]] != o[0] for o, idx in zip(own, s.mols)), "no split molecule whose first listed atom is off the lowest rank"
    return s


def molecular_virial(s, r, f, box, skip_pf=()):
    """molecularPressure.c:23-56 in longdouble: the diagonal of sum (r - R) f over the beads of every multi-bead molecule, R the centre
    of mass, images about the first listed atom.  Returns (diag[3], sum of |terms|[3], number of terms); skip_pf: molecules whose
    (P / M) o F is left out (what a run that loses the split term would compute)"""
    r, f, L = np.asarray(r, LD), np.asarray(f, LD), np.asarray(box, LD)
    m = np.asarray(s.mass, LD)[np.asarray(s.species)]
    per = np.array([(int(s.pbc) >> a) & 1 for a in range(3)], bool)
    out, mag, nterm = np.zeros(3, LD), np.zeros(3, LD), 0
    for k, idx in enumerate(s.mols):
        x = r[idx] - r[idx[0]]
        x = np.where(per, x - L * np.rint(x / L), x)
        Rc = (m[idx, None] * x).sum(axis=0) / m[idx].sum()
        if k in skip_pf:
            out += (x * f[idx]).sum(axis=0)
        else:
            out += ((x - Rc) * f[idx]).sum(axis=0)
        mag = np.maximum(mag, ((np.abs(x) + np.abs(Rc)) * np.abs(f[idx])).max(axis=0))
        nterm += len(idx)
    return out, mag, nterm


def pressure_bound(s, r, f, box, vir_diag, nkt):
    """bound on | (pmol V - N kT) - (vir - molv) | per component: the roundings of the sums that enter it -- (number of terms) x (largest
    magnitude of a term) x 2^-53 for vir (nrest terms f_a d_a of the restraint virial, the largest bounded by max |f_a| max |d_a|
    <= max |f_a| * 5 A * sqrt(3)) and for molv (one term (|x| + |R|) |f| per bead of a multi-bead molecule, |R| for the roundings of
    the centre of mass that multiply the net force, twice: the sum is taken in two passes) -- plus four roundings of the result's
    own arithmetic at the size of what cancels: the device divides (vir - molv + N kT) by V, the test multiplies by V and subtracts N kT"""
    _, mag, nterm = molecular_virial(s, r, f, box)
    fmax = np.abs(np.asarray(f, LD)).max(axis=0)
    vir_term = fmax * LD(5.0 * np.sqrt(3.0)) * LD(ANG)
    return (int(s.nrest) * vir_term + 2 * nterm * mag) * LD(U) + 4 * LD(U) * (abs(LD(nkt)) + np.abs(np.asarray(vir_diag, LD)) + nterm * mag)


_made = {}


def system(name, *args):
    """the named builder's result, made once and left unchanged"""
    key = (name,) + args
    if key not in _made:
        _made[key] = globals()[name](*args)
    return _made[key]


TRAJ_SETS = CONSTRAINT_SETS          # every builder runs 40 steps on the device


if __name__ == "__main__":      # the measurement behind the *_MEASURED constants, in one place
    w = [0.0, 0.0, 0.0, 0.0]
    for key, baro in [(k, False) for k in CONSTRAINT_SETS] + [(("faces", 7), True), (("domains", (2, 1, 1)), True)]:
        s, t = system(*key)
        s = with_barostat(s) if baro else s
        skip = getattr(s, "stuck_groups", ())
        dr, dv = measure(s, t, 1, barostat=baro, skip=skip)
        w[0], w[1] = max(w[0], dr / ANG), max(w[1], dv)
        dr, dv = measure(s, t, NSTEPS, dts=traj_dts(s, key), barostat=baro, skip=skip)
        w[2], w[3] = max(w[2], dr / ANG), max(w[3], dv)
        print(key, baro, "%.3e %.3e" % (dr / ANG, dv), flush=True)
    print("POS %.3e A  VEL %.3e  TRAJ_R %.3e A  TRAJ_V %.3e" % tuple(w))

"""Adversarial systems for bead ownership and migration between bricks (helper module, no tests in here).

k_mig_classify decides at every rebuild which brick owns a bead -- wrap on the periodic axes, b = floor((r + L/2) / (L/P)) clamped to
[0, P - 1], dd = b - (own brick), folded by -+P on a periodic axis -- and packs the beads that leave into one of 26 direction segments;
k_compact_order / k_gather_state close the gaps, k_unpack_mig appends the arrivals.  Thermal motion never puts a bead within an ulp of
a face, through a corner, through a brick face and a periodic face at once, or two bricks away.  These builders do, on the gas of
tests/restraint_systems.py whose pair terms vanish identically: a bead's trajectory is x = fma(dt, v, x) step after step and depends on
no neighbour, so one domain and any decomposition must agree bit for bit, and any speed is legal.

Box 96 x 56.6 x 64 A at rcut 8 A + skin 2 A: every brick of every grid of GRIDS is at least one list radius (10 A) wide; in internal
units no side, no L / P and no face k L / P - L / 2 (other than 0) is a binary fraction.

  * `crossers(grid, pbc)`: for every brick and every one of the 26 directions that leads to another brick, 8 beads 0.25 ... 0.9 A inside
    the brick with a velocity that carries them through that face, edge or corner in the first rebuild period, and 4 that follow in the
    second.  On a periodic axis the outer faces of the grid are brick faces too: there the crossing coincides with the wrap.
    (The gas has no force that could turn a bead round: the way back through a face is the neighbour's planted set for the opposite
    direction; beads that cross and come back are `returners()`.)
  * `face_sitters(grid, pbc)`: beads at rest and slow beads (1e-3 A per step) at face + k u, k in -2 ... 2, u = the spacing of doubles at
    L / 2, on every face plane between two bricks (the outer faces -L/2 and +L/2 of a divided periodic axis among them: there the wrap's
    strict comparisons and the clamp of b to P - 1 decide), on the edge lines and at the corner where faces of two and three axes meet;
    on an open axis beads up to 0.45 L outside the box, which the edge brick keeps.
  * `two_hops(grid, pbc)`: beads that cross a whole brick in one period, brick 0 -> brick 2 (periodic) or brick 0 -> brick P - 1 (open)
    and the way back.  s.legal: periodic and P = 3 -- the destination is the other neighbour.
  * `crowd(variant)`: 1100 beads that leave one brick through one direction in one rebuild ("face": (2,1,1), +x; "corner": (2,2,2),
    +x+y+z): more than the first mig_cap of 1024 records per direction.
  * `returners()`: (2,1,1), two FIXEDVELOCITY groups with a vector; the test reverses the vectors after the first period, and every
    planted bead re-crosses the face it came through.
  * `many_species(s)`: 300 species, every planted bead with an id of 256 and more and a mass of its own.
  * `passengers(s)`: two species of different mass (the builders alternate them), groups FREE / LANGEVIN / FIXEDVELOCITY (coasting) /
    FROZEN (sitters at rest only; no sitter at rest is LANGEVIN) dealt out so that every planted set holds the first three, LCG64 streams by gid, a weak restraint (period
    20 000 steps) on every fifth planted mover.  LANGEVIN at 1e-6 K and tau = 1e6 ps and the restraints change a trajectory by less
    than 1e-3 A over 30 steps (`perturbation_bound`): the planted margins of 0.1 A and more keep every predicted owner.

Reference (nothing of the device code): `owner_exact` (rational arithmetic), `near_face` (within 4 ulp of L of a face between two
bricks: either side is an acceptable owner), `drift_reference` (the stored positions at every rebuild, bit for bit for beads without a
force: the drift is a correctly rounded fma, the wrap is the device's two strict comparisons; the single-domain wrap back_in_box and
k_mig_classify's wrap are the same statement, so positions are compared bit for bit), `direction_census`."""
from fractions import Fraction

import numpy as np

import restraint_systems as R
from ddcmd_amd.deck import Setup, units_convert

ANG = R.ANG
BOX_A = (96.0, 56.6, 64.0)
RLIST_A = 10.0
UPDATE = 10
FREE, LANGEVIN, FROZEN, FIXEDVELOCITY = 0, 2, 4, 5
GROUP_KINDS = (FREE, LANGEVIN, FIXEDVELOCITY, FROZEN)
GRIDS = [((2, 1, 1), 7), ((1, 1, 2), 7), ((2, 2, 2), 7), ((3, 1, 1), 7), ((1, 3, 1), 7), ((3, 2, 1), 7), ((4, 1, 1), 7),
         ((3, 1, 1), 6), ((1, 3, 1), 5), ((3, 2, 1), 6), ((4, 1, 1), 6), ((3, 2, 1), 3)]
NBG = 1000
NEAR_ULPS = 4
MARGIN_A = 0.1             # every planted mover is at least this far from every face at every rebuild
NCROWD = 1100


def box_of(s):
    return np.array([s.h[0], s.h[4], s.h[8]])


def per_axis(pbc):
    return [bool((int(pbc) >> a) & 1) for a in range(3)]


# ---- reference ------------------------------------------------------------------------------------------------------------------
def faces_exact(L, P):
    """the P + 1 planes k L / P - L / 2 of an axis as Fractions"""
    L = Fraction(float(L))
    return [L * k / P - L / 2 for k in range(P + 1)]


def brick_faces(L, P, periodic):
    """the planes of an axis that separate two bricks: the internal ones, and the outer two where the axis is periodic and divided"""
    f = faces_exact(L, P)
    if P == 1:
        return []
    return f if periodic else f[1:-1]


def _wrap_exact(x, L, periodic):
    if periodic:
        if x > L / 2:
            x -= L
        if x < -L / 2:
            x += L
    return x


def brick_exact(x, L, P, periodic):
    """the brick index of one float64 coordinate along an axis of length L (float64) divided in P: wrap, floor, clamp as k_mig_classify
    states them, in rational arithmetic"""
    L = Fraction(float(L))
    x = _wrap_exact(Fraction(float(x)), L, periodic)
    q = (x + L / 2) / (L / P)
    b = q.numerator // q.denominator
    return min(max(b, 0), P - 1)


def coords_exact(r, box, grid, pbc):
    """(n, 3) brick coordinates"""
    r = np.asarray(r, float).reshape(-1, 3)
    per = per_axis(pbc)
    out = np.zeros(r.shape, np.int64)
    for a in range(3):
        if grid[a] == 1:
            continue
        # float prefilter: the floor is safe where the quotient is further than 1e-9 from an integer; the rest in rationals
        L = float(box[a])
        x = r[:, a].copy()
        if per[a]:
            x = np.where(x > 0.5 * L, x - L, x)
            x = np.where(x < -0.5 * L, x + L, x)
        q = (x + 0.5 * L) / (L / grid[a])
        b = np.floor(q)
        unsafe = np.flatnonzero(np.abs(q - np.rint(q)) < 1e-9)
        b = np.clip(b, 0, grid[a] - 1).astype(np.int64)
        for i in unsafe:
            b[i] = brick_exact(r[i, a], L, grid[a], per[a])
        out[:, a] = b
    return out


def rank_of(coords, grid):
    coords = np.asarray(coords)
    return (coords[..., 2] * grid[1] + coords[..., 1]) * grid[0] + coords[..., 0]


def owner_exact(r, box, grid, pbc):
    """the rank that owns every float64 position (n, 3)"""
    return rank_of(coords_exact(r, box, grid, pbc), grid)


def near_face_axes(r, box, grid, pbc):
    """(n, 3) bool: the coordinate lies within NEAR_ULPS spacings of doubles at L of a plane between two bricks (before or after the wrap)"""
    r = np.asarray(r, float).reshape(-1, 3)
    per = per_axis(pbc)
    out = np.zeros(r.shape, bool)
    for a in range(3):
        L = float(box[a])
        tol = Fraction(NEAR_ULPS) * Fraction(float(np.spacing(L)))
        for f in brick_faces(L, grid[a], per[a]):
            cand = np.flatnonzero(np.abs(r[:, a] - float(f)) < 1e-9 * L)
            for i in cand:
                if abs(Fraction(float(r[i, a])) - f) <= tol:
                    out[i, a] = True
    return out


def near_face(r, box, grid, pbc):
    return near_face_axes(r, box, grid, pbc).any(axis=1)


def acceptable_owner(owner, r, box, grid, pbc):
    """bool per bead: `owner` is owner_exact -- or, for a near_face bead, a brick one step to either side along the axes it is near a
    face of.  Returns (ok, number of beads whose owner was left open)"""
    r = np.asarray(r, float).reshape(-1, 3)
    c = coords_exact(r, box, grid, pbc)
    nf = near_face_axes(r, box, grid, pbc)
    per = per_axis(pbc)
    owner = np.asarray(owner)
    got = np.stack([owner % grid[0], (owner // grid[0]) % grid[1], owner // (grid[0] * grid[1])], 1)
    ok = np.ones(len(r), bool)
    for a in range(3):
        d = got[:, a] - c[:, a]
        if per[a]:
            d = (d + grid[a] // 2 + grid[a]) % grid[a] - grid[a] // 2 if grid[a] > 2 else d
        same = got[:, a] == c[:, a]
        beside = (np.abs(d) == 1) | ((grid[a] == 2) & ~same)
        ok &= same | (nf[:, a] & beside)
    return ok, int(nf.any(axis=1).sum())


def fma64(a, x, p):
    """fma(a, x, p) of float64 arrays, correctly rounded: formed in the 64-bit significand of numpy.longdouble, and in rationals
    wherever that lands too close to the middle between two doubles to decide the rounding"""
    assert np.finfo(np.longdouble).nmant >= 63
    LD = np.longdouble
    a, x, p = np.broadcast_arrays(np.asarray(a, float), np.asarray(x, float), np.asarray(p, float))
    prod = a.astype(LD) * x.astype(LD)
    s = p.astype(LD) + prod
    out = s.astype(np.float64)
    err = (np.abs(p).astype(LD) + np.abs(prod)) * LD(2.0) ** -61
    half = (np.spacing(np.abs(out)) / 2).astype(LD)
    off = np.abs(s - out.astype(LD))
    doubt = np.flatnonzero((np.abs(off - half) <= err).ravel() & (prod != 0).ravel())
    flat = out.ravel().copy()
    af, xf, pf = a.ravel(), x.ravel(), p.ravel()
    for i in doubt:
        flat[i] = float(Fraction(float(af[i])) * Fraction(float(xf[i])) + Fraction(float(pf[i])))
    return flat.reshape(out.shape)


def wrap64(r, box, pbc):
    """back_in_box / k_mig_classify: if (x > 0.5 L) x -= L; if (x < -0.5 L) x += L -- on the periodic axes"""
    r = np.array(r, float)
    for a, on in enumerate(per_axis(pbc)):
        if on:
            L = float(box[a])
            x = r[:, a]
            x = np.where(x > 0.5 * L, x - L, x)
            x = np.where(x < -0.5 * L, x + L, x)
            r[:, a] = x
    return r


def positions(s):
    return R.positions(s)


def velocities(s):
    return np.stack([np.asarray(s.vx, float), np.asarray(s.vy, float), np.asarray(s.vz, float)], 1)


def moves(s):
    """bool per bead: the integrator drifts it (every kind but FROZEN)"""
    if getattr(s, "ngroup", 0) and len(np.asarray(s.group_type)):
        return np.asarray(s.group_type)[np.asarray(s.group)] != FROZEN
    return np.ones(s.natoms, bool)


def drift_reference(s, nsteps, rebuild_every=UPDATE):
    """the stored positions at the rebuild of step 0 and of every step that is a multiple of rebuild_every: a list of (n, 3) float64.
    Every step x = fma(dt, v, x) for the beads that move, with the velocities of the setup; at a rebuild the wrap.  Bit for bit what the
    device holds for FREE beads without a restraint and FIXEDVELOCITY beads; LANGEVIN and restrained beads within perturbation_bound."""
    box = box_of(s)
    r = wrap64(positions(s), box, s.pbc)
    v = velocities(s) * moves(s)[:, None]
    go = np.flatnonzero((v != 0).any(axis=1))
    out = [r.copy()]
    for step in range(1, nsteps + 1):
        r[go] = fma64(float(s.dt), v[go], r[go])
        if step % rebuild_every == 0:
            r = wrap64(r, box, s.pbc)
            out.append(r.copy())
    return out


def direction_census(s, grid, snaps):
    """from the reference's snapshots alone: per rebuild after the first, (count[27] of the direction codes (dx + 1) + 3 (dy + 1) +
    9 (dz + 1) that k_mig_classify gives the beads which change brick, nlocal per rank afterwards, number of beads further than one brick
    away).  The first entry is (zeros, nlocal at step 0, 0)."""
    box, per = box_of(s), per_axis(s.pbc)
    n = grid[0] * grid[1] * grid[2]
    prev = coords_exact(snaps[0], box, grid, s.pbc)
    out = [(np.zeros(27, int), np.bincount(rank_of(prev, grid), minlength=n), 0)]
    for r in snaps[1:]:
        c = coords_exact(r, box, grid, s.pbc)
        d = c - prev
        for a in range(3):
            if per[a]:
                d[:, a] = np.where(d[:, a] > 1, d[:, a] - grid[a], d[:, a])
                d[:, a] = np.where(d[:, a] < -1, d[:, a] + grid[a], d[:, a])
        far = (np.abs(d) > 1).any(axis=1)
        code = (d[:, 0] + 1) + 3 * (d[:, 1] + 1) + 9 * (d[:, 2] + 1)
        cnt = np.bincount(code[~far & (code != 13)], minlength=27)[:27]
        out.append((cnt, np.bincount(rank_of(c, grid), minlength=n), int(far.sum())))
        prev = c
    return out


def possible_codes(grid, pbc):
    """the direction codes k_mig_classify can give on this grid: per axis dd = b - pc after the fold -- {0} undivided; P = 2: +1 from
    brick 0, -1 from brick 1 (through whichever face); P >= 3 periodic: -1, 0, 1; P >= 3 open: what the edges allow"""
    opts = [{0} if grid[a] == 1 else {-1, 0, 1} for a in range(3)]
    return sorted((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1) for dx in opts[0] for dy in opts[1] for dz in opts[2] if (dx, dy, dz) != (0, 0, 0))


def perturbation_bound(s, nsteps):
    """A: how far a LANGEVIN or restrained bead can be from drift_reference after nsteps.  Restraint: |a| = 2 kb |d| / m with |d| <= 8 A in
    every component gives a t^2 / 2; LANGEVIN: friction 1 - exp(-dt / tau) per step on the setup's largest speed and the noise
    sqrt(dt T / (m tau)) per step, both added up over the steps and the path"""
    t = nsteps * s.dt
    m = float(np.min(s.mass))
    b = 0.0
    if int(getattr(s, "nrest", 0)) > 0:
        b += 2.0 * float(np.max(s.rest_kb)) * 8.0 * ANG / m * t * t / 2.0
    gt = np.asarray(getattr(s, "group_type", []))
    for g in np.flatnonzero(gt == LANGEVIN):
        tau, T = float(s.group_tau[g]), float(s.group_Teq[g])
        vmax = float(np.abs(velocities(s)).max())
        b += nsteps * nsteps * (s.dt / tau * vmax * s.dt + s.dt * 6.0 * np.sqrt(s.dt * T / (m * tau)))
    return b / ANG


# ---- builders -------------------------------------------------------------------------------------------------------------------
def _base(grid, pbc, rng, nbg=NBG):
    s = Setup()
    R._forcefield(s, UPDATE)
    s.h = np.array([BOX_A[0], 0, 0, 0, BOX_A[1], 0, 0, 0, BOX_A[2]]) * ANG
    s.pbc = int(pbc)
    s.grid = tuple(grid)
    L = np.array(BOX_A)
    dims = np.array([10, 10, 10])
    k = rng.permutation(1000)[:nbg]
    ijk = np.stack([k % 10, (k // 10) % 10, k // 100], 1)
    r = -0.5 * L + (ijk + 0.5) * L / dims + rng.uniform(-0.3, 0.3, (nbg, 3)) * L / dims
    # the background rests at least 0.5 A from every plane of every grid used (halves, thirds, quarters of a side)
    for a in range(3):
        for P in (2, 3, 4):
            for kk in range(P + 1):
                f = kk * L[a] / P - 0.5 * L[a]
                close = np.abs(r[:, a] - f) < 0.5
                r[close, a] = f + np.where(r[close, a] >= f, 0.75, -0.75)
    assert (np.abs(r) < 0.5 * L).all()
    return s, r


def _brick_bounds(grid):
    L = np.array(BOX_A)
    W = L / np.array(grid)
    return L, W


def _finish(s, r_A, u_A, rng, planted, name):
    """u_A: velocities in A per step"""
    n = len(r_A)
    R._finish(s, r_A, np.asarray(u_A, float) * ANG / s.dt, rng, (np.arange(n) % 2).astype(np.int32))
    s.planted = {k: np.asarray(v, int) for k, v in planted.items()}
    s.planted_all = np.sort(np.concatenate([np.asarray(v, int).ravel() for v in planted.values()])) if planted else np.zeros(0, int)
    s.nrest = 0
    s.name = name
    widths = box_of(s) / ANG / np.array(s.grid)
    assert (widths[np.array(s.grid) > 1] >= RLIST_A).all(), widths
    return s


def physical_directions(grid, pbc, pc):
    """the (dx, dy, dz) != 0 along which the brick at coordinates pc has another brick: an undivided axis has none, an open axis none
    beyond its edge bricks"""
    per = per_axis(pbc)
    opts = []
    for a in range(3):
        o = [0]
        if grid[a] > 1:
            if per[a] or pc[a] > 0:
                o.append(-1)
            if per[a] or pc[a] < grid[a] - 1:
                o.append(1)
        opts.append(o)
    return [(dx, dy, dz) for dz in opts[2] for dy in opts[1] for dx in opts[0] if (dx, dy, dz) != (0, 0, 0)]


def crossers(grid, pbc=7, seed=20261101):
    rng = np.random.RandomState(seed + 100 * rank_of(np.array(grid), (10, 10, 10)) + pbc)
    s, r = _base(grid, pbc, rng)
    L, W = _brick_bounds(grid)
    pos, vel, planted = [r], [np.zeros_like(r)], {}
    n = len(r)
    for rank in range(grid[0] * grid[1] * grid[2]):
        pc = np.array([rank % grid[0], (rank // grid[0]) % grid[1], rank // (grid[0] * grid[1])])
        lo = -0.5 * L + pc * W
        for d in physical_directions(grid, pbc, pc):
            for wave, count in ((1, 8), (2, 4)):
                p = lo + rng.uniform(3.0, W - 3.0, (count, 3))
                u = rng.uniform(-0.02, 0.02, (count, 3))
                for a in range(3):
                    if d[a] == 0:
                        continue
                    ua = rng.uniform(0.08, 0.15, count)
                    # wave 1: 10 u carries the bead 0.25 ... 0.6 A past the face; wave 2: the face is still 0.2 ... 0.5 A ahead after 10
                    # steps and 0.3 ... 1.3 A behind after 20
                    e = UPDATE * ua - rng.uniform(0.25, 0.6, count) if wave == 1 else UPDATE * ua + rng.uniform(0.2, 0.5, count)
                    face = lo[a] + (W[a] if d[a] > 0 else 0.0)
                    p[:, a] = face - d[a] * e
                    u[:, a] = d[a] * ua
                planted[(rank, d, wave)] = np.arange(n, n + count)
                n += count
                pos.append(p); vel.append(u)
    return _finish(s, np.concatenate(pos), np.concatenate(vel), rng, planted, "crossers_%d%d%d_pbc%d" % (tuple(grid) + (pbc,)))


def face_sitters(grid, pbc=7, seed=20261102):
    rng = np.random.RandomState(seed + 100 * rank_of(np.array(grid), (10, 10, 10)) + pbc)
    s, r = _base(grid, pbc, rng)
    Lint = box_of(s)
    L, W = _brick_bounds(grid)
    per = per_axis(pbc)
    planes = []          # per axis: the float64 nearest to every plane between two bricks (internal units)
    for a in range(3):
        fl = [float(f) for f in brick_faces(Lint[a], grid[a], per[a])]
        if per[a] and grid[a] > 1:
            fl[0], fl[-1] = -0.5 * Lint[a], 0.5 * Lint[a]
        planes.append(fl)
    usp = [float(np.spacing(0.5 * Lint[a])) for a in range(3)]
    pos, vel, rest, on_face, outside = [], [], [], [], []

    def interior():
        pc = np.array([rng.randint(g) for g in grid])
        return (-0.5 * L + pc * W + rng.uniform(3.0, W - 3.0)) * ANG

    def add(p, u, at_rest, single):
        pos.append(p); vel.append(u); rest.append(at_rest); on_face.append(single)

    axes_sets = [(a,) for a in range(3) if planes[a]]
    axes_sets += [(a, b) for a in range(3) for b in range(a + 1, 3) if planes[a] and planes[b]]
    if all(planes):
        axes_sets.append((0, 1, 2))
    for axes in axes_sets:
        combos = [[]]
        for a in axes:
            # (a corner at +L/2 is the periodic image of the one at -L/2: corners take the lower outer plane and the first internal one)
            pick = planes[a] if len(axes) == 1 else sorted(set(planes[a][:2] + planes[a][-1:])) if len(axes) == 2 else planes[a][:2]
            combos = [c + [f] for c in combos for f in pick]
        variants = [(k, slow) for k in (-2, -1, 0, 1, 2) for slow in (0, 1, -1)]
        for q, faces in enumerate(combos):
            # a corner is one point: one bead each, the fifteen variants dealt out over the corners (two beads ulps apart would divide
            # by their distance in the pair kernel, whatever eps is)
            for k, slow in (variants if len(axes) < 3 else variants[2 * q % 15:2 * q % 15 + 1]):
                p = interior()
                u = np.zeros(3)
                for a, f in zip(axes, faces):
                    p[a] = f + k * usp[a]
                    u[a] = slow * 1e-3
                add(p, u, slow == 0, len(axes) == 1)
    nface = len(pos)
    for a in range(3):          # outside the box on an open axis: the edge brick keeps them
        if per[a] or grid[a] == 1:
            continue
        for side in (-1.0, 1.0):
            for frac in (1e-9, 0.01, 0.2, 0.45):
                for slow in (0, 1):
                    p = interior()
                    p[a] = side * (0.5 + frac) * Lint[a]
                    u = np.zeros(3)
                    u[a] = side * slow * 0.05
                    add(p, u, slow == 0, False)
    n0 = len(r)
    npl = len(pos)
    r_all = np.concatenate([r * ANG, np.array(pos).reshape(-1, 3)]) / ANG
    u_all = np.concatenate([np.zeros_like(r), np.array(vel).reshape(-1, 3)])
    planted = {"face": np.arange(n0, n0 + nface), "outside": np.arange(n0 + nface, n0 + npl)}
    s = _finish(s, r_all, u_all, rng, planted, "face_sitters_%d%d%d_pbc%d" % (tuple(grid) + (pbc,)))
    # the planted coordinates exactly as built (r_A * ANG need not give them back)
    P = np.array(pos).reshape(-1, 3)
    s.rx[n0:], s.ry[n0:], s.rz[n0:] = P[:, 0], P[:, 1], P[:, 2]
    s.at_rest = np.concatenate([np.ones(n0, bool), np.array(rest, bool)])
    s.single_face = np.concatenate([np.zeros(n0, bool), np.array(on_face, bool)])
    return s


def two_hops(grid, pbc=7, seed=20261103):
    """8 beads from brick 0 to brick 2 (periodic axis) or to brick P - 1 (open axis) along the first axis with P >= 3, and 8 the way back,
    in the first rebuild period.  s.legal: the hop is the other neighbour's (periodic, P = 3)"""
    rng = np.random.RandomState(seed + 100 * rank_of(np.array(grid), (10, 10, 10)) + pbc)
    s, r = _base(grid, pbc, rng)
    L, W = _brick_bounds(grid)
    a = [k for k in range(3) if grid[k] >= 3][0]
    periodic = per_axis(pbc)[a]
    far = 2 if periodic else grid[a] - 1
    pos, vel = [r], [np.zeros_like(r)]
    n = len(r)
    planted = {}
    for name, b0, b1 in (("out", 0, far), ("back", far, 0)):
        p = -0.5 * L + rng.uniform(3.0, W - 3.0, (8, 3))
        x0 = -0.5 * L[a] + (b0 + rng.uniform(0.3, 0.7, 8)) * W[a]
        x1 = -0.5 * L[a] + (b1 + rng.uniform(0.3, 0.7, 8)) * W[a]
        p[:, a] = x0
        u = rng.uniform(-0.02, 0.02, (8, 3))
        u[:, a] = (x1 - x0) / UPDATE          # through the bricks in between, not through the periodic face
        planted[name] = np.arange(n, n + 8)
        n += 8
        pos.append(p); vel.append(u)
    s = _finish(s, np.concatenate(pos), np.concatenate(vel), rng, planted, "two_hops_%d%d%d_pbc%d" % (tuple(grid) + (pbc,)))
    s.legal = bool(periodic and grid[a] == 3)
    s.axis = a
    return s


def crowd(variant, seed=20261104):
    rng = np.random.RandomState(seed + len(variant))
    grid = (2, 1, 1) if variant == "face" else (2, 2, 2)
    s, r = _base(grid, 7, rng)
    L, W = _brick_bounds(grid)
    n0 = len(r)
    if variant == "face":
        p = rng.uniform(-0.5, 0.5, (NCROWD, 3)) * (L - 6.0)
        p[:, 0] = -rng.uniform(0.25, 0.9, NCROWD)
        u = rng.uniform(-0.02, 0.02, (NCROWD, 3))
        u[:, 0] = (-p[:, 0] + rng.uniform(0.25, 0.6, NCROWD)) / UPDATE
        d = (1, 0, 0)
    else:
        # spread over the brick and over the one diagonally opposite: some hundred neighbours within the list radius, not thousands
        span = np.array([45.0, 27.0, 30.0])
        p = -rng.uniform(0.3, span, (NCROWD, 3))
        u = (-p + rng.uniform(0.3, span, (NCROWD, 3))) / UPDATE
        d = (1, 1, 1)
    s = _finish(s, np.concatenate([r, p]), np.concatenate([np.zeros_like(r), u]), rng, {(0, d, 1): np.arange(n0, n0 + NCROWD)}, "crowd_" + variant)
    s.code = (d[0] + 1) + 3 * (d[1] + 1) + 9 * (d[2] + 1)
    return s


def passengers(s0):
    """module docstring; returns a decorated copy"""
    import copy
    import pyoracle
    s = copy.copy(s0)
    n = s.natoms
    _K, _PS = units_convert(1.0, "K"), units_convert(1.0, "ps")
    s.ngroup = 4
    s.group_name = ["free", "langevin", "fixed", "frozen"]
    s.group_type = np.array(GROUP_KINDS, np.int32)
    s.group_Teq = np.array([0.0, 1e-6 * _K, 0.0, 0.0])
    s.group_tau = np.array([0.0, 1e6 * _PS, 0.0, 0.0])
    s.group_interval = np.ones(4, np.int32)
    s.group_vcm = np.zeros((4, 3))
    s.group_vset = np.zeros(4, np.int32)
    s.group_v = np.zeros(12)
    s.rng_seed = 20261105
    gr = (np.arange(n) % 2).astype(np.int32)            # the background: FREE and LANGEVIN
    at_rest = getattr(s, "at_rest", None)
    for idx in s.planted.values():
        idx = np.asarray(idx).ravel()
        j = np.arange(len(idx))
        if at_rest is None:
            gr[idx] = j % 3
        else:
            # sitters come in threes -- at rest, slow up, slow down.  At rest: FREE, FIXEDVELOCITY or FROZEN in turn, never LANGEVIN, whose
            # noise (1e-10 A per step) would carry the bead out of the 4 ulp of its face in a direction no reference knows
            gr[idx] = np.where(at_rest[idx], np.array([0, 2, 3])[(j // 3) % 3], (j // 3 + j) % 3)
    s.group = gr
    s.lcg64 = pyoracle.lcg64_default(s.gid)
    # restraints: every fifth planted mover (sitters: every fifth bead at rest on a single face, free along the face's axis only)
    pl = s.planted_all
    if at_rest is None:
        bead = pl[::5]
        fc = np.ones((len(bead), 3), np.int32)
    else:
        cand = pl[at_rest[pl] & s.single_face[pl] & (gr[pl] == 0)]
        bead = cand[::5]
        fc = None
    if len(bead):
        rng = np.random.RandomState(len(bead))
        bead = bead[rng.permutation(len(bead))]
        if at_rest is not None:
            fc = (~near_face_axes(positions(s)[bead], box_of(s), s.grid, s.pbc)).astype(np.int32)
        disp = rng.uniform(1.0, 3.0, (len(bead), 3)) * rng.choice([-1.0, 1.0], (len(bead), 3))
        w = 2.0 * np.pi / (20000.0 * s.dt)
        kb = s.mass[s.species[bead]] * w * w / 2.0
        L = box_of(s)
        x0 = positions(s)[bead] + disp * ANG
        s.nrest = len(bead)
        s.rest_bead = bead
        s.rest_gid = np.asarray(s.gid, np.uint64)[bead].copy()
        s.rest_fc = np.ascontiguousarray(fc, np.int32)
        s.rest_r0 = np.ascontiguousarray(x0 / L + 0.5)
        s.rest_kb = np.ascontiguousarray(kb)
        s.rest_origin = 0
    s.name = s0.name + "+passengers"
    return s


_made = {}


def system(name, *args, **kw):
    """the named builder's Setup, made once and left unchanged; passengers=True: decorated"""
    key = (name,) + args + (bool(kw.get("passengers")),)
    if key not in _made:
        s = globals()[name](*args)
        _made[key] = passengers(s) if kw.get("passengers") else s
    return _made[key]


_snaps = {}


def snapshots(s, nsteps):
    key = (s.name, nsteps)
    if key not in _snaps:
        _snaps[key] = drift_reference(s, nsteps)
    return _snaps[key]


def min_face_distance(r, s):
    """A: per bead the distance to the nearest plane between two bricks of the setup's grid"""
    box = box_of(s)
    per = per_axis(s.pbc)
    d = np.full(len(r), np.inf)
    for a in range(3):
        for f in brick_faces(box[a], s.grid[a], per[a]):
            d = np.minimum(d, np.abs(r[:, a] - float(f)))
    return d / ANG


def many_species(s0, nspecies=300):
    """a copy with `nspecies` species that are the gas's two over and over (species 2 q + t has the mass, LJ type and molecule type of
    species t, ids of 256 and more a quarter heavier): every planted bead gets an id of 256 and more, so that a species decoded from fewer than nine bits of a migration
    record is another species of another mass"""
    import copy
    s = copy.copy(s0)
    assert nspecies % 2 == 0 and nspecies > 258
    t = np.asarray(s0.species, np.int64)
    q = (np.arange(s.natoms) * 7) % (nspecies // 2)
    pl = s.planted_all
    q[pl] = 128 + np.arange(len(pl)) % (nspecies // 2 - 128)
    s.species = (2 * q + t).astype(np.int32)
    s.nspecies = nspecies
    for key in ("mass", "charge", "ljtype", "moltype", "resitype", "atomoffset"):
        setattr(s, key, np.tile(np.asarray(getattr(s0, key)), nspecies // 2))
    # ... but for the mass: species 256 and up are a quarter heavier, so that a bead taken for species id & 0xff answers a restraint's
    # force and the LANGEVIN noise with another velocity (a download reads the species out of the tag word, not out of what
    # k_unpack_mig decoded: only the physics shows the decoded one)
    s.mass = np.asarray(s.mass, float) * (1.0 + 0.25 * (np.arange(nspecies) // 256))
    s.species_name = ["S%d" % k for k in range(nspecies)]
    s.name = s0.name + "+%dspecies" % nspecies
    return s


NRETURN = 16
U_RETURN = 0.1            # A per step


def returners(seed=20261106):
    """(2,1,1): two FIXEDVELOCITY groups with a vector, +x and -x at 0.1 A per step, 16 beads each 0.25 ... 0.6 A on the near side of the
    face x = 0 (and 16 each at the periodic face): they cross in the first period; the test then reverses both vectors
    (`reversed_velocity`) and they come back in the second -- arrivals that k_unpack_mig appended leave again at the next rebuild"""
    rng = np.random.RandomState(seed)
    grid = (2, 1, 1)
    s, r = _base(grid, 7, rng)
    L, W = _brick_bounds(grid)
    n0 = len(r)
    pos, vel, grp, planted = [r], [np.zeros_like(r)], [np.zeros(n0, int)], {}
    n = n0
    for g, sign in ((1, 1.0), (2, -1.0)):
        for face in (0.0, sign * 0.5 * L[0]):
            p = rng.uniform(-0.5, 0.5, (NRETURN, 3)) * (L - 6.0)
            p[:, 0] = face - sign * rng.uniform(0.25, 0.6, NRETURN)
            u = np.zeros((NRETURN, 3))
            u[:, 0] = sign * U_RETURN
            planted[(g, face != 0.0)] = np.arange(n, n + NRETURN)
            n += NRETURN
            pos.append(p); vel.append(u); grp.append(np.full(NRETURN, g))
    s = _finish(s, np.concatenate(pos), np.concatenate(vel), rng, planted, "returners")
    s.group = np.concatenate(grp).astype(np.int32)
    s.ngroup = 3
    s.group_name = ["free", "right", "left"]
    s.group_type = np.array([FREE, FIXEDVELOCITY, FIXEDVELOCITY], np.int32)
    s.group_Teq, s.group_tau = np.zeros(3), np.zeros(3)
    s.group_interval = np.ones(3, np.int32)
    s.group_vcm = np.zeros((3, 3))
    s.group_vset = np.array([0, 1, 1], np.int32)
    v = U_RETURN * ANG / s.dt
    s.group_v = np.array([0, 0, 0, v, 0, 0, -v, 0, 0], float)
    # the beads start with exactly the group's vector
    s.vx[s.group == 1], s.vx[s.group == 2] = v, -v
    return s


def returners_reference(s):
    """stored positions at the rebuilds of steps 0, 10 (outward) and 20 (the vectors reversed after step 10)"""
    box = box_of(s)
    r = wrap64(positions(s), box, s.pbc)
    v = velocities(s)
    out = [r.copy()]
    for sign in (1.0, -1.0):
        for _ in range(UPDATE):
            r = fma64(float(s.dt), sign * v, r)
        r = wrap64(r, box, s.pbc)
        out.append(r.copy())
    return out

"""Planted cholesterol systems for the cholAnalysis pass (helper module, no tests in here).

The gas of restraint_systems.py (every pair term vanishes identically, so beads stay where they are planted) holding 8-bead CHOL
residues of chosen geometry among three times as many other beads; residue ids are a random permutation, so the molecules' gids are
interleaved with the others' and the list is in no gid order.  All coordinates are multiples of 2^-36 (internal units): every bond
difference is exact in float64, so the float64 lane and the longdouble reference start from the same bonds.

  * `system(nmol, pbc)`: nmol molecules, 24 nmol other beads, in a box grown with nmol (about 0.012 beads / A^3).  The first molecules
    of a system of 400 or more are the planted edge cases (EDGE_CASES, axis-aligned and dyadic: dR1 and dR5 are exact; four of them sit
    exactly on a bin edge, which the 1 % share allows from 400 molecules on), the next ones of 63 or more sit on every periodic face
    and on a corner, the rest anywhere.  Offsets are drawn from [RMIN - 1, RMAX + 1].
  * `split_system()`: the box of restraint_systems.py for the brick grids: per axis three molecules cut 1+6, 3+4 and 6+1 by the
    internal face of a grid of twos, one molecule at the origin with a bead in each of seven octants, twenty whole molecules, and
    nothing at all in the octant x, y, z > 0.
  * `reference(r7, box, pbc)`: the issue's formulas in numpy.longdouble.
  * `d_bound`, `q_bound`: the derived rounding bounds (their docstrings)."""
import numpy as np

import restraint_systems as R
from ddcmd_amd.deck import Setup

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
GRID = 2.0 ** -36
RMIN, DELTA, NBINS = -4.0, 0.25, 32          # internal length units; RMAX = 4
RMAX = RMIN + DELTA * NBINS
SIZES = (1, 63, 64, 65, 257, 1025)
# the planted shapes: bond lengths of the triangle sides in [BMIN, BMAX], the sine of their angle at least SINMIN, the third bond at most AMAX
BMIN, BMAX, SINMIN, AMAX = 2.5, 4.0, 0.76, 5.5
# (h1, h5) of the exact molecules; None: beads 0, 2, 3 collinear (dR1 = 0/0).  Bins with RMIN, DELTA, NBINS: see expected_edge_bins
EDGE_CASES = ((0.5, -0.25), (RMIN, RMAX), (RMIN - 1.0, RMAX + 0.5), (None, 1.125), (3.9375, -4.0))


NEAR_EDGE_CASES = 4      # of EDGE_CASES, the molecules with an offset exactly on an integer (h - RMIN) / DELTA


def expected_edge_bins():
    """the bins of EDGE_CASES by hand: (h - RMIN) / DELTA is exact for these dyadic values; below RMIN and NaN: 0; at and above RMAX: NBINS - 1"""
    def b(h):
        if h is None:
            return 0
        return int(min(max((h - RMIN) / DELTA, 0.0), NBINS - 1))
    out = [(b(h1), b(h5)) for h1, h5 in EDGE_CASES]
    assert out == [(18, 15), (0, 31), (0, 31), (0, 20), (31, 0)]
    return out


def _quant(x):
    return np.rint(np.asarray(x, float) / GRID) * GRID


def _edge_molecule(k, h1, h5):
    """axis-aligned and dyadic, away from every face: B = (4,0,0), C = (0,2,0), A = (1, 0.5, h1): dR1 = 8 h1 / 8 = h1 exactly;
    E = (0,0,-4), F = (2,0,0), D = (0.5, h5, 1): E x F = (0,-8,0), dR5 = -(-8 h5) / 8 = h5 exactly"""
    r0 = np.array([-24.0 + 8.0 * k, 4.0, -8.0])
    r = np.zeros((8, 3))
    r[0] = r0
    r[2] = r0 + (4.0, 0.0, 0.0)
    r[3] = r0 + ((2.0, 0.0, 0.0) if h1 is None else (0.0, 2.0, 0.0))
    r[1] = r0 + (1.0, 0.5, 0.0 if h1 is None else h1)
    r[4] = r[3] + (0.0, 0.0, 4.0)
    r[6] = r[4] + (2.0, 0.0, 0.0)
    r[5] = r[4] + (0.5, h5, 1.0)
    r[7] = r[6] + (1.0, 1.0, 1.0)
    return r


def _random_shape(rng, h1=None, h5=None):
    """8 local positions (internal units) with dR1 = h1 and dR5 = h5 up to the roundings of the construction"""
    h1 = rng.uniform(RMIN - 1.0, RMAX + 1.0) if h1 is None else h1
    h5 = rng.uniform(RMIN - 1.0, RMAX + 1.0) if h5 is None else h5
    r = np.zeros((8, 3))
    b, c, phi = rng.uniform(BMIN, BMAX), rng.uniform(BMIN, BMAX), np.radians(rng.uniform(50.0, 130.0))
    r[2] = (b, 0.0, 0.0)
    r[3] = (c * np.cos(phi), c * np.sin(phi), 0.0)
    r[1] = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), h1)
    w = rng.normal(size=3)
    w *= rng.uniform(BMIN, BMAX) / np.linalg.norm(w)
    r[4] = r[3] + w                                   # E = -w
    eh = -w / np.linalg.norm(w)
    n5 = np.cross(eh, rng.normal(size=3))
    n5 /= np.linalg.norm(n5)
    mh = np.cross(n5, eh)
    f, th = rng.uniform(BMIN, BMAX), np.radians(rng.uniform(50.0, 130.0))
    r[6] = r[4] + f * (np.cos(th) * eh + np.sin(th) * mh)          # E x F is parallel to n5
    r[5] = r[4] + rng.uniform(-1.5, 1.5) * eh + rng.uniform(-1.5, 1.5) * mh - h5 * n5
    r[7] = r[6] + rng.uniform(-1.0, 1.0, 3) + 2.0
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return r @ q.T


def _box(nbeads):
    f = max(1.0, (nbeads / 0.012 / np.prod(R.BOX_A)) ** (1.0 / 3.0))
    return _quant(np.array(R.BOX_A) * f * R.ANG)


def _finish(s, mol_r, other_r, rng, name):
    """Setup from the molecules' positions [nmol, 8, 3] and the other beads' [nother, 3] (internal units, already in the box):
    residue ids a random permutation, gid = resid << 16 | bead, beads shuffled; s.gid7 the list in molecule order"""
    nmol, nother = len(mol_r), len(other_r)
    resid = rng.permutation(nmol + nother).astype(np.uint64)
    mg = (resid[:nmol, None] << np.uint64(16)) | np.arange(8, dtype=np.uint64)[None, :]
    og = resid[nmol:] << np.uint64(16)
    r = np.concatenate([np.asarray(mol_r, float).reshape(-1, 3), np.asarray(other_r, float).reshape(-1, 3)])
    gid = np.concatenate([mg.reshape(-1), og])
    order = rng.permutation(len(gid))
    r, gid = r[order], gid[order]
    n = len(gid)
    s.natoms = n
    s.rx, s.ry, s.rz = (np.ascontiguousarray(r[:, c]) for c in range(3))
    s.vx, s.vy, s.vz = (np.zeros(n) for _ in range(3))
    s.species = (np.arange(n) % 2).astype(np.int32)
    s.group = np.zeros(n, np.int32)
    s.gid = np.ascontiguousarray(gid)
    s.gid7 = np.ascontiguousarray(mg[:, :7])
    s.mol_r = np.asarray(mol_r, float)[:, :7].copy()
    s.name = name
    return s


def _wrap(r, L, pbc):
    r = np.array(r, float)
    for a in range(3):
        if (pbc >> a) & 1:
            r[..., a] -= L[a] * np.rint(r[..., a] / L[a])
    return r


def system(nmol, pbc=7, seed=20261021):
    rng = np.random.RandomState(seed + 7 * nmol + pbc)
    s = Setup()
    R._forcefield(s)
    L = _box(32 * nmol)
    s.h = np.array([L[0], 0, 0, 0, L[1], 0, 0, 0, L[2]])
    s.pbc = int(pbc)
    mols = []
    edge = EDGE_CASES if nmol >= 100 * NEAR_EDGE_CASES else ()      # (the share condition: at most 1 % of the molecules on a bin edge)
    for k, (h1, h5) in enumerate(edge[:nmol]):
        mols.append(_edge_molecule(k, h1, h5))
    faces = [(a, sgn) for a in range(3) for sgn in (-1.0, 1.0)] + [(-1, 1.0)]      # (-1: the corner)
    while len(mols) < nmol:
        c = rng.uniform(-0.5, 0.5, 3) * L
        if faces and nmol >= 63:
            a, sgn = faces.pop()
            if a < 0:
                c = 0.5 * L
            else:
                c[a] = sgn * 0.5 * L[a]
        for a in range(3):
            if not (pbc >> a) & 1:
                c[a] = np.clip(c[a], -0.5 * L[a] + 12.0, 0.5 * L[a] - 12.0)      # an open axis: nothing leaves the box
        shape = _random_shape(rng)
        mols.append(_quant(_wrap(c + shape - shape[:7].mean(axis=0), L, pbc)))
    s.nedge = len(edge[:nmol])
    other = _quant(rng.uniform(-0.5, 0.5, (24 * nmol, 3)) * (L - 1.0))
    return _finish(s, np.array(mols), other, rng, "chol%d_pbc%d" % (nmol, pbc))


def _cut(shape, axis, m):
    """the shape shifted along `axis` so that exactly m of its first seven beads lie below 0, none within 0.25 of it"""
    x = np.sort(shape[:7, axis])
    assert x[m] - x[m - 1] > 0.6, "the shape has no gap to put the face in"
    out = shape.copy()
    out[:, axis] -= 0.5 * (x[m] + x[m - 1])
    return out


def split_system(seed=31):
    """module docstring; s.nsplit_on[a]: the molecules the internal face of axis a cuts (the corner molecule included)"""
    rng = np.random.RandomState(seed)
    s = Setup()
    R._forcefield(s)
    L = _quant(np.array(R.BOX_A) * R.ANG)
    s.h = np.array([L[0], 0, 0, 0, L[1], 0, 0, 0, L[2]])
    s.pbc = 7
    mols = []
    for axis in range(3):
        for k, m in enumerate((1, 3, 6)):
            while True:
                shape = _random_shape(rng)
                x = np.sort(shape[:7, axis])
                if x[m] - x[m - 1] > 0.6:
                    break
            shape = _cut(shape, axis, m)
            for b in range(3):
                if b != axis:
                    shape[:, b] += -14.0 - 9.0 * k - shape[:, b].max()      # well below 0 on the other axes
            shape[7, axis] = abs(shape[7, axis]) * (-1.0)
            mols.append(_quant(shape))
    # the corner: role k in octant k + 1's complement pattern -- seven octants, never x, y, z > 0 together
    octants = [(-1, -1, -1), (1, -1, -1), (-1, 1, -1), (1, 1, -1), (-1, -1, 1), (1, -1, 1), (-1, 1, 1)]
    mag = np.array([[1.0, 2.0, 1.5], [2.5, 1.0, 0.75], [0.5, 2.25, 2.0], [1.5, 1.25, 2.5], [2.0, 0.5, 1.0], [1.25, 1.75, 0.5], [0.75, 1.5, 2.25]])
    corner = np.zeros((8, 3))
    corner[:7] = mag * np.array(octants, float)
    corner[7] = (-3.0, -3.0, -3.0)
    mols.append(corner)
    while len(mols) < 30:
        shape = _random_shape(rng)
        c = rng.uniform(-0.45, 0.45, 3) * L
        r = c + shape - shape[:7].mean(axis=0)
        lo = r[:7].min(axis=0)
        if (lo > -6.0).all() and (r[:7].max(axis=0) > -6.0).all():
            continue                                   # stay out of the empty octant and off the internal faces' far side
        if (np.abs(r[:7]) < 0.3).any() or ((r[:7] > 0).all(axis=1)).any() or (np.abs(r) > 0.5 * L - 0.3).any():
            continue
        mols.append(_quant(r))
    other = rng.uniform(-0.5, 0.5, (24 * 30 * 2, 3)) * (L - 1.0)
    other = _quant(other[~(other > 0).all(axis=1)][:24 * 30])
    s.nedge = 0
    out = _finish(s, np.array(mols), other, rng, "chol_split")
    assert not ((positions(out) > 0).all(axis=1)).any()
    out.nsplit_on = [int(sum(((m[:7, a] < 0).any() and (m[:7, a] > 0).any()) for m in out.mol_r)) for a in range(3)]
    return out


def positions(s):
    return np.stack([np.asarray(s.rx, float), np.asarray(s.ry, float), np.asarray(s.rz, float)], 1)


def box_of(s):
    return np.array([s.h[0], s.h[4], s.h[8]])


def reference(r7, box, pbc):
    """dR1, dR5 [nmol] in longdouble of the positions r7[nmol, 7, 3] (float64 values, taken as exact): b(i,j) = nearestImage(r_j - r_i)
    on the periodic axes, A = b(0,1), B = b(0,2), C = b(0,3), D = b(4,5), E = b(4,3), F = b(4,6), x1 = B x C, dR1 = (x1.A)/sqrt(x1.x1),
    x3 = E x F, dR5 = -(x3.D)/sqrt(x3.x3); collinear beads give NaN"""
    r = np.asarray(r7, LD).reshape(-1, 7, 3)
    L = np.asarray(box, LD)
    per = np.array([(int(pbc) >> a) & 1 for a in range(3)], bool)

    def b(i, j):
        d = r[:, j] - r[:, i]
        return d - np.where(per, L * np.rint(d / L), 0)

    def cross(u, v):
        return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)

    A, B, C, D, E, F = b(0, 1), b(0, 2), b(0, 3), b(4, 5), b(4, 3), b(4, 6)
    with np.errstate(all="ignore"):
        x1, x3 = cross(B, C), cross(E, F)
        d1 = (x1 * A).sum(axis=1) / np.sqrt((x1 * x1).sum(axis=1))
        d5 = -(x3 * D).sum(axis=1) / np.sqrt((x3 * x3).sum(axis=1))
    return d1, d5


def bins_of(d, rmin=RMIN, delta=DELTA, nbins=NBINS):
    """(bin, q) of longdouble offsets: q = (d - rmin) / delta, bin = (int)MIN(MAX(q, 0), nbins - 1), a NaN in bin 0"""
    q = (np.asarray(d, LD) - LD(rmin)) / LD(delta)
    with np.errstate(all="ignore"):
        t = np.where(q > 0, q, 0)
        t = np.where(t < nbins - 1, t, nbins - 1)
    return np.floor(t).astype(np.int64), q


def d_bound(Lmax):
    """|d_float64 - d_exact| for the planted shapes.  The bonds: the difference of two grid coordinates is exact; a wrapped component
    adds the rounded product L da (at most u L) and one rounded sum (at most u AMAX): eb = u (Lmax + AMAX) per component.  d = n . a
    with n the triangle's unit normal: an error eb in each component of a moves d by at most sqrt(3) eb; one of eb in the components
    of the sides u, v turns n by at most 2 sqrt(3) eb (1/|u| + 1/|v|) / sin <= 4 sqrt(3) eb / (BMIN SINMIN) and moves d by AMAX times
    that.  The arithmetic behind the bonds -- six products and three differences for the cross product, three products and two sums
    for each dot product, a square root and a division, fewer than 24 roundings in all, each relative to a term of size at most
    |x| |a| before the division by |x| -- adds at most 24 u AMAX / SINMIN (the cancellations in the cross product are bounded by the sine)."""
    eb = U * (Lmax + AMAX)
    return np.sqrt(3.0) * eb * (1.0 + 4.0 * AMAX / (BMIN * SINMIN)) + 24.0 * U * AMAX / SINMIN


def q_bound(Lmax, rmin=RMIN, delta=DELTA, nbins=NBINS):
    """how far (d - rmin) / delta in float64 may lie from the longdouble value: d_bound / delta, the subtraction's and the division's
    roundings relative to a quotient of at most nbins + 8 in magnitude for the planted offsets"""
    return d_bound(Lmax) / delta + 2.0 * U * (nbins + 8)


_made = {}


def made(name, *args):
    """the named builder's Setup, made once and left unchanged"""
    key = (name,) + args
    if key not in _made:
        _made[key] = globals()[name](*args)
    return _made[key]

"""Adversarial systems for the single-precision filter of the list search (helper module, no tests in here).

k_tile_build (ddcmi_listbuild.inl) decides which pairs enter the neighbour list from `float` coordinates relative to the tile
centre; the double-precision test `X * X + Y * Y + Z * Z < rl2` runs only inside a band around the list radius, and before that
the 5x5x5 cells around a bead are cut down with `float` gaps and fixed margins.  Thermal water holds all of that loosely: about
one pair in 5 M lies within 1e-7 of the list radius, none sits at a cell face with its partner two cells away.  The systems of this
module put the pairs THERE.

The grid, restated (`grid_of`):
  ddcmi_rebuild.inl, setup_grid:   `double W = L[a] / P;`  `gp.lo[a] = -0.5 * L[a] + ctx->pcoord[a] * W;`  `double cmin = 0.5 * rlist;`
                                   `int n = (int)floor(W / cmin);`  `const int r = n % tdim0[a];`
                                   `if (r > 0 && 2 * r <= tdim0[a] && n - r >= tdim0[a] && (double)n / (double)(n - r) <= 1.02) n -= r;`
                                   `gp.cinv[a] = (double)n / W;`  `gp.m[a] = (periodic || P > 1) ? tdim[a] : 0;`  `gp.g[a] = n + 2 * gp.m[a];`
                                   `gp.T[a] = (gp.g[a] + tdim[a] - 1) / tdim[a];`  `ncell *= gp.T[a] * tdim[a];`
  ddcmi_internal.h:                TCX, TCY, TCZ = 8, 4, 4
  ddcmi.hip, cell_coords:          `int ic = (int)floor((r[a] - gp.lo[a]) * gp.cinv[a]);  if (owned) ic = min(max(ic, 0), gp.n[a] - 1);  ic += gp.m[a];`
  ddcmi.hip, image_dirs:           the beads of the two outermost layers of cells of a periodic axis have an image at r +- L, in their
                                   own cell moved by n cells (k_fill_images); k_halo_update forms it as `p.x += (double)(code % 3 - 1) * L0`
  ddcmi_listbuild.inl:             `const double ox = gp.lo[0] + (TCX * tx - gp.m[0] + 0.5 * TCX) / gp.cinv[0]`, the staged `(float)(p.x - ox)`,
                                   `const double band = 4.0 * (4.0 * 1.7320508 * gp.rlist * (double)amax + 4.0 * rl2) * 5.9604645e-8 / rl2;`
                                   `rl2_hi = (float)(rl2 * (1.0 + band)), rl2_lo = (float)(rl2 * (1.0 - band))`; a tile stages the cells within two
                                   cells of it, amax is the largest |staged coordinate| of all of them.

The probe gas (`gas(name)`): probe pairs on a coarse lattice of sites.  A site's beads stay within SITE_REACH_A of its centre and
sites are at least SITE_A apart, so no bead of another site comes within rlist + MARGIN_A of a probe (`foreign_distance` measures it; the host
test asserts it).  The exact list is then known pair by pair: (i, j) is in it iff d^2 < rl2.  rcut 12 A, skin 4 A.  Pair families
(Setup.pair_family, with pair_e, pair_dir, pair_tag, pair_i, pair_j):

  sweep    d = rlist (1 + e), e = +-E_VALUES, along the axes, the face diagonals, the body diagonal and a generic direction
  band     d^2 = rl2 (1 +- band (1 +- 0.1)) with the band of the first bead's tile, restated from the tile's amax
  adverse  pairs at e = +-3e-8 placed, by a seeded search, where the single-precision r^2 falls on the wrong side of the list radius by more
           than a sixteenth of the band
  inner    a few pairs inside the cut-off (the forces of the gas are theirs)
  face     sweep pairs across every periodic face: the partners meet as images of each other
  domain   sweep pairs across the mid planes (the internal faces of 2-way decompositions), some with a bead exactly ON the plane
  place    first bead in one of the eight corner cells or in a centre cell of an interior tile, partner two cells outside the
           tile -- the outer ring of the staged region, where the staged coordinates are largest (48 A in x)
  prune    first bead on a face of its cell (on it, one ulp below, one ulp above), partner at rlist (1 - e) along +- the axis: two cells
           away for the bead on the far side of the face, one for the bead on the near side; and corner beads with partners at
           (+-2, +-1, +-1) cells, in every order of the axes and every combination of signs
  outside  (open axes) a pair three list radii outside the box and one 1000 A outside: clamped into edge cells, a widened band
  facecell first bead exactly on the low face of the box or on a mid plane, so that its image or received copy lies exactly on a high face, in a
           box where `floor((r - lo) * cinv)` alone files that point in the last interior cell; a third bead of the site is owned by that
           cell; the partner at rlist (1 - 1e-7) from the image (halo_cell's side forcing, ddcmi.hip)

Systems (`GAS`): "sweep" 562 A cubic; "place" 645 x 516 x 516 A; "prune_exact" 400 A (cells exactly rlist / 2 wide), "prune_eps" the same
times (1 + 1e-12), "prune_fold" 459 A (57 cells fold to 56 on every axis); "noncubic" 2 : 3 : 5; "open" pbc = 0 and "mixed" pbc = 5; "face_cell" 579.1 A (72 cells, 36 per half; L * (72 / L) rounds below 72).
Variants: one_type (pack_type 2: k_tile_build<false, 2>, 16-bit scratch words), types20 (20 LJ types: bare entries, k_tile_build<false, 0>,
32-bit scratch words), mol (every probe is atom 0 of a two-bead molecule whose atom 1 sits 5 A off the pair's axis: k_tile_build<true, 2>;
partners are in different molecules, every molecule adds one excluded pair) -- read from bl_plan: `ctx->pack_type = (ctx->stage_cap <
4096 && ctx->nnb <= 8) ? 2 : 0`, `has_mol |= ctx->mol_nspecies[m] > 1`.  k_tile_build<true, 0> is not reached here.

`crowded()` adds a clump of 448 beads on a 3.5 A lattice to a small gas: the build starts with rows of 24 words and LDS room for 384
staged beads (bl_plan: `tmpw = ((int)(expect * 1.25) + 24 + 7) & ~7`, `if (ctx->stage_cap < 384) ctx->stage_cap = 384`) and has to be started
over for both.  `nudged_water()` is make_water_setup(12) with about 2000 beads moved along the line to a chosen neighbour until their
distance is rlist (1 + e): full tiles, real amax values, thousands of pairs at the edge.

References: `reference_list(s, dtype)` all pairs under the minimum image in longdouble or float64 (the water box in float64, its pairs
within 1e-3 of the list radius again in longdouble: `near_pairs`).  rl2 is the device's: the double rlist = rmax + deltaR squared in double.
`staged_error(s)` emulates the staged arithmetic in float32 and returns the error of r^2 against the band.  Ambiguity floor: a pair with
|d^2 / rl2 - 1| < 2^-45 could be decided either way (the device subtracts an image position, the reference reduces a difference); no system
here holds one (`ambiguous`), so nothing is excluded from any comparison."""
import itertools

import numpy as np

from ddcmd_amd.deck import Setup, units_convert
from ddcmd_amd.synth import water_forcefield, make_water_setup, relabel_types

TC = np.array([8, 4, 4])        # ddcmi_internal.h: TCX, TCY, TCZ
IMG_LAYERS = 2                  # ddcmi.hip: #define IMG_LAYERS 2
FOLD_LIMIT = 1.02               # setup_grid: (double)n / (double)(n - r) <= 1.02
BAND_FACTOR = 4.0               # k_tile_build: band = 4.0 * (...)
SQRT3_F, EPS24_F = 1.7320508, 5.9604645e-8      # the band's constants as the kernel writes them
AMBIGUITY = 2.0 ** -45
ANG = units_convert(1.0, "Angstrom")
RCUT_A, SKIN_A = 12.0, 4.0
MARGIN_A = 4.0                  # no foreign bead within rlist + MARGIN_A of a probe
SITE_REACH_A = 30.0             # a site's beads stay within this of its centre (prune: a cell diagonal 14 A + a list radius 16 A)
SITE_A = 2.0 * SITE_REACH_A + RCUT_A + SKIN_A + MARGIN_A      # smallest site spacing (80 A): a box holds floor(L / SITE_A) sites per axis
E_VALUES = (3e-14, 1e-12, 1e-10, 1e-8, 3e-8, 1e-7, 3e-7, 1e-6, 3e-6, 1e-5, 1e-4, 1e-3)
E_SHORT = (1e-10, 3e-8, 1e-6)
VARIANTS = ("one_type", "types20", "mol")
DIRECTIONS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, -1), (0, 1, 1), (1, -1, 0), (1, 1, 1), (0.36, -0.48, 0.8)], float)
DIRECTIONS /= np.sqrt((DIRECTIONS ** 2).sum(axis=1))[:, None]
DIR_NAMES = ("x", "y", "z", "xy", "x-z", "yz", "x-y", "xyz", "generic")
GAS = {"sweep": dict(box_A=(562.1, 562.1, 562.1), pbc=7, families=("inner", "sweep", "band", "adverse", "face", "domain")),
       "place": dict(box_A=(645.0, 516.0, 516.0), pbc=7, families=("place",)),
       "prune_exact": dict(box_A=(400.0, 400.0, 400.0), pbc=7, families=("inner", "prune")),
       "prune_eps": dict(box_A=(400.0, 400.0, 400.0), scale=1.0 + 1e-12, pbc=7, families=("inner", "prune")),
       "prune_fold": dict(box_A=(459.0, 459.0, 459.0), pbc=7, families=("inner", "prune")),
       "noncubic": dict(box_A=(322.6, 483.9, 806.5), pbc=7, families=("inner", "sweep_short", "prune")),
       "open": dict(box_A=(562.1, 562.1, 562.1), pbc=0, families=("inner", "sweep_short", "outside")),
       "mixed": dict(box_A=(562.1, 562.1, 562.1), pbc=5, families=("inner", "sweep_short", "outside", "face")),
       "face_cell": dict(box_A=(579.1, 579.1, 579.1), pbc=7, families=("inner", "facecell"))}


class Grid(object):
    """setup_grid restated: n, cinv, lo, m, g, T per axis, ncell (= list_stats()["cells"])"""

    def __init__(self, L, pbc, rlist, pgrid=(1, 1, 1), pcoord=(0, 0, 0)):
        self.L, self.rlist, self.pbc = np.asarray(L, np.float64), float(rlist), int(pbc)
        self.n, self.m = np.zeros(3, np.int64), np.zeros(3, np.int64)
        self.cinv, self.lo = np.zeros(3), np.zeros(3)
        self.folded = [False] * 3
        for a in range(3):
            periodic = bool((self.pbc >> a) & 1)
            W = self.L[a] / pgrid[a]
            self.lo[a] = -0.5 * self.L[a] + pcoord[a] * W
            n = max(int(np.floor(W / (0.5 * self.rlist))), 1)
            r = n % TC[a]
            if r > 0 and 2 * r <= TC[a] and n - r >= TC[a] and float(n) / float(n - r) <= FOLD_LIMIT:
                n -= r
                self.folded[a] = True
            self.n[a], self.cinv[a] = n, float(n) / W
            self.m[a] = TC[a] if (periodic or pgrid[a] > 1) else 0
        self.g = self.n + 2 * self.m
        self.T = (self.g + TC - 1) // TC
        self.ncell = int(np.prod(self.T * TC))

    def owned_cell(self, r):
        """cell_coords(owned) without the margin: floor((r - lo) * cinv) clamped into 0 .. n - 1; r: (..., 3)"""
        ic = np.floor((np.asarray(r) - self.lo) * self.cinv).astype(np.int64)
        return np.minimum(np.maximum(ic, 0), self.n - 1)

    def raw_cell(self, r):
        return np.floor((np.asarray(r) - self.lo) * self.cinv).astype(np.int64)

    def tile_of(self, r):
        return (self.owned_cell(r) + self.m) // TC

    def tile_centre(self, t):
        return self.lo + (TC * np.asarray(t) - self.m + 0.5 * TC) / self.cinv

    def face(self, a, c):
        """the coordinate of the low face of owned cell c on axis a, as the first double that floor((r - lo) * cinv) puts into cell c"""
        x = self.lo[a] + c / self.cinv[a]
        cell = lambda v: int(np.floor((v - self.lo[a]) * self.cinv[a]))
        lo, hi = x - 1e-6, x + 1e-6          # bisection over the doubles: lo stays below the face, hi on or above it
        assert cell(lo) < c <= cell(hi)
        while True:
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if cell(mid) >= c:
                hi = mid
            else:
                lo = mid
        assert np.nextafter(hi, -np.inf) == lo
        x = hi
        return float(x)


def rlist_of(s):
    return float(s.rmax) + float(s.deltaR)


def rl2_of(s):
    return rlist_of(s) * rlist_of(s)


def box_of(s):
    return np.array([s.h[0], s.h[4], s.h[8]])


def grid_of(s, pgrid=(1, 1, 1), pcoord=(0, 0, 0)):
    return Grid(box_of(s), s.pbc, rlist_of(s), pgrid, pcoord)


def positions(s):
    return np.stack([np.asarray(s.rx, np.float64), np.asarray(s.ry, np.float64), np.asarray(s.rz, np.float64)], 1)


def band_of(rlist, amax):
    """(band, rl2_lo, rl2_hi) of a tile whose largest staged coordinate is amax (a float32)"""
    rl2 = rlist * rlist
    band = BAND_FACTOR * (4.0 * SQRT3_F * rlist * float(amax) + 4.0 * rl2) * EPS24_F / rl2
    return band, np.float32(rl2 * (1.0 - band)), np.float32(rl2 * (1.0 + band))


def staged_copies(s, g):
    """every bead a tile can stage: the owned beads and their periodic images.  (position, grid cell with the margin, bead index)"""
    r = positions(s)
    ic = g.owned_cell(r)
    idx = np.arange(len(r))
    R, C, I = [r], [ic + g.m], [idx]
    for sh in itertools.product((-1, 0, 1), repeat=3):
        if sh == (0, 0, 0):
            continue
        ok = np.ones(len(r), bool)
        for a in range(3):
            if sh[a] != 0 and g.m[a] == 0:
                ok[:] = False
            elif sh[a] == 1:
                ok &= ic[:, a] < IMG_LAYERS
            elif sh[a] == -1:
                ok &= ic[:, a] >= g.n[a] - IMG_LAYERS
        if ok.any():
            shv = np.array(sh)
            R.append(r[ok] + shv * g.L); C.append(ic[ok] + g.m + shv * g.n); I.append(idx[ok])
    return np.concatenate(R), np.concatenate(C), np.concatenate(I)


def tile_amax(s, g=None):
    """{tile (tx, ty, tz): amax} for every tile that owns a bead: the largest |(float)(p - o)| over the beads staged by the tile"""
    g = g or grid_of(s)
    R, C, _ = staged_copies(s, g)
    out = {}
    for t in set(map(tuple, g.tile_of(positions(s)).tolist())):
        lo, hi = TC * np.array(t) - 2, TC * (np.array(t) + 1) + 2
        st = ((C >= lo) & (C < hi)).all(axis=1)
        out[t] = np.float32(np.abs((R[st] - g.tile_centre(t)).astype(np.float32)).max())
    return out


def _fma32(a, b, c):
    """fma(a, b, c) on float32 arrays: the exact float64 product, the sum rounded to float64 and then to float32 (the double rounding
    can differ from the true fma by one float32 ulp: staged_error returns that slack)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def staged_r2(s, g, I, J):
    """the device's single-precision r^2 of the ordered pairs (I, J), as bead I's lane forms it: both beads staged relative to the centre of
    I's tile, the partner at its image nearest to I (formed as p + k L in double, as k_halo_update does), three float subtractions,
    fma(z, z, fma(y, y, x * x)).  Returns (r2 float32, the exact r^2 of the same two double positions as a longdouble, tiles of I)"""
    r = positions(s)
    per = np.array([(s.pbc >> a) & 1 for a in range(3)], float)
    pi, pj = r[I], r[J]
    k = np.rint((pi - pj) / g.L) * per
    pj = pj + k * g.L
    tiles = g.tile_of(pi)
    o = g.lo + (TC * tiles - g.m + 0.5 * TC) / g.cinv
    fi, fj = (pi - o).astype(np.float32), (pj - o).astype(np.float32)
    d = fi - fj
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r2 = _fma32(z, z, _fma32(y, y, (x.astype(np.float64) * x.astype(np.float64)).astype(np.float32)))
    dd = np.asarray(pi, np.longdouble) - np.asarray(pj, np.longdouble)
    return r2, (dd * dd).sum(axis=1), tiles


def staged_error(s, I, J):
    """for the ordered pairs (I, J): (|r2_f32 - r2_exact| / rl2, band / 4 of I's tile, the slack of the emulation -- one float32 ulp of r^2 / rl2,
    r2_f32, rl2_lo, rl2_hi)"""
    g = grid_of(s)
    am = tile_amax(s, g)
    r2, ex, tiles = staged_r2(s, g, I, J)
    rl, rl2 = rlist_of(s), rl2_of(s)
    b = np.array([band_of(rl, am[tuple(t)]) for t in tiles.tolist()])
    err = np.abs(np.asarray(r2, np.longdouble) - ex).astype(np.float64) / rl2
    return err, b[:, 0] / 4.0, float(np.spacing(np.float32(rl2))) / rl2, r2, b[:, 1].astype(np.float32), b[:, 2].astype(np.float32)


def reference_list(s, dtype=np.longdouble, near=None):
    """every ordered pair (i, j), i != j, with d^2 < rl2 under the minimum image, in `dtype`: a set of (i, j).  near (a dict) receives
    "I", "J", "x" = d^2 / rl2 - 1 of the ordered pairs within 2.1e-3 of the list radius"""
    r = np.asarray(positions(s), dtype)
    box = np.asarray(box_of(s), dtype)
    per = np.array([(s.pbc >> a) & 1 for a in range(3)], dtype)
    rl2 = dtype(rl2_of(s))
    out, nI, nJ, nx = set(), [], [], []
    for i0 in range(0, len(r), 400):
        d = r[i0:i0 + 400, None, :] - r[None, :, :]
        d -= box * per * np.rint(d / box)
        x = (d * d).sum(axis=2) / rl2 - 1
        ii, jj = np.nonzero(x < 0)
        keep = ii + i0 != jj
        out.update(zip((ii[keep] + i0).tolist(), jj[keep].tolist()))
        ii, jj = np.nonzero(np.abs(x) < 2.1e-3)
        nI.append(ii + i0); nJ.append(jj); nx.append(x[ii, jj])
    if near is not None:
        near["I"], near["J"], near["x"] = np.concatenate(nI), np.concatenate(nJ), np.concatenate(nx)
    return out


def near_pairs(s):
    """the ordered pairs within 2.1e-3 of the list radius (found in float64), their x = d^2 / rl2 - 1 in longdouble: (I, J, x)"""
    near = {}
    reference_list(s, np.float64, near)
    I, J = near["I"], near["J"]
    ld = np.longdouble
    r, box = np.asarray(positions(s), ld), np.asarray(box_of(s), ld)
    per = np.array([(s.pbc >> a) & 1 for a in range(3)], ld)
    d = r[I] - r[J]
    d -= box * per * np.rint(d / box)
    return I, J, (d * d).sum(axis=1) / ld(rl2_of(s)) - 1


def ambiguous(x):
    """how many of the values x = d^2 / rl2 - 1 lie inside the ambiguity floor"""
    return int((np.abs(np.asarray(x, np.longdouble)) < AMBIGUITY).sum())


def foreign_distance(s):
    """the smallest distance (internal units) between a bead and a bead of another site, under the minimum image"""
    r, box = positions(s), box_of(s)
    per = np.array([(s.pbc >> a) & 1 for a in range(3)], float)
    site = np.asarray(s.site)
    best = np.inf
    for i0 in range(0, len(r), 400):
        d = r[i0:i0 + 400, None, :] - r[None, :, :]
        d -= box * per * np.rint(d / box)
        d2 = (d * d).sum(axis=2)
        d2[site[i0:i0 + 400, None] == site[None, :]] = np.inf
        best = min(best, float(np.sqrt(d2.min())))
    return best


def cell_offsets(s, g=None):
    """owned-cell offset of the partner from the first bead for every labelled pair, the partner taken at its nearest image: (npair, 3)"""
    g = g or grid_of(s)
    r = positions(s)
    per = np.array([(s.pbc >> a) & 1 for a in range(3)], float)
    pi, pj = r[s.pair_i], r[s.pair_j]
    pj = pj + np.rint((pi - pj) / g.L) * per * g.L
    return g.raw_cell(pj) - g.owned_cell(pi)


def _mol_forcefield(s):
    """a third molecule type of two species (atoms 0 and 1, one bonded pair): declared like the types of tests/molecule_systems.py"""
    s.nspecies = 4
    s.species_name = list(s.species_name) + ["Mx0000", "Mx0001"]
    s.mass = np.full(4, float(s.mass[0]))
    s.charge = np.zeros(4)
    s.ljtype = np.array([1, 0, 1, 1], np.int32)
    s.moltype = s.resitype = np.array([0, 1, 2, 2], np.int32)
    s.atomoffset = np.array([0, 0, 0, 1], np.int32)
    s.nmoltype = s.nresi = 3
    s.mol_nspecies = s.resi_natoms = np.array([1, 1, 2], np.int32)
    s.bpair_off = np.array([0, 0, 0, 1], np.int32)
    s.bpairI, s.bpairJ = np.array([0], np.int32), np.array([1], np.int32)
    s.bond_off = s.angle_off = s.tors_off = s.cons_off = np.zeros(4, np.int32)


class _Builder(object):
    def __init__(self, box_A, pbc, variant, scale=1.0):
        self.s = Setup()
        water_forcefield(self.s, RCUT_A, SKIN_A)
        self.variant = variant
        if variant == "mol":
            _mol_forcefield(self.s)
        self.rlist = rlist_of(self.s)
        self.L = np.array(box_A, float) * ANG * scale
        self.g = Grid(self.L, pbc, self.rlist)
        self.pbc = pbc
        self.ns = np.maximum(np.floor(np.array(box_A) / SITE_A).astype(int), 1)
        self.sp = self.L / self.ns
        self.free = [c for c in itertools.product(*(range(n) for n in self.ns[::-1]))]      # (k, j, i), x fastest
        self.free = [(i, j, k) for k, j, i in self.free]
        self.taken = set()
        self.r, self.site, self.sp_of, self.mol = [], [], [], []
        self.pairs = []
        self.nsite = 0

    def centre(self, c):
        return (np.array(c) + 0.5) * self.sp - 0.5 * self.L

    def take(self, c=None):
        if c is None:
            c = next(q for q in self.free if q not in self.taken)
        assert c not in self.taken, c
        self.taken.add(c)
        return c

    def pair(self, p1, u, d, family, e=0.0, direction="", tag="", species=(0, 0)):
        """beads at p1 and p1 + d u (internal units); returns the pair's number"""
        k = self.nsite
        self.nsite += 1
        i = len(self.r)
        p2 = p1 + d * u
        mol = self.variant == "mol"
        self.r += [p1, p2]
        self.site += [k, k]
        self.sp_of += [2, 2] if mol else list(species)
        self.mol += [i, i + 1]
        if mol:
            # atom 1 of each probe's molecule, 5 A off the axis (16.8 A from the other probe: outside the list radius)
            w = np.cross(u, [0.0, 0.0, 1.0]) if abs(u[2]) < 0.9 else np.cross(u, [1.0, 0.0, 0.0])
            w /= np.sqrt((w * w).sum())
            self.r += [p1 + 5.0 * ANG * w, p2 - 5.0 * ANG * w]
            self.site += [k, k]
            self.sp_of += [3, 3]
            self.mol += [i, i + 1]
        self.pairs.append((i, i + 1, family, e, direction, tag))
        return len(self.pairs) - 1

    def centred(self, c, u, d, family, **kw):
        return self.pair(c - 0.5 * d * u, u, d, family, **kw)

    def finish(self):
        s, g = self.s, self.g
        r = np.array(self.r)
        for a in range(3):          # back_in_box (ddcmi.hip)
            if (self.pbc >> a) & 1:
                r[r[:, a] > 0.5 * g.L[a], a] -= g.L[a]
                r[r[:, a] < -0.5 * g.L[a], a] += g.L[a]
        s.h = np.array([g.L[0], 0, 0, 0, g.L[1], 0, 0, 0, g.L[2]])
        s.pbc = self.pbc
        s.natoms = len(r)
        s.rx, s.ry, s.rz = (np.ascontiguousarray(r[:, c]) for c in range(3))
        s.vx, s.vy, s.vz = (np.zeros(s.natoms) for _ in range(3))
        s.species = np.array(self.sp_of, np.int32)
        s.group = np.zeros(s.natoms, np.int32)
        idx = np.arange(s.natoms, dtype=np.uint64)
        if self.variant == "mol":
            s.gid = (np.array(self.mol, np.uint64) << np.uint64(32)) | (s.species == 3).astype(np.uint64)
            s.nmol = len(set(self.mol))
        else:
            s.gid = idx << np.uint64(32)
            s.nmol = 0
        s.site = np.array(self.site)
        if self.variant == "types20":
            s = relabel_types(s, 20)
        s.pair_i, s.pair_j = (np.array([p[q] for p in self.pairs]) for q in (0, 1))
        s.pair_family, s.pair_dir, s.pair_tag = (np.array([p[q] for p in self.pairs]) for q in (2, 4, 5))
        s.pair_e = np.array([p[3] for p in self.pairs])
        s.variant = self.variant
        return s


def _add_inner(b):
    for q, d in enumerate((5.2, 7.9, 10.3, 11.99, 12.01, 13.7)):
        b.centred(b.centre(b.take()), DIRECTIONS[(3 * q + 8) % 9], d * ANG, "inner", direction=DIR_NAMES[(3 * q + 8) % 9], species=(0, q % 2))


def _add_sweep(b, evalues):
    for e in evalues:
        for sign in (1, -1):
            for q, u in enumerate(DIRECTIONS):
                b.centred(b.centre(b.take()), u, b.rlist * (1.0 + sign * e), "sweep", e=sign * e, direction=DIR_NAMES[q])


def _add_band(b):
    # placed at the list radius; _set_band moves the partner once the tile's amax is known
    for q, u in enumerate(DIRECTIONS):
        for k, tag in enumerate(("lo*1.1", "lo*0.9", "hi*0.9", "hi*1.1")):
            off = 0.25 * ANG * np.array([k, 3 - k, 2 * k - 3])      # four different places in the cell
            b.centred(b.centre(b.take()) + off, u, b.rlist, "band", direction=DIR_NAMES[q], tag=tag)


def _set_band(s):
    """d^2 = rl2 (1 +- band (1 +- 0.1)) for the band pairs, band from the first bead's tile"""
    g = grid_of(s)
    am = tile_amax(s, g)
    r = positions(s)
    rl = rlist_of(s)
    e_of = {"lo*1.1": (-1, 1.1), "lo*0.9": (-1, 0.9), "hi*0.9": (1, 0.9), "hi*1.1": (1, 1.1)}
    for q in np.flatnonzero(s.pair_family == "band"):
        i, j = s.pair_i[q], s.pair_j[q]
        band = band_of(rl, am[tuple(g.tile_of(r[i]).tolist())])[0]
        sign, f = e_of[str(s.pair_tag[q])]
        u = DIRECTIONS[DIR_NAMES.index(str(s.pair_dir[q]))]
        d = rl * np.sqrt(1.0 + sign * f * band)
        moved = r[i] + d * u
        if s.variant == "mol":
            r[j + 2] += moved - r[j]          # the partner's molecule moves with it (beads i, j, then atom 1 of each)
        r[j] = moved
        s.pair_e[q] = d / rl - 1.0
    s.rx, s.ry, s.rz = (np.ascontiguousarray(r[:, c]) for c in range(3))


def _add_adverse(b, nsites=40, tries=300, seed=7):
    """pairs at e = +-3e-8 whose single-precision r^2 lies on the WRONG side of the list radius, as far as a search over places in the site
    and directions finds (a fixed seed; the emulation of staged_r2 with the pair's own largest coordinate for amax): a band narrower than
    the error bound it is derived from takes or rejects them unseen"""
    rng = np.random.RandomState(seed)
    g, rl = b.g, b.rlist
    rl2 = rl * rl
    for k in range(nsites):
        cen = b.centre(b.take())
        e = 3e-8 if k % 2 == 0 else -3e-8
        d = rl * (1.0 + e)
        best = None
        for _ in range(tries):
            c = cen + rng.uniform(-4.0, 4.0, 3) * ANG
            u = rng.normal(size=3)
            u /= np.sqrt((u * u).sum())
            p1, p2 = c - 0.5 * d * u, c + 0.5 * d * u
            o = g.tile_centre(g.tile_of(p1))
            fi, fj = (p1 - o).astype(np.float32), (p2 - o).astype(np.float32)
            x, y, z = (fi - fj)
            r2 = _fma32(z, z, _fma32(y, y, np.float32(np.float64(x) * np.float64(x))))
            wrong = -np.sign(e) * (float(r2) / rl2 - 1.0)
            score = wrong / band_of(rl, max(np.abs(fi).max(), np.abs(fj).max()))[0]
            if best is None or score > best[0]:
                best = (score, p1, u)
        b.pair(best[1], best[2], d, "adverse", e=e, direction="searched")


def _add_face(b):
    """across each periodic face, between two layers of sites (SITE_A / 2 from both): along the normal and along a diagonal"""
    col = 0
    for a in range(3):
        if not (b.pbc >> a) & 1:
            continue
        for e in (1e-10, -1e-10, 1e-7, -1e-7, 3e-6, -3e-6):
            c = b.centre((col % b.ns[0], (col // b.ns[0]) % b.ns[1], col % b.ns[2]))
            col += 1
            c[a] = -0.5 * b.L[a]
            u = np.eye(3)[a] if abs(e) != 1e-7 else DIRECTIONS[7]
            b.centred(c, u, b.rlist * (1.0 + e), "face", e=e, direction="xyz"[a] if abs(e) != 1e-7 else "xyz", tag="axis %d" % a)


def _add_domain(b):
    """across the mid planes.  Sites of the middle layer of each axis (an odd number of sites per axis); "on": the partner's coordinate
    on the axis is exactly 0.0, or the first double on either side of it that is not denormal-small (+-1e-13)"""
    mid = b.ns // 2
    assert all(n % 2 == 1 for n in b.ns)
    row = 0
    for a in range(3):
        for e, on in ((1e-10, None), (-1e-10, None), (1e-7, None), (-1e-7, None), (1e-7, 0.0), (-1e-7, 0.0), (-1e-7, 1e-13), (-1e-7, -1e-13)):
            q = row % 8
            c = [0, 0, 0]
            c[a], c[(a + 1) % 3], c[(a + 2) % 3] = mid[a], q % b.ns[(a + 1) % 3], q // b.ns[(a + 1) % 3] + 5
            row += 1
            cen = b.centre(b.take(tuple(c)))
            u = np.eye(3)[a] if row % 2 else DIRECTIONS[7]
            d = b.rlist * (1.0 + e)
            if on is None:
                b.centred(cen, u, d, "domain", e=e, direction="xyz"[a] if row % 2 else "xyz", tag="axis %d" % a)
            else:
                p2 = cen.copy()
                p2[a] = on
                b.pair(p2, -u, d, "domain", e=e, direction="xyz"[a] if row % 2 else "xyz", tag="axis %d on %g" % (a, on))


def _add_place(b):
    """one pair per interior tile, every second tile in x and every third in y and z: the first bead in a corner cell or the centre cell, 0.9 of a cell towards the
    outside; the partner along an outward axis or the outward body diagonal, two cells outside the tile"""
    g = b.g
    inner = [[t for t in range(g.T[a]) if TC[a] * t - 2 >= g.m[a] and TC[a] * (t + 1) + 2 <= g.m[a] + g.n[a]][::(2 if a == 0 else 3)] for a in range(3)]
    slots = list(itertools.product(*inner))
    cells = [tuple(np.array(c) * (TC - 1)) for c in itertools.product((0, 1), repeat=3)] + [tuple(TC // 2)]
    k = 0
    for loc in cells:
        out = np.array([1.0 if 2 * loc[a] >= TC[a] else -1.0 for a in range(3)])
        for dname, u in (("x", out * [1, 0, 0]), ("y", out * [0, 1, 0]), ("z", out * [0, 0, 1]), ("xyz", out / np.sqrt(3.0))):
            for e in (1e-7, -1e-7):
                t = np.array(slots[k]); k += 1
                frac = 0.5 + 0.4 * out
                p1 = g.lo + (TC * t - g.m + np.array(loc) + frac) / g.cinv
                b.pair(p1, u, b.rlist * (1.0 + e), "place", e=e, direction=dname, tag="cell %d%d%d" % loc)


def _add_prune(b):
    g = b.g
    e = 1e-7
    for a in range(3):
        for hi in (0, 1):
            for sign in (1, -1):
                for nudge in (-1, 0, 1):
                    cen = b.centre(b.take())
                    c = g.owned_cell(cen)
                    p1 = g.lo + (c + 0.37) / g.cinv
                    x = g.face(a, c[a] + hi)
                    p1[a] = x if nudge == 0 else np.nextafter(x, nudge * np.inf)
                    b.pair(p1, sign * np.eye(3)[a], b.rlist * (1.0 - e), "prune", e=-e, direction=("+" if sign > 0 else "-") + "xyz"[a],
                           tag="%s face %+d ulp" % ("high" if hi else "low", nudge))
    # corner beads: partner at (+-2, +-1, +-1) cells in every order of the axes.  A + sign: the bead one ulp below the high face of its cell,
    # a - sign: on the low face.  The long component takes what rlist (1 - e) leaves of two short ones of 0.16 cell
    for a in range(3):
        for sg in itertools.product((1, -1), repeat=3):
            cen = b.centre(b.take())
            c = g.owned_cell(cen)
            p1 = np.array([np.nextafter(g.face(q, c[q] + 1), -np.inf) if sg[q] > 0 else g.face(q, c[q]) for q in range(3)])
            d = b.rlist * (1.0 - e)
            v = np.array([0.16 / g.cinv[q] for q in range(3)])
            v[a] = np.sqrt(d * d - sum(v[q] ** 2 for q in range(3) if q != a))
            v *= np.array(sg)
            b.pair(p1, v / np.sqrt((v * v).sum()), d, "prune", e=-e, direction="2 on %s %+d%+d%+d" % (("xyz"[a],) + sg), tag="corner")


FACE_CELL_IN_A = 6.0            # facecell: how far inside the face the partner lies (a cell is 8.04 A wide)


def _add_facecell(b):
    """halo_cell's side forcing.  The box is chosen so that `floor((r - lo) * cinv)` puts a bead that lies exactly ON the high face of the
    box, or of the low domain of a 2-way split, into the LAST INTERIOR cell n - 1 (the product W * (n / W) rounds below n: the host test
    asserts it); only the forcing moves it out to the margin.  First bead exactly on the low face of the box (its image lies on the high
    face) or on the mid plane (the low domain receives it on its high face); the partner at rlist (1 - 1e-7) from that image, on the inner
    side of the face; and a third bead of the site (Setup.face_third) FACE_CELL_IN_A straight inside the face, so that cell n - 1 holds an
    OWNED bead as well: k_merge_cells gives a cell with owned beads the owned range alone, and an image filed there is lost to every row"""
    e = -1e-7
    d = b.rlist * (1.0 + e)
    q = 1
    b.third = []
    for where, tag in ((None, "periodic"), (0.0, "mid")):
        for a in range(3):
            p1 = b.centre(b.take((q, q, q)))          # a site of its own in every layer of every axis
            q += 1
            p1[a] = -0.5 * b.L[a] if where is None else where
            u = np.zeros(3)
            u[a] = -0.5 * FACE_CELL_IN_A * ANG / d
            u[(a + 1) % 3] = np.sqrt(1.0 - u[a] * u[a])
            k = b.pair(p1, u, d, "facecell", e=e, direction="xyz"[(a + 1) % 3], tag="%s axis %d" % (tag, a))
            b.third.append(len(b.r))
            b.r.append(p1 - FACE_CELL_IN_A * ANG * np.eye(3)[a])
            b.site.append(b.site[b.pairs[k][0]]); b.sp_of.append(0); b.mol.append(len(b.r) - 1)


def _add_outside(b):
    """open axes: a pair centred 3 rlist beyond the high face, one 3 rlist below the low face, one 1000 A beyond the high face"""
    col = 0
    for a in range(3):
        if (b.pbc >> a) & 1:
            continue
        for where, tag in ((0.5 * b.L[a] + 3.0 * b.rlist, "3 rlist above"), (-0.5 * b.L[a] - 3.0 * b.rlist, "3 rlist below"),
                           (0.5 * b.L[a] + 1000.0 * ANG, "1000 A above")):
            for e, u in ((1e-7, np.eye(3)[a]), (-1e-7, np.eye(3)[a]), (3e-6, DIRECTIONS[8]), (-3e-6, DIRECTIONS[8])):
                c = b.centre(((col + 1) % b.ns[0], (col // 2 + 2) % b.ns[1], (col + 3) % b.ns[2]))
                col += 1
                c[a] = where
                b.centred(c, u, b.rlist * (1.0 + e), "outside", e=e, direction="xyz"[a] if abs(e) == 1e-7 else "generic", tag=tag)


def gas(name, variant="one_type"):
    """the probe gas `name` of GAS (module docstring)"""
    cfg = GAS[name]
    b = _Builder(cfg["box_A"], cfg["pbc"], variant, cfg.get("scale", 1.0))
    fam = cfg["families"]
    if "domain" in fam:
        _add_domain(b)
    if "inner" in fam:
        _add_inner(b)
    if "sweep" in fam:
        _add_sweep(b, E_VALUES)
    if "sweep_short" in fam:
        _add_sweep(b, E_SHORT)
    if "band" in fam:
        _add_band(b)
    if "adverse" in fam:
        _add_adverse(b)
    if "prune" in fam:
        _add_prune(b)
    if "place" in fam:
        _add_place(b)
    if "face" in fam:
        _add_face(b)
    if "outside" in fam:
        _add_outside(b)
    if "facecell" in fam:
        _add_facecell(b)
    s = b.finish()
    if "band" in fam:
        _set_band(s)
    if "facecell" in fam:
        s.face_third = np.array(b.third)
    s.name = name
    return s


def crowded():
    """the "prune_fold" style small gas plus a clump of 8 x 8 x 7 beads 3.5 A apart at a free site: rows of up to 447 entries where the build
    starts with 24 words, a neighbourhood of more than 448 staged beads where it starts with room for 384"""
    b = _Builder((400.0, 400.0, 400.0), 7, "one_type")
    _add_inner(b)
    _add_sweep(b, E_SHORT)
    k = b.nsite
    b.nsite += 1
    c = b.centre(b.take())
    for iz in range(7):
        for iy in range(8):
            for ix in range(8):
                b.r.append(c + 3.5 * ANG * (np.array([ix, iy, iz]) - 3.5) + 0.01 * ANG * np.array([iy, iz, ix]))
                b.site.append(k); b.sp_of.append(0); b.mol.append(len(b.r) - 1)
    s = b.finish()
    s.name = "crowded"
    return s


def nudged_water(seed=20260, npick=2000):
    """make_water_setup(12) with up to npick beads moved along the line to a chosen neighbour until their distance is rlist (1 + e), e drawn from
    +-E_VALUES in turn; neither bead of such a pair is touched again.  Setup.pair_i, pair_j, pair_e label the nudged pairs"""
    s = make_water_setup(12)
    r, box = positions(s), box_of(s)
    rl = rlist_of(s)
    rng = np.random.RandomState(seed)
    used = np.zeros(s.natoms, bool)
    evals = [sg * e for e in E_VALUES for sg in (1, -1)]
    pi, pj, pe = [], [], []
    for i in rng.permutation(s.natoms):
        if len(pi) >= npick:
            break
        if used[i]:
            continue
        d = r - r[i]
        d -= box * np.rint(d / box)
        dist = np.sqrt((d * d).sum(axis=1))
        cand = np.flatnonzero(~used & (np.abs(dist - rl) < 1.0 * ANG))
        cand = cand[cand != i]
        if cand.size == 0:
            continue
        j = int(cand[rng.randint(cand.size)])
        e = evals[len(pi) % len(evals)]
        r[i] = (r[i] + d[j]) - (d[j] / dist[j]) * rl * (1.0 + e)
        used[i] = used[j] = True
        pi.append(int(i)); pj.append(j); pe.append(e)
    r -= box * np.rint(r / box)
    s.rx, s.ry, s.rz = (np.ascontiguousarray(r[:, c]) for c in range(3))
    s.pair_i, s.pair_j, s.pair_e = np.array(pi), np.array(pj), np.array(pe)
    s.pair_family = np.array(["nudged"] * len(pi)); s.pair_dir = np.array([""] * len(pi)); s.pair_tag = np.array([""] * len(pi))
    s.name, s.variant, s.nmol = "nudged_water", "one_type", 0
    return s


def describe(s, pairs):
    """one line per ordered pair (i, j) of `pairs` for a failure report: family, e, direction, tag and cell offset of the labelled pair it belongs to"""
    g = grid_of(s)
    off = cell_offsets(s, g)
    label = {}
    for q in range(len(s.pair_i)):
        label[(int(s.pair_i[q]), int(s.pair_j[q]))] = label[(int(s.pair_j[q]), int(s.pair_i[q]))] = q
    out = []
    for i, j in sorted(pairs)[:40]:
        q = label.get((i, j))
        if q is None:
            out.append("(%d, %d): not a labelled pair" % (i, j))
        else:
            out.append("(%d, %d): %s e %+.3g dir %s %s cell offset %s" % (i, j, s.pair_family[q], s.pair_e[q], s.pair_dir[q], s.pair_tag[q], off[q].tolist()))
    return "\n".join(out)


_systems, _lists = {}, {}


def system(name, variant="one_type"):
    """gas(name, variant), crowded() or nudged_water(), made once"""
    key = (name, variant)
    if key not in _systems:
        _systems[key] = crowded() if name == "crowded" else nudged_water() if name == "nudged_water" else gas(name, variant)
    return _systems[key]


def exact_list(name, variant="one_type"):
    """the reference list of system(name, variant), made once: longdouble for the gas, float64 for the water box (whose pairs near the list
    radius the host test holds against longdouble); variant "mol": without the molecules' own pairs"""
    key = (name, variant)
    if key not in _lists:
        s = system(name, variant)
        ref = reference_list(s, np.float64 if name == "nudged_water" else np.longdouble)
        if variant == "mol":          # the list keeps no bonded pair of a molecule (reOrgPairs): atom 0 - atom 1 go to the excluded list
            mol = (np.asarray(s.gid, np.uint64) >> np.uint64(32)).tolist()
            ref = {(i, j) for i, j in ref if mol[i] != mol[j]}
        _lists[key] = ref
    return _lists[key]


def excluded_pairs(s):
    """unordered pairs of one molecule inside the list radius: the molecules' atom 0 - atom 1 pairs (5 A)"""
    return int(getattr(s, "nmol", 0))

"""Tiles of chosen occupancy for the pair kernel's lane splits and row parts (helper module, no tests in here).

k_nonbond (ddcmi_nonbond.inl) gives a bead 1, 2, 4 ... 64 lanes that share its neighbour row, by the number of rows its work item walks:
a tile's owned beads, or -- for the items schedule_tiles cuts at the tail of a launch -- one of 2, 3, 4, 6 or 8 row ranges of them.  In a
water box or a bilayer neither number is a test's choice.  `make_split_setup(variant)` is a box of 4 x 4 x 4 tiles (8 x 4 x 4 cells of 8.2 A
each; with the margin of image tiles the grid has 6 x 6 x 6) in which 23 tiles own exactly

    1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 600

beads and the other 41 none.  DDCMI_DEBUG_HOOKS=1 DDCMI_DEBUG_TAIL=k then cuts every one of them into k parts, and ddcmi_debug_tile_items
(include/ddcmi_test.h) returns what was launched.

Geometry, the same for every variant: a tile holds a 14 x 7 x 7 lattice of sites 4.686 A apart (686 sites), each moved by up to 0.3 A per
axis (splitmix64 hashes: the same inputs on every machine); no site is closer than 1.4 A to a face of its tile, so the tile of a bead does not
hang on a rounding.  The seven tiles of 255 and more beads take a hashed subset of their sites and sit apart from each other; each of the
sixteen smaller ones shares a face with one of them and takes the sites nearest to the centre of that face, so even the one bead of the
1-bead tile has partners.  Tiles lie on periodic faces, edges and a corner of the box (their partners are shifted copies: tshift tiles, the
virial booked per pair) and in its interior (no image staged).  The beads interact weakly -- sigma = 3.0 / 3.2 A under a nearest distance of
4.09 A, every pair on the attractive side of its minimum -- so 600 beads in a tile are no explosion and no pair force vanishes.

Variants (what they make of the kernel's template parameters):
  one_type      two uncharged LJ types, 2 classes                      packed entries, the shifted-copy bit in the entry
  charged_mol   10 (LJ type, charge) classes, charges 0, +-0.05, +-0.1, half of the beads in molecules of 3 and 6 whose pairs are all
                excluded: HAS_Q, the excluded walk of the sub == 0 lane (6-bead molecules: a fifth partner behind the four the walk
                prefetches).  More than 8 classes: bare entries, class and shifted-copy flag in the staged z.  The charges are small
                on purpose: the reaction-field force kq (1 / r^2 - r / rc^3) of two like charges opposes the LJ attraction and falls
                to zero at the cut-off, so with Martini's unit charges every like pair has a distance at which its force vanishes and
                some of 70 000 pairs sit there; with |q_i q_j| <= 0.01 it stays below 0.45 of the LJ force everywhere beyond 4.09 A
  types20       the first under 20 LJ types (relabel_types)            bare entries, tags in the staged z

`split_plan` restates the kernel's arithmetic (the formulas, nothing else of it).  `reference` is every pair in numpy.longdouble under the
minimum image, written from the force field's formulas as tests/closed_forms.py cites them (lj_rf_pair_E, lj_rf_pair_F: martiniNonBond,
bioMartini.c:1063-1090) with the reaction-field-only term kq (krf r^2 - crf) for excluded pairs (martiniIntraMoleReaction) and the self term
-1/2 sum q^2 keR crf in `ele` (bioMartini.c:1030-1035); nothing of it comes from oracle/ or from the device code."""
import numpy as np

from ddcmd_amd.deck import Setup, units_convert
from ddcmd_amd.synth import water_forcefield, relabel_types, lj_shift, splitmix64, _uniform

TCX, TCY, TCZ = 8, 4, 4         # ddcmi_internal.h: cells of a tile
NB_WAVES = 8                    # ddcmi_internal.h: NB_THREADS 512 / 64
CELL_A = 8.2                    # cell width (A): floor(L / (rlist / 2)) = floor(L / 8 A) gives exactly 32 / 16 / 16 cells
NTILE = 4                       # owned tiles per axis
SITES = (14, 7, 7)              # sites of a tile, 4.686 A apart on every axis
SITE_OFFSET = 0.37              # first site at 0.37 of the spacing from the tile's corner: 1.73 A (1.43 A with the jitter) from the low faces, 2.95 A from the high ones
JITTER_A = 0.3
SEED = 20261020
COUNTS = (1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 600)
NPARTS = (1, 2, 3, 4, 6, 8)     # what schedule_tiles cuts a tile into (ddcmi_rebuild.inl: const int parts[] = {2, 3, 4, 6, 8})
VARIANTS = ("one_type", "charged_mol", "types20")
SIGMA_A = (3.0, 3.2)            # like pairs / the mixed pair: minima at 3.37 / 3.59 A, the nearest two sites can come is 4.686 - 0.6 = 4.09 A
# the tiles of 255 and more beads: apart from each other (no two share a face), in the interior, on faces, an edge and a corner of the box
BIG = {(1, 1, 1): 600, (2, 2, 2): 512, (0, 0, 0): 513, (3, 1, 2): 511, (1, 3, 0): 257, (2, 0, 3): 256, (0, 2, 1): 255}
SMALL = tuple(c for c in COUNTS if c < 255)
DIRS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
ANG = units_convert(1.0, "Angstrom")


def tile_plan():
    """{owned tile (i, j, k), 0 <= i, j, k < 4: (beads, anchor)}: anchor None for a hashed subset of the sites, or the direction of the
    face (shared with a big tile, through the periodic boundary if need be) whose centre the tile's beads gather at"""
    plan = {t: (c, None) for t, c in BIG.items()}
    bigs = list(BIG)
    for q, c in enumerate(SMALL):
        for turn in range(len(bigs) * 6):
            b = bigs[(q + turn // 6) % len(bigs)]
            d = DIRS[(q + turn) % 6]
            t = tuple((b[a] + d[a]) % NTILE for a in range(3))
            if t not in plan:
                plan[t] = (c, tuple(-x for x in d))
                break
        else:
            raise AssertionError("no free tile next to a big one")
    return plan


def _tile_sites():
    """site coordinates (A) relative to the tile's low corner, [686, 3], x fastest"""
    nx, ny, nz = SITES
    a = np.arange(nx * ny * nz)
    idx = np.stack([a % nx, (a // nx) % ny, a // (nx * ny)], 1)
    size = np.array([TCX, TCY, TCZ]) * CELL_A
    return (idx + SITE_OFFSET) * (size / np.array(SITES)), size


def _geometry():
    """positions (A) of all beads, the owned tile (i, j, k) of each, tile after tile"""
    sites, size = _tile_sites()
    L = NTILE * size
    r, tile = [], []
    for t, (count, anchor) in sorted(tile_plan().items()):
        tnum = (t[2] * NTILE + t[1]) * NTILE + t[0]
        sid = np.arange(len(sites), dtype=np.uint64) + np.uint64(1000 * tnum)
        if anchor is None:
            order = np.argsort(splitmix64(np.uint64(SEED) ^ sid), kind="stable")
        else:
            centre = 0.5 * size * (1.0 + np.array(anchor))
            order = np.argsort(((sites - centre) ** 2).sum(axis=1), kind="stable")
        pick = np.sort(order[:count])
        jit = np.stack([JITTER_A * (2.0 * _uniform(SEED, sid[pick], 1 + c) - 1.0) for c in range(3)], 1)
        r.append(-0.5 * L + np.array(t) * size + sites[pick] + jit)
        tile += [t] * count
    return np.concatenate(r), np.array(tile), L


def _velocities(s, n):
    """Maxwell-Boltzmann at 50 K from hashes, as ddcmd_amd.synth draws them (the fused steps need velocities, nothing hangs on their values)"""
    idx = np.arange(n, dtype=np.uint64)
    sig_v = np.sqrt(units_convert(50.0, "K") / np.asarray(s.mass)[s.species])
    v = []
    for c in range(3):
        u1, u2 = 1.0 - _uniform(SEED + 1, idx, 10 + 2 * c), _uniform(SEED + 1, idx, 11 + 2 * c)
        v.append(sig_v * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    return v


CHARGES = (0.0, 0.1, -0.1, 0.05, -0.05)
MOL3 = dict(n=3, charge=(0.1, -0.1, 0.05), lj=(1, 0, 1))
MOL6 = dict(n=6, charge=(0.1, -0.05, 0.05, -0.1, 0.1, 0.0), lj=(1, 1, 0, 1, 0, 1))
MOL_SPAN_A = 11.0               # the beads of a molecule lie within this of each other: every excluded pair inside the 12 A cut-off


def _charged_species(s):
    """ten one-bead species, one per (LJ type, charge) class, then the atoms of the two molecule types (classes among those ten)"""
    names, charge, lj, moltype, offset, mol_nspecies, bpair_off, bI, bJ = [], [], [], [], [], [], [0], [], []
    for l in (0, 1):
        for q in CHARGES:
            names.append("S%d%+03dxS" % (l, int(round(100 * q)))); charge.append(q); lj.append(l); moltype.append(len(mol_nspecies)); offset.append(0)
            mol_nspecies.append(1); bpair_off.append(0)
    first = {}
    for name, mol in (("M3", MOL3), ("M6", MOL6)):
        first[name] = len(names)
        for a in range(mol["n"]):
            names.append("%sx%04X" % (name, a)); charge.append(mol["charge"][a]); lj.append(mol["lj"][a]); moltype.append(len(mol_nspecies)); offset.append(a)
        for a in range(mol["n"]):
            for b in range(a + 1, mol["n"]):
                bI.append(a); bJ.append(b)
        mol_nspecies.append(mol["n"]); bpair_off.append(len(bI))
    s.nspecies = len(names)
    s.species_name = names
    s.mass = np.full(s.nspecies, float(s.mass[0]))
    s.charge = np.array(charge)
    s.ljtype, s.moltype, s.atomoffset = (np.array(x, np.int32) for x in (lj, moltype, offset))
    s.resitype = s.moltype.copy()
    s.nmoltype = s.nresi = len(mol_nspecies)
    s.mol_nspecies = np.array(mol_nspecies, np.int32)
    s.resi_natoms = s.mol_nspecies.copy()
    s.bpair_off, s.bpairI, s.bpairJ = (np.array(x, np.int32) for x in (bpair_off, bI, bJ))
    s.bond_off = s.angle_off = s.tors_off = s.cons_off = np.zeros(s.nresi + 1, np.int32)
    return first


def _label_charged(s, r_A, tile):
    """species and gid of every bead: in each tile, bead after bead, a bead not yet in a molecule starts one of 3 (the first bead of a tile of 3
    or more, then one bead in eight) or 6 (the next free bead of a tile of 6 or more, then one in sixteen) with the nearest free beads of its
    tile, if they all lie within MOL_SPAN_A of each other; everybody else is a single bead of a hashed class"""
    first = _charged_species(s)
    n = len(r_A)
    species = (splitmix64(np.uint64(SEED + 7) ^ np.arange(n, dtype=np.uint64)) % np.uint64(10)).astype(np.int32)
    gid = np.arange(n, dtype=np.uint64) << np.uint64(32)
    mol_of = np.full(n, -1, np.int64)
    draw = splitmix64(np.uint64(SEED + 11) ^ np.arange(n, dtype=np.uint64)) % np.uint64(16)
    nmol = 0
    for t in sorted(set(map(tuple, tile))):
        beads = np.flatnonzero((tile == np.array(t)).all(axis=1))
        made = {3: 0, 6: 0}
        for i in beads:
            if mol_of[i] >= 0:
                continue
            free = beads[mol_of[beads] < 0]
            size = 0
            if made[3] == 0 and len(beads) >= 3:
                size = 3
            elif made[6] == 0 and len(beads) >= 6:
                size = 6
            elif draw[i] == 0:
                size = 6
            elif draw[i] in (1, 2):
                size = 3
            if size == 0 or len(free) < size:
                continue
            d = np.sqrt(((r_A[free] - r_A[i]) ** 2).sum(axis=1))
            members = free[np.argsort(d, kind="stable")[:size]]
            span = np.sqrt(((r_A[members][:, None, :] - r_A[members][None, :, :]) ** 2).sum(axis=2)).max()
            if span >= MOL_SPAN_A:
                continue
            name = "M%d" % size
            for a, m in enumerate(members):
                species[m] = first[name] + a
                gid[m] = (np.uint64(n + nmol) << np.uint64(32)) | np.uint64(a)
                mol_of[m] = nmol
            made[size] += 1
            nmol += 1
    s.species, s.gid, s.mol_of = species, gid, mol_of


def make_split_setup(variant):
    """the box of the module docstring; the Setup carries for the tests: tile_ijk (owned tile of every bead, [n, 3]), plan (tile_plan()),
    variant, and for charged_mol mol_of (molecule number of every bead, -1: a single bead)"""
    assert variant in VARIANTS
    s = Setup()
    water_forcefield(s)
    sig = np.array([[SIGMA_A[0], SIGMA_A[1]], [SIGMA_A[1], SIGMA_A[0]]]) * ANG
    s.sigma = sig.ravel().copy()
    s.shift = lj_shift(s.sigma, s.eps, s.rmax)
    r_A, tile, L_A = _geometry()
    n = len(r_A)
    s.h = np.array([L_A[0], 0, 0, 0, L_A[1], 0, 0, 0, L_A[2]]) * ANG
    s.pbc = 7
    s.natoms = n
    s.rx, s.ry, s.rz = (np.ascontiguousarray(r_A[:, c] * ANG) for c in range(3))
    s.group = np.zeros(n, np.int32)
    if variant == "charged_mol":
        _label_charged(s, r_A, tile)
    else:
        s.species = (splitmix64(np.uint64(SEED + 3) ^ np.arange(n, dtype=np.uint64)) % np.uint64(4) == 0).astype(np.int32)      # a quarter of the other type
        s.gid = np.arange(n, dtype=np.uint64) << np.uint64(32)
    s.vx, s.vy, s.vz = _velocities(s, n)
    if variant == "types20":
        s = relabel_types(s, 20)
    s.tile_ijk, s.plan, s.variant = tile, tile_plan(), variant
    return s


# ---- the cell and tile assignment, restated from setup_grid (ddcmi_rebuild.inl) and cell_coords / cell_linear (ddcmi.hip)
def grid_of(s):
    """dict(n, m, T, cinv, lo) of a single periodic domain"""
    rlist = s.rmax + s.deltaR
    tdim = (TCX, TCY, TCZ)
    n, m, T, cinv, lo = [], [], [], [], []
    for a in range(3):
        W = float(s.h[4 * a])
        na = max(1, int(np.floor(W / (0.5 * rlist))))
        r = na % tdim[a]
        if r > 0 and 2 * r <= tdim[a] and na - r >= tdim[a] and na / (na - r) <= 1.02:
            na -= r
        periodic = (int(s.pbc) >> a) & 1
        ma = tdim[a] if periodic else 0
        n.append(na); m.append(ma); T.append((na + 2 * ma + tdim[a] - 1) // tdim[a]); cinv.append(na / W); lo.append(-0.5 * W)
    return dict(n=n, m=m, T=T, cinv=cinv, lo=lo)


def tile_of(s, r=None):
    """the device's tile number of every bead and its distance (internal units) from the nearest face of that tile"""
    g = grid_of(s)
    r = np.stack([s.rx, s.ry, s.rz], 1) if r is None else r
    tdim = (TCX, TCY, TCZ)
    tc, margin = [], []
    for a in range(3):
        u = (r[:, a] - g["lo"][a]) * g["cinv"][a]
        ic = np.clip(np.floor(u).astype(np.int64), 0, g["n"][a] - 1) + g["m"][a]
        tc.append(ic // tdim[a])
        v = (u + g["m"][a]) / tdim[a]
        margin.append(np.minimum(v - np.floor(v), np.ceil(v) - v) * tdim[a] / g["cinv"][a])
    return (tc[2] * g["T"][1] + tc[1]) * g["T"][0] + tc[0], np.min(margin, axis=0)


def device_tile(s, ijk):
    """tile number of the owned tile (i, j, k): one tile of margin on every periodic axis"""
    g = grid_of(s)
    off = [1 if g["m"][a] else 0 for a in range(3)]
    return ((ijk[2] + off[2]) * g["T"][1] + ijk[1] + off[1]) * g["T"][0] + ijk[0] + off[0]


def stages_images(ijk):
    """whether the neighbourhood of owned tile (i, j, k) -- the tile and two cells around it -- reaches into the margin of image cells"""
    return any(c == 0 or c == NTILE - 1 for c in ijk)


# ---- k_nonbond's split, restated (ddcmi_nonbond.inl: r_lo / r_hi, the row0 loop, R, nchunks, kb, parts)
def row_range(nown, part, nparts):
    return (nown * part) // nparts, (nown * (part + 1)) // nparts


def row_trips(nown, part, nparts):
    """trips through `for (row0 = r_lo; row0 < r_hi; row0 += 64 * NWAVES)`"""
    r_lo, r_hi = row_range(nown, part, nparts)
    return len(range(r_lo, r_hi, 64 * NB_WAVES))


def split_plan(nown, part, nparts):
    """the set of (R, parts, kb) an item walks: R rows per chunk, `parts` lanes per bead, kb beads in the chunk"""
    r_lo, r_hi = row_range(nown, part, nparts)
    out = set()
    for row0 in range(r_lo, r_hi, 64 * NB_WAVES):
        nhere = min(r_hi - row0, 64 * NB_WAVES)
        R = 64
        while R > 1 and (R >> 1) * NB_WAVES >= nhere:
            R >>= 1
        nchunks = (nhere + R - 1) // R
        for chunk in range(nchunks):
            kb = min(R, nhere - chunk * R)
            parts = 64 // R
            while parts * 2 * kb <= 64:
                parts *= 2
            out.add((R, parts, kb))
    return out


def plan_union(counts, nparts_list):
    """union of split_plan over tiles of `counts` beads cut into each of nparts_list"""
    out = set()
    for c in counts:
        for k in nparts_list:
            for p in range(k):
                out |= split_plan(c, p, k)
    return out


def decode_item(item):
    """(tile, part, nparts) of a work item as k_nonbond reads it"""
    return item & 0xffffff, (item >> 24) & 7, ((item >> 27) & 7) + 1


# ---- the reference
def excluded_mask(s, I, J):
    """pairs of one molecule of several species whose (atom, atom) is in the type's bonded-pair list (here: every pair of a molecule)"""
    gid = np.asarray(s.gid, np.uint64)
    ids, code = gid >> np.uint64(32), (gid & np.uint64(0xffff)).astype(np.int64)
    mt = np.asarray(s.moltype)[np.asarray(s.species)]
    out = np.zeros(I.size, bool)
    same = np.flatnonzero((ids[I] == ids[J]) & (I != J))
    if same.size == 0:
        return out
    bonded = [set(zip(s.bpairI[a:b].tolist(), s.bpairJ[a:b].tolist())) for a, b in zip(s.bpair_off[:-1], s.bpair_off[1:])]
    for k in same:
        i, j = I[k], J[k]
        out[k] = (code[i], code[j]) in bonded[mt[i]] or (code[j], code[i]) in bonded[mt[i]]
    return out


def reference(s):
    """every pair i < j inside the cut-off, numpy.longdouble, minimum image.  dict:
      f [n, 3]; lj, ele (with the self term); vir [6] = sum over pairs f_ij,a d_ij,b for ab = xx yy zz xy xz yz
      A [n] = sum_j |f_ij|; lj_abs, ele_abs = sum over pairs of |e_ij| (and the |self term|); vir_abs [6] = sum |f_ij,a d_ij,b|
      G [n] = sum_j of the largest singular value of d f_ij / d r (what a displaced partner moves the pair force by, per unit length),
      G_e = sum over pairs |f_ij|, G_vir = sum over pairs (G_ij |d_ij| + |f_ij|): energy / virial per unit of displacement
      npair, nexcl (pairs with a term), rel_gap = min |r / rmax - 1| over ALL pairs, fmin_rel = min over pairs with a term of |f_ij| / max(A_i, A_j)"""
    ld = np.longdouble
    n = s.natoms
    r = np.stack([np.asarray(s.rx, ld), np.asarray(s.ry, ld), np.asarray(s.rz, ld)], axis=1)
    box = np.array([s.h[0], s.h[4], s.h[8]], ld)
    spc = np.asarray(s.species)
    q = np.asarray(s.charge, ld)[spc]
    lj = np.asarray(s.ljtype)[spc]
    sig, eps, shift = (np.asarray(a, ld).reshape(s.nlj, s.nlj) for a in (s.sigma, s.eps, s.shift))
    keR, krf, crf, rc, rc2 = ld(s.keR), ld(s.krf), ld(s.crf), ld(s.rmax), ld(s.rmax) ** 2
    f, A, G = np.zeros((n, 3), ld), np.zeros(n, ld), np.zeros(n, ld)
    self_ele = -ld(0.5) * (q * q).sum() * keR * crf
    vlj, vele, vir = ld(0), self_ele, np.zeros(6, ld)
    lj_abs, ele_abs, vir_abs, G_e, G_vir = ld(0), abs(self_ele), np.zeros(6, ld), ld(0), ld(0)
    rel_gap, npair, nexcl = ld(1), 0, 0
    parts = []
    for i0 in range(0, n, 300):
        d = r[i0:i0 + 300, None, :] - r[None, :, :]
        d -= box * np.rint(d / box)
        r2 = (d * d).sum(axis=2)
        ii, jj = np.nonzero(r2 < rc2 * ld(1.21))
        up = ii + i0 < jj
        ii, jj = ii[up], jj[up]
        d, r2, I = d[ii, jj], r2[ii, jj], ii + i0
        if r2.size:
            rel_gap = min(rel_gap, np.abs(np.sqrt(r2) / rc - 1).min())
        cut = r2 < rc2
        I, jj, d, r2 = I[cut], jj[cut], d[cut], r2[cut]
        ex = excluded_mask(s, I, jj)
        keep = (~ex).astype(ld)
        kq = keR * q[I] * q[jj]
        sg, ep, sh = sig[lj[I], lj[jj]], eps[lj[I], lj[jj]], shift[lj[I], lj[jj]]
        rr = np.sqrt(r2)
        s6 = (sg / rr) ** 6
        e_lj = (4 * ep * (s6 * s6 - s6) + sh) * keep                                    # lj_rf_pair_E, the LJ part
        e_el = kq * (keep / rr + krf * r2 - crf)                                        # ... the reaction-field part; excluded: kq (krf r^2 - crf)
        # lj_rf_pair_F: -dV/dr = 24 eps (2 s12 - s6) / r + kq (1 / r^2 - 2 krf r); excluded pairs keep -2 kq krf r.  g = (-dV/dr) / r
        g = (24 * ep * (2 * s6 * s6 - s6) / r2 + kq / (r2 * rr)) * keep - 2 * kq * krf
        rdg = (24 * ep * (-28 * s6 * s6 + 8 * s6) / r2 - 3 * kq / (r2 * rr)) * keep      # r dg/dr
        fij = g[:, None] * d
        fabs = np.abs(g) * rr
        gij = np.maximum(np.abs(g), np.abs(g + rdg))          # d f / d d = g 1 + (r g') d d^T / r^2: eigenvalues g, g, g + r g'
        live = (keep > 0) | (kq != 0)
        npair += int((keep > 0).sum()); nexcl += int(((keep == 0) & (kq != 0)).sum())
        vlj += e_lj.sum(); vele += e_el.sum()
        lj_abs += np.abs(e_lj).sum(); ele_abs += np.abs(e_el).sum()
        np.add.at(f, I, fij); np.subtract.at(f, jj, fij)
        np.add.at(A, I, fabs); np.add.at(A, jj, fabs)
        np.add.at(G, I, gij); np.add.at(G, jj, gij)
        G_e += fabs.sum(); G_vir += (gij * rr + fabs).sum()
        for c, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            vir[c] += (fij[:, a] * d[:, b]).sum()
            vir_abs[c] += np.abs(fij[:, a] * d[:, b]).sum()
        parts.append((I[live], jj[live], fabs[live]))
    I, J, fabs = (np.concatenate(x) for x in zip(*parts))
    fmin_rel = (fabs / np.maximum(A[I], A[J])).min()
    return dict(f=f, lj=vlj, ele=vele, vir=vir, A=A, lj_abs=lj_abs, ele_abs=ele_abs, vir_abs=vir_abs, G=G, G_e=G_e, G_vir=G_vir,
                npair=npair, nexcl=nexcl, rel_gap=rel_gap, fmin_rel=fmin_rel)


def excluded_partners(s):
    """number of same-molecule partners of every bead (every pair of a molecule is in its type's list)"""
    mol = getattr(s, "mol_of", None)
    if mol is None:
        return np.zeros(s.natoms, np.int64)
    size = np.bincount(mol[mol >= 0])
    return np.where(mol >= 0, size[np.maximum(mol, 0)] - 1, 0)


_systems, _refs = {}, {}


def system(variant):
    """make_split_setup(variant), made once"""
    if variant not in _systems:
        _systems[variant] = make_split_setup(variant)
    return _systems[variant]


def system_reference(variant):
    """reference(system(variant)), made once and left unchanged"""
    if variant not in _refs:
        _refs[variant] = reference(system(variant))
    return _refs[variant]

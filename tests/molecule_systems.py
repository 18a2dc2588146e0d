"""Adversarial molecular systems for the list build's exclusion logic (helper module, no tests in here).

`make_molecule_setup(variant)` relabels the beads of the 4000-bead synthetic water box -- nobody is moved, so no pair is
closer than in water -- into molecules whose atom codes (gid & 0xffff = GROUP 8 | ATOM 8), bonded-pair lists and molecule
ids (gid bits 63:32) walk every escape of k_tile_build's compressed encodings:

  type A  12 atoms, codes 0..11                          the bonded-pair mask, as on the lipid deck (control)
  type B  70 atoms, codes 0..69, pairs with 63, 64, 69   a type whose mask cannot be used, beads on both sides of code 63
  type C  300 atoms, codes in many groups (0..0xffff)    6-bit image code -> 8-bit tag -> gid; bonded pairs across 63 / 255 / 256 /
                                                         0xffff and, next to each, a NON-pair whose codes alias under truncation
  type D  40 atoms, a hub bonded to 35 of them           more excluded partners than the 16 rows the build starts with (regrow);
                                                         mask type that also holds never-bonded atoms coded 63, 64, 255, 0x300
  type E  one species, 3 beads                           every same-molecule pair pruned: any confusion of two ids shows

A molecule is a compact brick of lattice cells (4 beads each) walked boustrophedon, so consecutive atoms are lattice
neighbours (5.7 - 12.8 A: inside the 16 A list radius, most inside the 12 A cut-off).  Copies straddle the periodic faces and
the mid planes of the box (the domain faces of 2-way decompositions); neighbouring copies are mirrored so that atoms with
BONDED CODES of DIFFERENT molecules face each other, and their ids collide in the compressed forms: equal low byte
(m, m + 256), equal low 16 bits (m + 2^16), equal low 24 bits (m + 2^24, m + 2^31: only the 32-bit confirmation tells them
apart), 0 and 0xffffffff, an id whose bits make the record's tag word a signalling NaN (0xfff0....), and a molecule whose id is
a neighbouring WATER bead's id + 2^24.  variant "narrow" keeps every id below 2^24 (the build then never confirms against
the 32-bit id) with the low-byte and low-16-bit collisions in place.

No bonded terms, no constraints: bpair_off / bpairI / bpairJ only define exclusions.  Molecule atoms carry charges
+1 / -1 / 0 so that the charged pair kernel runs and excluded pairs carry a reaction-field term.

`classify(s)` sorts, from the inputs alone, every ordered pair inside the list radius into the cases of the build's decision
ladder and returns the counts.  The end of the module holds what the CPU and the GPU tests share: the oracle's lists as sets
of pairs, and a brute-force reference independent of the oracle -- all pairs, numpy.longdouble, the pruning rule in five lines.

The two variants differ in molecule ids only; their oracle, reference and counts are made once per process."""
import ctypes

import numpy as np

from ddcmd_amd.synth import make_water_setup

N_LATTICE = 10          # 4 * 10^3 = 4000 beads
CHARGE_SCALE = 1.0      # (to be lowered if the oracle found the relabelled box unstable over 45 steps; it does not)


def _serpentine(dims, natoms, mirror):
    """cells of a dims = (dx, dy, dz) brick in boustrophedon order (consecutive cells share a face), 4 sites per cell"""
    dx, dy, dz = dims
    out = []
    row = 0
    for z in range(dz):
        for yy in range(dy):
            y = yy if z % 2 == 0 else dy - 1 - yy
            for xx in range(dx):
                x = xx if row % 2 == 0 else dx - 1 - xx
                for b in range(4):
                    out.append((dx - 1 - x if mirror else x, y, z, b))
            row += 1
    return out[:natoms]


def _type_A():
    codes = list(range(12))
    pairs = [(k, k + 1) for k in range(11)] + [(0, 2), (3, 5), (6, 8), (9, 11)]
    return dict(name="A", dims=(3, 1, 1), codes=codes, pairs=pairs)


def _type_B():
    # sequence order: 5, 69, 64, 63, 62 sit in neighbouring cells
    codes = [0, 1, 2, 3, 4, 5, 69, 64, 63, 62, 6, 7] + list(range(8, 62)) + [65, 66, 67, 68]
    pairs = [(k, k + 1) for k in range(62)] + [(k, k + 2) for k in range(60)] + [(62, 63), (63, 64), (5, 69), (64, 69)]
    return dict(name="B", dims=(3, 3, 2), codes=codes, pairs=pairs)


# type C: four cells in the middle of the walk hold the codes at the encodings' boundaries
C_HEAD = [7, 0x0107, 254, 62,
          3, 255, 256, 0x01ff,
          10, 63, 64, 0xffff,
          0xfffe, 257, 0x0200, 0x013f]
C_HEAD_PAIRS = [(3, 255), (255, 256), (254, 255), (10, 63), (63, 64), (62, 63), (255, 0xffff), (63, 255), (0xfffe, 0xffff),
                (257, 0x0200), (256, 257), (7, 254), (62, 254), (0x01ff, 0x0200), (64, 0x013f)]
# ... and these are NOT bonded although a truncated or saturated code of one side would make them a pair of the list above
C_DECOYS = [(3, 256), (3, 0x01ff), (3, 0xffff), (10, 64), (7, 0x0107), (254, 256), (62, 64), (63, 0xffff), (63, 0x013f), (63, 256),
            (255, 0xfffe), (256, 0xffff), (257, 0xffff), (254, 0xfffe), (0x0200, 0xffff), (64, 255), (10, 0x013f), (62, 0x013f)]


def _type_C():
    low = [c for c in range(62) if c not in (3, 7, 10)]          # 59 codes below 63
    nl = len(low)
    rest = []
    for i in range(nl):                                            # a low code next to codes of other groups with a neighbour's low byte
        rest += [low[i], ((2 + i % 3) << 8) | low[(i + 1) % nl], ((5 + i % 3) << 8) | low[i], ((8 + i % 3) << 8) | low[(i - 1) % nl]]
    for j in range(12):
        rest += [((0x40 + j) << 8) | b for b in (0, 63, 254, 255)]
    codes = rest[:12] + C_HEAD + rest[12:]
    # elastic network on the rest: every atom bonded to the three before and the three after it in the walk
    pairs = list(C_HEAD_PAIRS)
    for d in (1, 2, 3):
        pairs += [(rest[k], rest[k + d]) for k in range(len(rest) - d)]
    return dict(name="C", dims=(5, 5, 3), codes=codes, pairs=pairs)


def _type_D():
    codes = list(range(36)) + [63, 64, 255, 0x0300]               # the last four are bonded to nobody
    sites = np.array([(x + (0.5 if b in (1, 2) else 0.0), y + (0.5 if b in (1, 3) else 0.0), z + (0.5 if b in (2, 3) else 0.0))
                      for x, y, z, b in _serpentine((3, 2, 2), 40, False)])
    hub = int(np.argmin(((sites[:36] - sites.mean(axis=0)) ** 2).sum(axis=1)))
    pairs = [(hub, c) for c in range(36) if c != hub] + [(k, k + 1) for k in range(35) if hub not in (k, k + 1)]
    return dict(name="D", dims=(3, 2, 2), codes=codes, pairs=pairs, hub=hub)


def _type_E():
    return dict(name="E", dims=(1, 1, 1), codes=[0, 0, 0], pairs=[], one_species=True)


def molecule_types():
    return [_type_A(), _type_B(), _type_C(), _type_D(), _type_E()]


def water_collider(n=N_LATTICE):
    """lattice index of the water bead left in the cell (7, 0, 7) of the last E copy of the row (the fourth site of the cell); its
    molecule id is that index, and that E copy's id is it + 2^24 (wide) or + 2^16 (narrow)"""
    return ((7 * n + 0) * n + 7) * 4 + 3


def _copies(variant, n):
    """(type, origin cell, mirrored, molecule id) of every copy"""
    wide = variant == "wide"
    a, b, c, d, e = 0x5101, 0x6202, 0x012345, 0x7303, 0x8404
    w = water_collider(n)
    out = [("A", (0, 0, 2), False, a), ("A", (3, 0, 2), True, a + 256), ("A", (8, 9, 2), False, a + (1 << 16)),
           ("B", (4, 4, 9), False, b), ("B", (7, 4, 9), True, b + (1 << 16) if wide else b + 256),
           ("C", (3, 3, 4), False, c), ("C", (8, 3, 4), True, c + (1 << 24) if wide else c + 256),
           ("D", (4, 8, 4), False, d), ("D", (4, 0, 4), False, d + (1 << 31) if wide else d + (1 << 16))]
    e_ids = [e, e + 256, e + (1 << 16), e + (1 << 24), e + (1 << 31), 0xfff00000 | e] if wide else \
            [e, e + 256, e + (1 << 16), e + 512, e + (1 << 16) + 256, e + (2 << 16)]
    out += [("E", (k, 0, 7), False, m) for k, m in enumerate(e_ids)]
    out += [("E", (7, 0, 7), False, w + (1 << 24) if wide else w + (1 << 16)),
            ("E", (0, 0, 0), False, 0), ("E", (1, 0, 0), False, 0xffffffff if wide else 0xffffff)]
    return out


def make_molecule_setup(variant="wide"):
    """the relabelled water box; variant "wide": ids up to 0xffffffff, "narrow": every id below 2^24"""
    assert variant in ("wide", "narrow")
    n = N_LATTICE
    s = make_water_setup(n)
    types = {t["name"]: t for t in molecule_types()}
    order = ["A", "B", "C", "D", "E"]
    # species: the two of water, then one per atom of every type (one in all for the one-species type)
    names, charge, ljtype, moltype, atomoffset = list(s.species_name), [0.0, 0.0], [1, 0], [0, 1], [0, 0]
    mol_nspecies, bpair_off, bI, bJ = [1, 1], [0, 0, 0], [], []
    first_species = {}
    for mt, name in enumerate(order, start=2):
        t = types[name]
        codes = t["codes"]
        first_species[name] = len(names)
        if t.get("one_species"):
            names.append("%sx0000" % name); charge.append(-1.0 * CHARGE_SCALE); ljtype.append(1); moltype.append(mt); atomoffset.append(0)
            mol_nspecies.append(1)
        else:
            assert len(set(codes)) == len(codes) and max(codes) <= 0xffff, name
            rank = {c: k for k, c in enumerate(sorted(codes))}      # residues are sorted by gid: an atom's offset is the rank of its code
            for pos, c in enumerate(codes):
                names.append("%sx%04X" % (name, c))
                q = (1.0, -1.0, 0.0)[pos % 3]
                if pos == t.get("hub", -1):
                    q = 1.0
                charge.append(q * CHARGE_SCALE); ljtype.append(0 if pos % 7 == 3 else 1); moltype.append(mt); atomoffset.append(rank[c])
            mol_nspecies.append(len(codes))
            have = set(codes)
            seen = set()
            for i, j in t["pairs"]:
                assert i in have and j in have and i != j and (min(i, j), max(i, j)) not in seen, (name, i, j)
                seen.add((min(i, j), max(i, j)))
                bI.append(i); bJ.append(j)
        bpair_off.append(len(bI))
    s.nspecies = len(names)
    s.species_name = names
    s.mass = np.full(s.nspecies, float(s.mass[0]))
    s.charge = np.array(charge)
    s.ljtype, s.moltype, s.atomoffset = (np.array(x, np.int32) for x in (ljtype, moltype, atomoffset))
    s.resitype = s.moltype.copy()
    s.nmoltype = s.nresi = len(mol_nspecies)
    s.mol_nspecies = np.array(mol_nspecies, np.int32)
    s.resi_natoms = s.mol_nspecies.copy()
    s.bpair_off, s.bpairI, s.bpairJ = (np.array(x, np.int32) for x in (bpair_off, bI, bJ))
    s.bond_off = s.angle_off = s.tors_off = s.cons_off = np.zeros(s.nresi + 1, np.int32)
    # the beads
    species, gid = np.array(s.species, np.int32), np.array(s.gid, np.uint64)
    mol_kind = np.full(s.natoms, "W", dtype="U1")
    copy_of = np.full(s.natoms, -1, np.int64)
    taken = set()
    for k, (name, origin, mirror, molid) in enumerate(_copies(variant, n)):
        t = types[name]
        for pos, (x, y, z, b) in enumerate(_serpentine(t["dims"], len(t["codes"]), mirror)):
            idx = ((((origin[2] + z) % n) * n + (origin[1] + y) % n) * n + (origin[0] + x) % n) * 4 + b
            assert idx not in taken, (name, origin)
            taken.add(idx)
            one = bool(t.get("one_species"))
            species[idx] = first_species[name] + (0 if one else pos)
            resi = pos if one else 0                                # a one-species molecule is a run of one-atom residues
            gid[idx] = (np.uint64(molid) << np.uint64(32)) | np.uint64((resi << 16) | t["codes"][pos])
            mol_kind[idx] = name
            copy_of[idx] = k
    water = np.flatnonzero(copy_of < 0)
    ids = gid >> np.uint64(32)
    assert np.unique(gid).size == s.natoms
    assert not np.isin(ids[copy_of >= 0], ids[water]).any(), "a molecule's id is also a water bead's"
    if variant == "narrow":
        assert int(ids.max()) < (1 << 24)
    s.species, s.gid = species, gid
    s.mol_kind, s.copy_of = mol_kind, copy_of           # (for the tests: type letter and copy number of every bead, "W" / -1 = water)
    return s


def _bonded_keys(s):
    """per molecule type: sorted array of (code_i << 16 | code_j), both orders"""
    out = []
    for mt in range(s.nmoltype):
        sl = slice(int(s.bpair_off[mt]), int(s.bpair_off[mt + 1]))
        i, j = np.asarray(s.bpairI[sl], np.int64), np.asarray(s.bpairJ[sl], np.int64)
        out.append(np.unique(np.concatenate(((i << 16) | j, (j << 16) | i))))
    return out


_pairs_cache = {}


def pairs_within(s, radius):
    """all ordered pairs (i, j), i != j, closer than radius under the minimum image: two index arrays"""
    r = np.stack([np.asarray(s.rx), np.asarray(s.ry), np.asarray(s.rz)], axis=1)
    box = np.array([s.h[0], s.h[4], s.h[8]])
    key = (float(radius), box.tobytes(), r.tobytes())          # (both id variants have the same geometry: searched once)
    if key in _pairs_cache:
        return _pairs_cache[key]
    I, J = [], []
    for i0 in range(0, s.natoms, 500):
        d = r[i0:i0 + 500, None, :] - r[None, :, :]
        d -= box * np.rint(d / box)
        ii, jj = np.nonzero((d * d).sum(axis=2) < radius * radius)
        keep = ii + i0 != jj
        I.append(ii[keep] + i0); J.append(jj[keep])
    _pairs_cache[key] = (np.concatenate(I), np.concatenate(J))
    return _pairs_cache[key]


def classify(s):
    """counts of the ordered pairs (i, j) inside the list radius by the case the build's decision for them falls into, and of
    the beads by their number of excluded partners"""
    I, J = pairs_within(s, s.rmax + s.deltaR)
    gid = np.asarray(s.gid, np.uint64)
    ids = (gid >> np.uint64(32)).astype(np.int64)
    code = (gid & np.uint64(0xffff)).astype(np.int64)
    mt = np.asarray(s.moltype)[np.asarray(s.species)]
    mns = np.asarray(s.mol_nspecies)[mt]
    keys = _bonded_keys(s)
    mask_type = np.array([all(k < 63 for k in np.concatenate((s.bpairI[s.bpair_off[m]:s.bpair_off[m + 1]], s.bpairJ[s.bpair_off[m]:s.bpair_off[m + 1]])))
                          for m in range(s.nmoltype)])
    eq8, eq24, eq32 = (ids[I] & 0xff) == (ids[J] & 0xff), (ids[I] & 0xffffff) == (ids[J] & 0xffffff), ids[I] == ids[J]
    bonded_codes = np.zeros(I.size, bool)
    for m in range(s.nmoltype):
        sel = (mt[I] == m) & (mt[J] == m)
        bonded_codes[sel] = np.isin((code[I[sel]] << 16) | code[J[sel]], keys[m])
    multi = mns[I] > 1
    pruned = eq32 & (~multi | bonded_codes)
    out = {"ids_equal_8_not_24": int((eq8 & ~eq24).sum()), "ids_equal_24_not_32": int((eq24 & ~eq32).sum()), "ids_equal_32": int(eq32.sum()),
           "one_species_pruned": int((eq32 & ~multi).sum()),
           "other_molecule_bonded_codes": int((~eq32 & bonded_codes & multi).sum()),
           "other_molecule_bonded_codes_ids_equal_8": int((~eq32 & bonded_codes & multi & eq8).sum()),
           "other_molecule_bonded_codes_ids_equal_24": int((~eq32 & bonded_codes & multi & eq24).sum()),
           "other_molecule_one_species_ids_equal_8": int((~eq32 & ~multi & eq8 & (mt[I] == mt[J])).sum()),
           "other_molecule_one_species_ids_equal_24": int((~eq32 & ~multi & eq24 & (mns[J] == 1)).sum())}
    by_mask = mask_type[mt[I]] & (code[I] < 63)
    cls = np.where(code[J] < 63, 0, np.where(code[J] < 255, 1, 2))
    for path, psel in (("mask", by_mask), ("search", ~by_mask)):
        for c, cname in enumerate(("partner_lt_63", "partner_63_254", "partner_ge_255")):
            sel = eq32 & multi & psel & (cls == c)
            out["%s_%s" % (path, cname)] = int(sel.sum())
            if not (path == "mask" and c > 0):                  # (a mask type has no bonded partner coded 63 or more)
                out["%s_%s_pruned" % (path, cname)] = int((sel & pruned).sum())
    nexcl = np.bincount(I[pruned], minlength=s.natoms)
    out["beads_excluded_1_4"] = int(((nexcl >= 1) & (nexcl <= 4)).sum())
    out["beads_excluded_5_16"] = int(((nexcl >= 5) & (nexcl <= 16)).sum())
    out["beads_excluded_gt_16"] = int((nexcl > 16).sum())
    out["max_excluded"] = int(nexcl.max())
    return out


# ---- what the CPU and the GPU tests share: the oracle's lists as pair sets, the brute-force reference, both made once per variant
VARIANTS = ("wide", "narrow")
_cache = {}


def system(variant):
    """(Setup, oracle after build_list + forces, energies, virial) -- made once per variant"""
    if variant not in _cache:
        import pyoracle
        s = make_molecule_setup(variant)
        o = pyoracle.Oracle(s)
        npairs = o.build_list()
        e, vir = o.forces()
        _cache[variant] = (s, o, npairs, e, vir)
    return _cache[variant]


def oracle_list(o, which):
    """the oracle's half list `which` (0: kept, 1: excluded) as a set of (i, j), both orders"""
    cs, cj = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_int)()
    o.L.orc_nbr_csr(o.nbr, which, ctypes.byref(cs), ctypes.byref(cj))
    start = np.ctypeslib.as_array(cs, shape=(o.n + 1,))
    if start[-1] == 0:
        return set()
    j = np.ctypeslib.as_array(cj, shape=(start[-1],))
    i = np.repeat(np.arange(o.n), np.diff(start))
    half = set(zip(i.tolist(), j.tolist()))
    return half | set((b, a) for a, b in half)


def reference_pruned(s, I, J):
    """the pruning rule (reOrgPairs): same 32-bit molecule id and (one-species type or (code_i, code_j) in the type's pair list, either order)"""
    ids, code = np.asarray(s.gid, np.uint64) >> np.uint64(32), (np.asarray(s.gid, np.uint64) & np.uint64(0xffff)).astype(np.int64)
    mt = np.asarray(s.moltype)[np.asarray(s.species)]
    bonded = [set(zip(s.bpairI[a:b].tolist(), s.bpairJ[a:b].tolist())) for a, b in zip(s.bpair_off[:-1], s.bpair_off[1:])]
    out = np.zeros(I.size, bool)
    for k in np.flatnonzero(ids[I] == ids[J]):
        i, j = I[k], J[k]
        out[k] = s.mol_nspecies[mt[i]] == 1 or (code[i], code[j]) in bonded[mt[i]] or (code[j], code[i]) in bonded[mt[i]]
    return out


def brute_force_reference(s):
    """every pair i < j in numpy.longdouble under the minimum image: LJ + shift + reaction field for kept pairs, kq (krf r^2 - crf)
    for pruned pairs inside the cut-off; the self term -1/2 sum q^2 keR crf is part of `ele` (bioMartini.c:1030-1035).
    Returns per-bead forces (3, n), lj, ele, virial (xx yy zz xy xz yz), kept and excluded pair sets inside the LIST radius."""
    ld = np.longdouble
    n = s.natoms
    r = np.stack([np.asarray(s.rx, ld), np.asarray(s.ry, ld), np.asarray(s.rz, ld)], axis=1)
    box = np.array([s.h[0], s.h[4], s.h[8]], ld)
    q = np.asarray(s.charge, ld)[np.asarray(s.species)]
    lj = np.asarray(s.ljtype)[np.asarray(s.species)]
    sig, eps, shift = (np.asarray(a, ld).reshape(s.nlj, s.nlj) for a in (s.sigma, s.eps, s.shift))
    keR, krf, crf, rc2, rl2 = ld(s.keR), ld(s.krf), ld(s.crf), ld(s.rmax) ** 2, (ld(s.rmax) + ld(s.deltaR)) ** 2
    f = np.zeros((n, 3), ld)
    vlj, vele, vir = ld(0), -ld(0.5) * (q * q).sum() * keR * crf, np.zeros(6, ld)
    kept, excluded = set(), set()
    # Every pair i < j is looked at.  A pair goes on to the longdouble arithmetic if its double-precision r^2 is below the list
    # radius squared times (1 + 1e-9): the double r^2 is off by a few 1e-16 relative, so no pair inside the radius is dropped, and
    # the longdouble test below decides
    r64, box64 = np.asarray(r, np.float64), np.asarray(box, np.float64)
    for i0 in range(0, n, 400):
        d64 = r64[i0:i0 + 400, None, :] - r64[None, :, :]
        d64 -= box64 * np.rint(d64 / box64)
        ii, jj = np.nonzero((d64 * d64).sum(axis=2) < float(rl2) * (1.0 + 1e-9))
        up = ii + i0 < jj
        ii, jj = ii[up], jj[up]
        I = ii + i0
        d = r[I] - r[jj]
        d -= box * np.rint(d / box)
        r2 = (d * d).sum(axis=1)
        inside = r2 < rl2
        I, jj, d, r2 = I[inside], jj[inside], d[inside], r2[inside]
        pruned = reference_pruned(s, I, jj)
        for sel, out in ((~pruned, kept), (pruned, excluded)):
            out.update(zip(I[sel].tolist(), jj[sel].tolist()))
        cut = r2 < rc2
        I, jj, d, r2, pruned = I[cut], jj[cut], d[cut], r2[cut], pruned[cut]
        kq = keR * q[I] * q[jj]
        sg, ep, sh = sig[lj[I], lj[jj]], eps[lj[I], lj[jj]], shift[lj[I], lj[jj]]
        ir2 = 1 / r2
        ir = np.sqrt(ir2)
        s6 = (sg * sg * ir2) ** 3
        keep = ~pruned
        vlj += ((4 * ep * (s6 * s6 - s6) + sh) * keep).sum()
        vele += (kq * (ir * keep + krf * r2 - crf)).sum()
        dvdr = (24 * ep * (s6 - 2 * s6 * s6) * ir2 - kq * ir2 * ir) * keep + 2 * kq * krf          # (dV/dr) / r
        fij = -dvdr[:, None] * d
        np.add.at(f, I, fij)
        np.subtract.at(f, jj, fij)
        for c, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            vir[c] += (fij[:, a] * d[:, b]).sum()
    sym = lambda h: h | set((b, a) for a, b in h)
    return f.T, vlj, vele, vir, sym(kept), sym(excluded)


_ref_cache = {}


def reference(variant):
    if variant not in _ref_cache:
        _ref_cache[variant] = brute_force_reference(make_molecule_setup(variant))
    return _ref_cache[variant]


_counts = {}


def counts(variant):
    """classify(make_molecule_setup(variant)), made once"""
    if variant not in _counts:
        _counts[variant] = classify(make_molecule_setup(variant))
    return _counts[variant]

"""CPU: the systems of tests/bonded_systems.py are what they claim to be, and their reference is right -- before the device is asked
(tests/test_gpu_bonded_layout.py).  The reference against central differences of tests/closed_forms.py's energies and against the
oracle on the lipid deck; the geometry conditions; the lane layout, recomputed from the term lists alone; the counts of the cases."""
import os

import numpy as np
import pytest

import closed_forms as cf
import bonded_systems as bs
from bonded_systems import A

LIPID_DECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lipid_deck", "object.data")
TIGHT = 1e-10
KINDS = ("bond", "angle", "tors", "impr")
SINGLES = [bs.type_P(), bs.type_L(64), bs.type_G(40), bs.type_X(), bs.type_H(), bs.type_UL(12), bs.type_UH(12, 3), bs.type_T(), bs.type_E(5)]


def closed_form_energies(terms, x):
    e = dict.fromkeys(KINDS, 0.0)
    for t, (i, j) in enumerate(terms["bond_ij"].reshape(-1, 2)):
        e["bond"] += cf.bond_E(x[i], x[j], terms["bond_kb"][t], terms["bond_b0"][t])
    for t, (i, j, k) in enumerate(terms["angle_ijk"].reshape(-1, 3)):
        e["angle"] += cf.angle_E(x[i], x[j], x[k], int(terms["angle_func"][t]), terms["angle_k"][t], terms["angle_t0"][t])
    for t, (i, j, k, l) in enumerate(terms["tors_ijkl"].reshape(-1, 4)):
        f = int(terms["tors_func"][t])
        e["tors" if f == 1 else "impr"] += cf.torsion_E(x[i], x[j], x[k], x[l], f, int(terms["tors_n"][t]), terms["tors_k"][t], terms["tors_delta"][t])
    return e


@pytest.mark.parametrize("mol", SINGLES, ids=[m["name"] for m in SINGLES])
def test_reference_against_central_differences(mol):
    """one copy of each type alone: the reference's energies are the closed forms', its forces their central differences (h = 1e-5,
    the bound of tests/test_closed_forms.py: 2e-7 of the largest force), its virial sum f (x) r in open coordinates"""
    s, terms = bs.single_copy(mol)
    x = np.stack([s.rx, s.ry, s.rz], axis=1)
    f, e, vir = bs.reference(s, terms)
    c = closed_form_energies(terms, x)
    scale = max(abs(v) for v in c.values())
    for k in KINDS:
        assert abs(float(e[k]) - c[k]) < 1e-12 * scale, k
    f = f.astype(np.float64)
    fd = cf.fd_forces(lambda y: sum(closed_form_energies(terms, y).values()), x)
    err = np.abs(f - fd).max() / np.abs(fd).max()
    print(mol["name"], "reference vs central differences: %.2e" % err)
    assert err < 2e-7
    W = f.T @ x
    want = np.array([W[0, 0], W[1, 1], W[2, 2], W[0, 1], W[0, 2], W[1, 2]])
    assert np.abs(vir.astype(np.float64) - want).max() < 1e-11 * max(np.abs(want).max(), np.abs(f).max() * np.abs(x).max())
    assert np.abs(f.sum(axis=0)).max() < 1e-12 * np.abs(f).max()


def test_reference_against_the_oracle_on_the_lipid_deck(built):
    """ties the new reference to the one every other test trusts, on a system both can read: forces, the four energies and the virial
    at 1e-10, relative.  The deck holds an improper at 3.140769 rad (sin phi = 8.2e-4): there the regulariser of the reference's
    dihedral (eps = 1e-12 under the root of cos phi's denominator, bioDihedralFast) moves the force by 2.0e-10 of the largest one, so
    a reference without it misses this bound on that term's four beads -- reference() carries it.  What remains there, 3e-11, is the
    float64 acos of the oracle; the beads of every other term agree to 2e-13 (printed)."""
    import pyoracle
    from ddcmd_amd.deck import load_deck
    from ddcmd_amd.martini import expand_bonded_terms
    s = load_deck(LIPID_DECK)
    s.excludePotentialTerm = 128
    o = pyoracle.Oracle(s)
    fx, fy, fz, e4, vir = o.bonded_only()
    f, e, v = bs.reference(s, expand_bonded_terms(s))
    f = f.astype(np.float64)
    err = max(np.abs(f[:, c] - g).max() for c, g in enumerate((fx, fy, fz))) / max(np.abs(g).max() for g in (fx, fy, fz))
    print("reference vs oracle: forces %.2e" % err, [abs(float(e[k]) - e4[q]) / abs(e4[q]) for q, k in enumerate(KINDS)],
          np.abs(v.astype(np.float64) - vir).max() / np.abs(vir).max())
    for q, k in enumerate(KINDS):
        assert e4[q] != 0.0 and abs(float(e[k]) - e4[q]) < TIGHT * abs(e4[q]), k
    assert np.abs(v.astype(np.float64) - vir).max() < TIGHT * np.abs(vir).max()
    # the beads of no near-planar dihedral first
    t = expand_bonded_terms(s)
    q4 = t["tors_ijkl"].reshape(-1, 4)
    r = np.stack([s.rx, s.ry, s.rz], axis=1)
    box = np.array([s.h[0], s.h[4], s.h[8]])
    x = np.zeros((q4.shape[0], 4, 3))
    for a in (1, 2, 3):
        d = r[q4[:, a]] - r[q4[:, a - 1]]
        x[:, a] = x[:, a - 1] + d - box * np.rint(d / box)
    planar = np.array([abs(np.sin(cf.dihedral_angle(*y))) < 1e-2 for y in x])
    rest = np.setdiff1d(np.arange(s.natoms), q4[planar].ravel())
    g = np.stack([fx, fy, fz], axis=1)
    err_rest = np.abs(f[rest] - g[rest]).max() / np.abs(g).max()
    print("beads of no dihedral with |sin phi| < 1e-2 (%d of %d beads): %.2e" % (rest.size, s.natoms, err_rest))
    assert rest.size >= s.natoms - 8 and err_rest < TIGHT
    assert err < TIGHT


def _sep(s, i, j):
    box = np.array([s.h[0], s.h[4], s.h[8]])
    r = np.stack([s.rx, s.ry, s.rz], axis=1)
    d = r[i] - r[j]
    return d - box * np.rint(d / box)


def _sin(u, w):
    c = (u * w).sum(axis=1) / np.sqrt((u * u).sum(axis=1) * (w * w).sum(axis=1))
    return np.sqrt(np.maximum(0.0, 1.0 - c * c))


@pytest.mark.parametrize("variant", bs.VARIANTS)
def test_geometry_conditions(variant):
    s, terms, info = bs.make_bonded_setup(variant)
    assert 4000 <= s.natoms <= 6000 and s.ngroup == 1 and s.excludePotentialTerm == 128
    ij = terms["bond_ij"].reshape(-1, 2)
    b = np.linalg.norm(_sep(s, ij[:, 0], ij[:, 1]), axis=1)
    assert b.min() >= 3.0 * A and b.max() <= 8.0 * A, (b.min() / A, b.max() / A)
    ijk = terms["angle_ijk"].reshape(-1, 3)
    sel = terms["angle_func"] != 2
    sa = _sin(_sep(s, ijk[:, 0], ijk[:, 1]), _sep(s, ijk[:, 2], ijk[:, 1]))
    assert sel.sum() > 100 and sa[sel].min() >= 0.3
    q = terms["tors_ijkl"].reshape(-1, 4)
    a, bb, c = _sep(s, q[:, 0], q[:, 1]), _sep(s, q[:, 1], q[:, 2]), _sep(s, q[:, 2], q[:, 3])
    assert min(_sin(a, -bb).min(), _sin(bb, -c).min()) >= 0.3
    x = np.zeros((q.shape[0], 4, 3))
    x[:, 1], x[:, 2], x[:, 3] = -a, -a - bb, -a - bb - c
    phi = np.array([cf.dihedral_angle(*y) for y in x])
    assert np.abs(np.sin(phi)).min() >= 0.05
    imp = terms["tors_func"] == 2
    d = phi[imp] - terms["tors_delta"][imp]
    assert imp.sum() >= 3 and np.abs(d).max() < np.pi - 0.2          # (no wrap, and none near it)
    # a 16 A halo holds every partner with room for 45 steps
    for idx, na in ((ij, 2), (ijk, 3), (q, 4)):
        for r in range(1, na):
            assert np.linalg.norm(_sep(s, idx[:, 0], idx[:, r]), axis=1).max() <= 13.0 * A
    # copies of L300 and G are cut by every face of the 2-way grids; so is a copy of every other type but the spacers
    from ddcmd_amd.martini import domain_of
    for grid in ((2, 1, 1), (1, 2, 2), (2, 2, 2)):
        owner = domain_of(s, grid)[np.argsort(info["perm"])]          # by bead of the ordered system
        cut = {k for m in range(info["nmol"]) for k in [info["kind"][info["mol"] == m][0]] if np.unique(owner[info["mol"] == m]).size > 1}
        assert {"L300", "G", "L257", "L256", "P", "X", "H"} <= cut, (grid, cut)


def test_parameter_pairs_of_type_T_differ_in_one_field():
    s, terms, info = bs.make_bonded_setup("lds")
    first = int(np.flatnonzero(info["kind"] == "T")[0])
    q = terms["tors_ijkl"].reshape(-1, 4)
    mine = np.flatnonzero((q[:, 0] >= first) & (q[:, 0] < first + 16))
    par = [(terms["tors_k"][t], terms["tors_delta"][t], int(terms["tors_func"][t]), int(terms["tors_n"][t])) for t in mine]
    assert par[0][:3] == par[1][:3] and (par[0][3], par[1][3]) == (2, 3)
    assert par[2][:2] == par[3][:2] and par[2][3] == par[3][3] and (par[2][2], par[3][2]) == (1, 2)
    b0 = terms["bond_b0"]
    assert np.any((b0 == 0.0) & ~np.signbit(b0)) and np.any((b0 == 0.0) & np.signbit(b0))
    lay = bs.layout(terms)
    # sets are shared by value and only by value: as many as there are distinct rows of constants
    nb = len({(k, b) for k, b in zip(terms["bond_kb"].tolist(), (terms["bond_b0"] + 0.0).tolist())})
    na = len(set(zip(terms["angle_k"].tolist(), terms["angle_t0"].tolist(), terms["angle_func"].tolist())))
    nt = len(set(zip(terms["tors_k"].tolist(), terms["tors_delta"].tolist(), terms["tors_func"].tolist(), terms["tors_n"].tolist())))
    assert (lay[0]["census"]["sets_a"], lay[0]["census"]["sets_b"], lay[1]["census"]["sets_b"]) == (nb, na, nt)


@pytest.mark.parametrize("variant", bs.ORDERED)
def test_layout_targets(variant):
    """every L copy at the lane the table claims, with a filler exactly where the run would have ended at lane 256; G has gaps, X
    alternates; the tables' piece counts"""
    s, terms, info = bs.make_bonded_setup(variant)
    lay = bs.layout(terms)
    lane, atoms, near = lay[0]["lane_of"], lay[0]["atoms"], lay[0]["near"]
    seen = set()
    for m, n, target in info["targets"]:
        at = np.flatnonzero(info["mol"] == m)
        assert at.size == n and info["kind"][at[0]] == "L%d" % n
        l0 = int(lane[at[0]])
        assert np.array_equal(lane[at], l0 + np.arange(n))
        if n <= 256 and target + n > 256:
            assert l0 % 256 == 0 and np.all(atoms[l0 - (256 - target):l0] == -1) and atoms[l0 - (256 - target) - 1] >= 0
            assert near[lane[at]].all()
        else:
            assert l0 % 256 == target and (l0 == 0 or atoms[l0 - 1] >= 0)
            assert near[lane[at]].all() == (n <= 256)
        if n > 256:          # straddles by design: far exactly where a partner (the two atoms before, the two behind) is in another workgroup
            l = lane[at]
            far = np.array([any((l[k] // 256) != (l[j] // 256) for j in range(max(0, k - 2), min(n, k + 3))) for k in range(n)])
            assert np.array_equal(~near[l], far) and far.any()
        seen.add((n, target + n - 256 if n <= 256 else None))
    for n in (64, 65, 255, 256):
        assert (n, 0) in seen and (n, 1) in seen, (n, seen)          # fits exactly; one lane too long
    g = np.flatnonzero(info["kind"] == "G")
    for q in (0, 1):
        mine = g[lay[q]["lane_of"][g] >= 0]
        assert np.array_equal(mine % 2, np.full(mine.size, 1 - q) ^ (g[0] % 2)) and mine.size == 100
        assert np.all(np.diff(lay[q]["lane_of"][mine]) == 1) and np.all(np.diff(mine) == 2)
        assert not lay[q]["near"][lay[q]["lane_of"][mine]].any()
        w = lay[q]["lane_of"][mine] // 64          # ... and true elsewhere in the same wave
        others = [l for l in np.flatnonzero(np.isin(np.arange(lay[q]["atoms"].size) // 64, (w.min(), w.max()))) if lay[q]["atoms"][l] >= 0 and lay[q]["atoms"][l] not in mine]
        assert len(others) > 0 and lay[q]["near"][others].all()
    x = np.flatnonzero(info["kind"] == "X")
    assert np.all(np.diff(lane[x]) == 1) and near[lane[x]].all()
    ij = terms["bond_ij"].reshape(-1, 2)
    xb = ij[np.isin(ij[:, 0], x)]
    assert np.all(np.abs(xb[:, 0] - xb[:, 1]) == 2) and np.all(np.abs(lane[xb[:, 0]] - lane[xb[:, 1]]) == 2)
    want = {"lds": (True, True), "light_spills": (False, True), "heavy_spills": (True, False), "edge": (True, True), "edge385": (False, True)}[variant]
    pieces = (lay[0]["census"]["pieces"], lay[1]["census"]["pieces"])
    assert (pieces[0] <= bs.GB_TAB_PIECES, pieces[1] <= bs.GB_TAB_PIECES) == want, pieces
    if variant.startswith("edge"):
        assert pieces[0] == (384 if variant == "edge" else 385)


@pytest.mark.parametrize("variant", bs.VARIANTS)
def test_case_counts(variant):
    """every variant has filler lanes and waves of all three classes; terms of every kind span two waves, bonds and func 2/10 angles
    two workgroups.  A run of at most 256 lanes never spans two workgroups (that is what the fillers are for), so of the L copies
    L257 and L300 contribute those, and both do"""
    s, terms, info = bs.make_bonded_setup(variant)
    lay = bs.layout(terms)
    cen = [lay[q]["census"] for q in (0, 1)]
    print(variant, cen, bs.span_counts(terms, lay))
    assert cen[0]["fillers"] + cen[1]["fillers"] >= 2
    for k in ("waves_all_near", "waves_mixed", "waves_far"):
        assert cen[0][k] + cen[1][k] >= 1, k
    sp = bs.span_counts(terms, lay)
    for kind in ("bond", "angle2", "angle1", "dihedral"):
        assert sp[kind][0] >= 3, (kind, sp)
    assert sp["bond"][1] >= 4 and sp["angle2"][1] >= 4
    if variant in bs.ORDERED:
        lane = lay[0]["lane_of"]
        ij, ijk = terms["bond_ij"].reshape(-1, 2), terms["angle_ijk"].reshape(-1, 3)
        for m, n, target in info["targets"]:
            at = np.flatnonzero(info["mol"] == m)
            nb = int((np.isin(ij[:, 0], at) & (lane[ij[:, 0]] // 256 != lane[ij[:, 1]] // 256)).sum())
            na = int((np.isin(ijk[:, 0], at) & (lane[ijk].max(axis=1) // 256 != lane[ijk].min(axis=1) // 256)).sum())
            assert (nb >= 1 and na >= 2) if n > 256 else (nb == 0 and na == 0), (n, target, nb, na)

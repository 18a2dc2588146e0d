"""CPU tests of the adversarial molecular systems (tests/molecule_systems.py): the generator populates every case of the list
build's decision ladder, and the oracle decides and evaluates them like the brute-force reference of that module -- all pairs
in numpy.longdouble, independent of the oracle's cell list and of its pair_is_pruned."""
import numpy as np
import pytest

import pyoracle
import molecule_systems
from molecule_systems import (make_molecule_setup, molecule_types, pairs_within, C_HEAD_PAIRS, C_DECOYS, VARIANTS,
                              system, reference, oracle_list, water_collider)

PAIR_CASES = ("ids_equal_8_not_24", "ids_equal_32", "one_species_pruned", "other_molecule_bonded_codes", "other_molecule_bonded_codes_ids_equal_8",
              "other_molecule_one_species_ids_equal_8",
              "mask_partner_lt_63", "mask_partner_lt_63_pruned", "mask_partner_63_254", "mask_partner_ge_255",
              "search_partner_lt_63", "search_partner_lt_63_pruned", "search_partner_63_254", "search_partner_63_254_pruned",
              "search_partner_ge_255", "search_partner_ge_255_pruned")
WIDE_ONLY = ("ids_equal_24_not_32", "other_molecule_bonded_codes_ids_equal_24", "other_molecule_one_species_ids_equal_24")


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_case_of_the_decision_ladder_is_populated(variant):
    """a condition on the inputs: at least 20 ordered pairs inside the list radius in every case, a bead with more excluded
    partners than the 16 rows the build starts with, beads with 5..16 (entries past the four the pair kernel prefetches)"""
    s = make_molecule_setup(variant)
    counts = molecule_systems.counts(variant)
    print(variant, counts)
    for k in PAIR_CASES + (WIDE_ONLY if variant == "wide" else ()):
        assert counts[k] >= 20, (k, counts[k])
    if variant == "narrow":
        assert all(counts[k] == 0 for k in WIDE_ONLY)
    assert counts["beads_excluded_gt_16"] >= 1 and counts["max_excluded"] >= 24
    assert counts["beads_excluded_5_16"] >= 20 and counts["beads_excluded_1_4"] >= 20
    # the hubs: bonded to at least 24 beads inside the list radius, hub and partners charged
    D = next(t for t in molecule_types() if t["name"] == "D")
    I, J = pairs_within(s, s.rmax + s.deltaR)
    code = (np.asarray(s.gid, np.uint64) & np.uint64(0xffff)).astype(np.int64)
    q = np.asarray(s.charge)[np.asarray(s.species)]
    hubs = np.flatnonzero((s.mol_kind == "D") & (code == D["hub"]))
    assert hubs.size == 2
    for h in hubs:
        partners = J[(I == h) & (s.copy_of[J] == s.copy_of[h]) & (code[J] < 36)]
        assert partners.size >= 24 and q[h] != 0 and (q[partners] != 0).sum() >= 12


def test_the_boundary_pairs_and_their_decoys_face_each_other():
    """type C: every bonded pair across a boundary of the encodings and every aliasing non-pair lies inside the list radius
    in both copies -- and, for the two neighbouring copies whose ids differ only above bit 23, between the copies too"""
    s = make_molecule_setup("wide")
    I, J = pairs_within(s, s.rmax + s.deltaR)
    code = (np.asarray(s.gid, np.uint64) & np.uint64(0xffff)).astype(np.int64)
    isC = s.mol_kind == "C"
    near = set(zip(I[isC[I] & isC[J]].tolist(), J[isC[I] & isC[J]].tolist()))
    copies = np.unique(s.copy_of[isC])
    assert copies.size == 2
    where = {(k, c): int(np.flatnonzero((s.copy_of == k) & (code == c))[0]) for k in copies for c in set(sum(C_HEAD_PAIRS + C_DECOYS, ()))}
    for a, b in C_HEAD_PAIRS + C_DECOYS:
        for k in copies:
            assert (where[(k, a)], where[(k, b)]) in near, (hex(a), hex(b), k)
    across = sum((where[(copies[0], a)], where[(copies[1], b)]) in near or (where[(copies[1], a)], where[(copies[0], b)]) in near for a, b in C_HEAD_PAIRS)
    assert across >= 6, across
    ids = np.asarray(s.gid, np.uint64) >> np.uint64(32)
    m0, m1 = (int(ids[s.copy_of == k][0]) for k in copies)
    assert m1 - m0 == 1 << 24


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_molecule_id_collides_with_a_neighbouring_water_beads(variant):
    """the case `a one-species molecule whose id is a neighbouring WATER bead's id + 2^24` (+ 2^16 in the narrow variant) exists:
    the water generator's id of a bead is its lattice index, bead w is still water, and it lies inside the list radius of all
    three beads of that molecule"""
    s = make_molecule_setup(variant)
    w = water_collider()
    ids = (np.asarray(s.gid, np.uint64) >> np.uint64(32)).astype(np.int64)
    assert ids[w] == w and s.mol_kind[w] == "W" and s.mol_nspecies[s.moltype[s.species[w]]] == 1
    mol = np.flatnonzero(ids == w + ((1 << 24) if variant == "wide" else (1 << 16)))
    assert mol.size == 3 and (s.mol_kind[mol] == "E").all() and np.unique(s.copy_of[mol]).size == 1
    I, J = pairs_within(s, s.rmax + s.deltaR)
    assert set(J[I == w].tolist()) >= set(mol.tolist())
    assert (ids[mol] & 0xffff == w).all() and ((ids[mol] & 0xffffff == w).all() == (variant == "wide"))


@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_equals_the_brute_force_reference(variant):
    """the oracle's kept and excluded lists are the reference's pair SETS; forces, lj, ele and virial agree to the tolerances
    of the lipid deck's O(N^2) check (test_oracle.py)"""
    s, o, npairs, e, vir = system(variant)
    f, vlj, vele, bvir, kept, excluded = reference(variant)
    assert oracle_list(o, 0) == kept
    assert oracle_list(o, 1) == excluded
    assert npairs[0] == len(kept) // 2 and npairs[1] == len(excluded) // 2 and npairs[1] > 1000
    fmax = np.abs(f).max()
    worst = max(np.abs(np.asarray(g, np.longdouble) - f[c]).max() for c, g in enumerate((o.fx, o.fy, o.fz))) / fmax
    print(variant, "forces %.2e lj %.2e ele %.2e virial %.2e" % (worst, abs(vlj - e["lj"]) / abs(vlj), abs(vele - e["ele"]) / abs(vele),
                                                                   np.abs((bvir - vir) / bvir).max()))
    assert worst < 1e-12
    assert abs(vlj - e["lj"]) < 1e-12 * abs(vlj) and abs(vele - e["ele"]) < 1e-11 * abs(vele)
    assert np.allclose(np.asarray(bvir, np.float64), vir, rtol=1e-10, atol=1e-12)
    # the excluded pairs matter: leaving their reaction-field terms out moves `ele` by far more than any tolerance here
    assert abs(e["ele"]) > 1e-3


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_relabelled_box_steps_stably(variant):
    """45 steps of the oracle: finite energies, nobody moves more than the skin in one step, the excluded list changes with
    the rebuilds but stays as large"""
    s = make_molecule_setup(variant)
    o = pyoracle.Oracle(s)
    n1 = o.build_list()[1]
    o.forces()
    box = np.array([s.h[0], s.h[4], s.h[8]])
    for step in range(45):
        before = np.stack([o.rx, o.ry, o.rz], axis=1).copy()
        e, vir, rk, _ = o.step(1)
        d = np.stack([o.rx, o.ry, o.rz], axis=1) - before
        d -= box * np.rint(d / box)
        assert np.isfinite(e["total"]) and np.isfinite(rk) and np.isfinite(vir).all(), step
        assert np.sqrt((d * d).sum(axis=1)).max() < s.deltaR, step
    assert abs(o.L.orc_nbr_npairs(o.nbr, 1) - n1) < 0.05 * n1

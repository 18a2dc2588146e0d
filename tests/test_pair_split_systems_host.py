"""CPU tests of the split-occupancy boxes (tests/pair_split_systems.py): the tiles own the counts they are meant to, the counts drive every
lane split and row part of the pair kernel as split_plan restates it, the geometry keeps a lost pair far above every rounding bound, and the
module's longdouble reference agrees with the oracle."""
import numpy as np
import pytest

import pyoracle
import pair_split_systems as P


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_target_tiles_hold_the_intended_counts(variant):
    """the counts come from tile_of, a restatement of the device's cell and tile assignment (setup_grid, cell_coords, cell_linear), not from
    the generator's bookkeeping; no bead is closer than 1 A to a face of its tile, so no rounding decides; 41 owned tiles stay empty"""
    s = P.system(variant)
    g = P.grid_of(s)
    assert g["n"] == [32, 16, 16] and g["T"] == [6, 6, 6] and g["m"] == [8, 4, 4]
    t, margin = P.tile_of(s)
    assert margin.min() > 1.0 * P.ANG
    cnt = np.bincount(t, minlength=216)
    want = {P.device_tile(s, ijk): c for ijk, (c, _) in s.plan.items()}
    assert {int(k): int(cnt[k]) for k in np.flatnonzero(cnt)} == want
    assert sorted(want.values()) == sorted(P.COUNTS) and s.natoms == sum(P.COUNTS) == 3606
    assert P.NTILE ** 3 - len(want) == 41
    # the generator's own record of a bead's tile says the same
    assert np.array_equal(t, [P.device_tile(s, ijk) for ijk in s.tile_ijk])
    # tiles whose neighbourhood reaches the image margin (shifted partners, the virial per pair) and tiles that stage owned beads only
    faces = [c for ijk, (c, _) in s.plan.items() if P.stages_images(ijk)]
    inner = [c for ijk, (c, _) in s.plan.items() if not P.stages_images(ijk)]
    assert len(faces) >= 12 and len(inner) >= 5 and max(inner) == 600 and min(inner) == 1 and 513 in faces and 3 in faces
    # every neighbourhood below the 4096 beads of packed entries: the whole box is
    assert s.natoms < 4096


def test_split_plan_arithmetic():
    """split_plan against hand-worked cases of the kernel's formulas"""
    assert P.split_plan(1, 0, 1) == {(1, 64, 1)}
    assert P.split_plan(8, 0, 1) == {(1, 64, 1)}
    assert P.split_plan(9, 0, 1) == {(2, 32, 2), (2, 64, 1)}
    assert P.split_plan(64, 0, 1) == {(8, 8, 8)}
    assert P.split_plan(65, 0, 1) == {(16, 4, 16), (16, 64, 1)}
    assert P.split_plan(512, 0, 1) == {(64, 1, 64)}
    assert P.split_plan(513, 0, 1) == {(64, 1, 64), (1, 64, 1)} and P.row_trips(513, 0, 1) == 2
    assert P.split_plan(600, 0, 1) == {(64, 1, 64), (16, 4, 16), (16, 8, 8)} and P.row_trips(600, 0, 1) == 2
    assert P.row_range(5, 0, 8) == (0, 0) and P.split_plan(5, 0, 8) == set() and P.row_trips(5, 0, 8) == 0      # a part without rows
    assert [P.row_range(3, p, 8) for p in range(8)] == [(0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 3)]
    assert P.split_plan(600, 2, 3) == {(32, 2, 32), (32, 8, 8)}
    assert P.decode_item(77 | (5 << 24) | (7 << 27)) == (77, 5, 8) and P.decode_item(9) == (9, 0, 1)


def test_the_counts_drive_every_split():
    """what tests/test_gpu_pair_split.py walks under DDCMI_DEBUG_TAIL=k, k in NPARTS: every R and every `parts` in {1, 2, 4 ... 64}, chunks
    with kb < R, tiles with two row0 trips, parts without rows -- k = 1 alone holds every R and every `parts`, every k a partial chunk and 64 lanes per bead"""
    pow2 = {1, 2, 4, 8, 16, 32, 64}
    union = P.plan_union(P.COUNTS, P.NPARTS)
    assert {R for R, _, _ in union} == pow2
    assert {parts for _, parts, _ in union} == pow2
    assert any(kb < R for R, _, kb in union)
    assert any(P.row_trips(c, 0, 1) == 2 for c in P.COUNTS)
    assert {R for R, _, _ in P.plan_union(P.COUNTS, (1,))} == pow2 and {parts for _, parts, _ in P.plan_union(P.COUNTS, (1,))} == pow2
    for k in P.NPARTS:
        u = P.plan_union(P.COUNTS, (k,))
        assert 64 in {parts for _, parts, _ in u} and any(kb < R for R, _, kb in u), k
        if k > 1:
            assert any(P.row_range(c, p, k)[0] == P.row_range(c, p, k)[1] for c in P.COUNTS for p in range(k)), k      # nown < nparts
    # every lanes-per-bead count meets an R-chunk that is full and one that is not
    assert all(any(p == parts and kb == R for R, p, kb in union) for parts in pow2 - {64})
    # lanes per bead of 32 and 64: the __shfl_xor steps behind the DPP butterflies
    assert {(2, 32, 2), (1, 64, 1), (64, 64, 1)} <= union


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_geometry_keeps_a_lost_pair_visible(variant):
    """no pair within 1e-6 (relative) of the cut-off; every pair with a term has |f_ij| >= 1e-6 of the larger of A_i, A_j (pairs with a
    term: the kept ones, and excluded pairs of two charged beads -- an excluded pair with an uncharged bead has no term at all); every
    bead has partners"""
    s, ref = P.system(variant), P.system_reference(variant)
    print(variant, "pairs %d excluded with a term %d, nearest to the cut-off %.3g, smallest |f_ij| / A %.3g" % (ref["npair"], ref["nexcl"], ref["rel_gap"], ref["fmin_rel"]))
    assert ref["rel_gap"] >= 1e-6
    assert ref["fmin_rel"] >= 1e-6
    assert ref["A"].min() > 0
    assert ref["npair"] > 60000
    r = np.stack([s.rx, s.ry, s.rz], 1)
    near = np.sqrt(((r[:, None, :] - r[None, :, :]) ** 2).sum(axis=2) + 1e30 * np.eye(s.natoms)).min()
    assert near > 4.09 * P.ANG


def test_charged_variant_drives_the_excluded_walk():
    """charged_mol: 10 classes (more than the 8 of packed entries, fewer than 17); every tile of three or more beads holds a molecule, so the
    excluded walk meets every lanes-per-bead count; beads with five partners (one behind the four the walk prefetches); no bead has more
    excluded partners than the 16 rows the build starts with, and every excluded pair lies inside the cut-off, so inside its tile's staged
    neighbourhood"""
    s, ref = P.system("charged_mol"), P.system_reference("charged_mol")
    classes = {(int(s.ljtype[sp]), float(s.charge[sp])) for sp in range(s.nspecies)}
    assert len(classes) == 10
    ne = P.excluded_partners(s)
    assert ne.max() == 5 and (ne == 5).sum() >= 300 and (ne == 2).sum() >= 300
    for ijk, (c, _) in s.plan.items():
        sel = (s.tile_ijk == np.array(ijk)).all(axis=1)
        assert (ne[sel] > 0).any() == (c >= 3), (ijk, c)
    r = np.stack([s.rx, s.ry, s.rz], 1) / P.ANG
    for mol in range(int(s.mol_of.max()) + 1):
        x = r[s.mol_of == mol]
        assert np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)).max() < P.MOL_SPAN_A
    assert ref["nexcl"] > 1500
    q = s.charge[s.species]
    assert (q != 0).sum() > 0.6 * s.natoms and abs(q).max() == 0.1


def test_types20_has_twenty_classes_and_one_type_two():
    assert P.system("types20").nlj == 20 and len(set(P.system("types20").ljtype.tolist())) == 20
    assert P.system("one_type").nlj == 2 and not np.any(P.system("one_type").charge)


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_reference_equals_the_oracle(variant):
    """forces, lj, ele and virial of reference() against pyoracle on the same setup, to the tolerances of
    tests/test_molecule_systems_host.py; the oracle excludes the pairs the reference excludes"""
    s, ref = P.system(variant), P.system_reference(variant)
    o = pyoracle.Oracle(s)
    npairs = o.build_list()
    e, vir = o.forces()
    f = ref["f"]
    fmax = np.abs(f).max()
    worst = max(np.abs(np.asarray(g, np.longdouble) - f[:, c]).max() for c, g in enumerate((o.fx, o.fy, o.fz))) / fmax
    print(variant, "forces %.2e lj %.2e virial %.2e" % (worst, abs(ref["lj"] - e["lj"]) / abs(ref["lj"]), np.abs((ref["vir"] - vir) / ref["vir"]).max()))
    assert worst < 1e-12
    assert abs(ref["lj"] - e["lj"]) < 1e-12 * abs(ref["lj"])
    if variant == "charged_mol":
        assert abs(ref["ele"] - e["ele"]) < 1e-11 * abs(ref["ele"]) and abs(e["ele"]) > 1e-3
        assert npairs[1] >= ref["nexcl"] > 0
    else:
        assert e["ele"] == 0.0 and ref["ele"] == 0
    assert np.allclose(np.asarray(ref["vir"], np.float64), vir, rtol=1e-10, atol=1e-12)

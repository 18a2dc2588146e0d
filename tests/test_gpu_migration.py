"""GPU tests (-m gpu): bead ownership and migration at brick faces, edges and corners -- k_mig_classify, k_compact_order,
k_unpack_mig and the host rounds of ddcmi_multigpu.inl -- on the systems of tests/migration_systems.py (its docstring says what each
plants and what the reference is).

After the first force evaluation and after every rebuild period, for every builder and grid:
  * every gid is owned exactly once (the multiset of the ranks' downloads, not a count);
  * the owner is owner_exact; only the planted near_face beads (their number is fixed by tests/test_migration_systems_host.py) may
    sit on either side, and their count is printed;
  * the direction codes taken (from the owners before and after) and nlocal per rank are the census of the reference, apart from those
    open cases;
  * positions (after the wrap's own statement on both downloads: back_in_box and k_mig_classify's wrap are the same operation),
    velocities, forces (the restraints follow the gid), species and the LCG64 state, prime and multID of every bead equal a
    single-domain MartiniHIP run of the same setup BIT FOR BIT; FROZEN beads have not moved, FIXEDVELOCITY beads have the velocity
    they started with -- restrained ones too, whose FREE neighbours in the planted set have been accelerated;
  * the VAF and MSD sums of the ranks, added in rank order, equal the single domain's within  2 n u sum|t_i| (1 + 1e-3)  per class of
    n beads: both are sums of the same n per-bead terms (bit-identical beads) added in two different orders, each within
    (n - 1) u sum|t_i| of the exact sum; the MSD also equals the unwrapped drift of the reference within the passengers'
    perturbation bound, so a wrap taken for a displacement (a box length, squared) cannot hide."""
import os
import sys
import tempfile

import numpy as np
import pytest

import migration_systems as M
from ddcmd_amd.martini import DdcmiError, MartiniGroup, MartiniHIP
from ranks import ROOT, rank_env, run_ranks

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
DDCMI_EINVAL = -2
IDS = ["%d%d%d-pbc%d" % (g + (p,)) for g, p in M.GRIDS]
THREES = [(g, p) for g, p in M.GRIDS if max(g) >= 3]
ID3 = ["%d%d%d-pbc%d" % (g + (p,)) for g, p in THREES]

_single = {}


def _order(s):
    return np.argsort(np.asarray(s.gid, np.uint64), kind="stable")


def _frame_single(m, s, vaf):
    d = m.download()
    box = M.box_of(s)
    f = dict(r=M.wrap64(np.stack(d["r"], 1), box, s.pbc), v=np.stack(d["v"], 1), f=np.stack(d["f"], 1))
    if getattr(s, "lcg64", None) is not None:
        f["lcg"] = m.get_random_lcg64()
    if vaf:
        f["vaf"] = m.vaf_sample()
    return f


def single_domain(s, periods, vaf=True):
    """the one-domain run of the setup, frames in setup order; made once per setup"""
    key = (s.name, periods, vaf)
    if key not in _single:
        m = MartiniHIP(s)
        m.eval_forces()
        if vaf:
            m.vaf_origin()
        frames = [_frame_single(m, s, vaf)]
        for _ in range(periods):
            m.step(M.UPDATE)
            frames.append(_frame_single(m, s, vaf))
        m.close()
        _single[key] = frames
    return _single[key]


def _frame_group(g, s, vaf):
    """setup order; owner per bead; raises on a lost or duplicated gid"""
    parts = [r.download_particles() for r in g.ranks]
    gid = np.concatenate([p["gid"] for p in parts])
    want = np.sort(np.asarray(s.gid, np.uint64))
    assert len(gid) == s.natoms and (np.sort(gid) == want).all(), \
        "gids lost: %s, twice or unknown: %s" % (np.setdiff1d(want, gid)[:8], [int(x) for x in gid if (gid == x).sum() > 1 or x not in want][:8])
    owner = np.concatenate([np.full(len(p["gid"]), k) for k, p in enumerate(parts)])
    o = np.argsort(gid, kind="stable")
    back = np.empty(s.natoms, int)
    back[_order(s)] = np.arange(s.natoms)          # setup index -> place in gid order

    def by_setup(a):
        return a[o][back]
    box = M.box_of(s)
    f = dict(owner=by_setup(owner), nlocal=np.array([len(p["gid"]) for p in parts]),
             species=by_setup(np.concatenate([p["species"] for p in parts])))
    for k in ("r", "v", "f"):
        f[k] = by_setup(np.stack([np.concatenate([p[k][c] for p in parts]) for c in range(3)], 1))
    f["r"] = M.wrap64(f["r"], box, s.pbc)
    if getattr(s, "lcg64", None) is not None:
        f["lcg"] = by_setup(np.concatenate([p["lcg64"] for p in parts if "lcg64" in p]))
    if vaf:
        f["vaf"] = g.vaf_sample()
    return f


def group_run(s, grid, periods, vaf=True):
    g = MartiniGroup(s, grid)
    try:
        g.eval_forces()
        if vaf:
            g.vaf_origin()
        frames = [_frame_group(g, s, vaf)]
        for _ in range(periods):
            g.step(M.UPDATE)
            frames.append(_frame_group(g, s, vaf))
    finally:
        g.close()
    return frames


def _classes(s):
    """membership of the 1 + ngroup + nspecies classes of a VAF sample"""
    ng, ns = max(1, int(s.ngroup)), int(s.nspecies)
    gr, sp = np.asarray(s.group), np.asarray(s.species)
    return [np.ones(s.natoms, bool)] + [gr == k for k in range(ng)] + [sp == k for k in range(ns)]


def check_vaf(s, fg, fs, k, label):
    v0 = M.velocities(s)
    mv = M.moves(s)
    pert = M.perturbation_bound(s, 30) * M.ANG if (s.nrest or getattr(s, "lcg64", None) is not None) else 0.0
    L = M.box_of(s).max()
    d = np.abs(v0) * mv[:, None] * (k * M.UPDATE * s.dt)               # the unwrapped drift of the reference, per component
    delta = pert + (k * M.UPDATE + 4 * k + 4) * U * L                  # per component: one rounding per step, the wrap's corrections
    (vg, mg), (vs, ms) = fg["vaf"], fs["vaf"]
    for c, member in enumerate(_classes(s)):
        n = int(member.sum())
        tv = (np.abs(fs["v"][member]) * np.abs(v0[member])).sum()
        tol_v = 2 * n * U * tv * 1.001
        tol_m = 2 * n * U * abs(ms[c]) * 1.001
        print("%s frame %d class %d: n %d  dVAF %.3e (bound %.3e)  dMSD %.3e (bound %.3e)" % (label, k, c, n, abs(vg[c] - vs[c]), tol_v, abs(mg[c] - ms[c]), tol_m))
        assert abs(vg[c] - vs[c]) <= tol_v and abs(mg[c] - ms[c]) <= tol_m, (label, k, c)
        want = (d[member] ** 2).sum()
        tol_w = (2 * d[member] * delta + delta * delta).sum() + n * U * want
        assert abs(mg[c] - want) <= tol_w, (label, k, c, mg[c], want, tol_w)          # a wrap is no displacement


def check_frames(s, grid, frames, single, label, census=True):
    box = M.box_of(s)
    periods = len(frames) - 1
    snaps = M.snapshots(s, periods * M.UPDATE)
    cen = M.direction_census(s, grid, snaps)
    v0 = M.velocities(s)
    kinds = np.asarray(s.group_type)[np.asarray(s.group)] if getattr(s, "ngroup", 0) else np.zeros(s.natoms, int)
    for k, (fg, fs) in enumerate(zip(frames, single)):
        # the right owner: of the device's own stored position (bit for bit the single domain's, below), open only for near_face beads
        ok, nopen = M.acceptable_owner(fg["owner"], fg["r"], box, grid, s.pbc)
        exact = M.owner_exact(fg["r"], box, grid, s.pbc)
        print("%s frame %d: %d near_face beads, %d of them on the other side of the rational face" % (label, k, nopen, int((fg["owner"] != exact).sum())))
        assert ok.all(), (label, k, np.flatnonzero(~ok)[:8], fg["owner"][~ok][:8], exact[~ok][:8])
        nf = M.near_face(fg["r"], box, grid, s.pbc)
        ref_owner = M.owner_exact(snaps[k], box, grid, s.pbc)
        assert (fg["owner"][~nf] == ref_owner[~nf]).all(), (label, k)                    # ... and the owner the reference predicted
        assert np.abs(fg["nlocal"] - cen[k][1]).sum() <= 2 * nopen and fg["nlocal"].sum() == s.natoms, (label, k, fg["nlocal"], cen[k][1])
        if k and census:
            # the directions taken, as k_mig_classify folds them, of the beads that were and are away from the faces
            prev = frames[k - 1]
            sure = ~nf & ~M.near_face(prev["r"], box, grid, s.pbc)
            c0 = np.stack([prev["owner"] % grid[0], (prev["owner"] // grid[0]) % grid[1], prev["owner"] // (grid[0] * grid[1])], 1)
            c1 = np.stack([fg["owner"] % grid[0], (fg["owner"] // grid[0]) % grid[1], fg["owner"] // (grid[0] * grid[1])], 1)
            d = c1 - c0
            for a, per in enumerate(M.per_axis(s.pbc)):
                if per:
                    d[:, a] = np.where(d[:, a] > 1, d[:, a] - grid[a], np.where(d[:, a] < -1, d[:, a] + grid[a], d[:, a]))
            code = (d[:, 0] + 1) + 3 * (d[:, 1] + 1) + 9 * (d[:, 2] + 1)
            got = np.bincount(code[sure & (code != 13)], minlength=27)
            assert np.abs(got - cen[k][0]).sum() <= (~sure).sum(), (label, k, got, cen[k][0])
            if not nf.any():
                assert (got == cen[k][0]).all()
        # state rides along, bit for bit
        for key in ("r", "v", "f"):
            same = fg[key] == fs[key]
            assert same.all(), (label, k, key, np.flatnonzero(~same.all(axis=1))[:8], fg[key][~same][:4], fs[key][~same][:4])
        assert (fg["species"] == np.asarray(s.species)).all(), (label, k)
        if "lcg" in fg:
            for key in ("state", "prime", "multID"):
                assert (fg["lcg"][key] == fs["lcg"][key]).all(), (label, k, key)
            assert (fg["lcg"]["prime"] == s.lcg64["prime"]).all() and (fg["lcg"]["multID"] == s.lcg64["multID"]).all()
            lang = kinds == M.LANGEVIN
            if k:
                assert (fg["lcg"]["state"][lang] != s.lcg64["state"][lang]).all()          # the streams were drawn from
        # the kinds: FROZEN has not moved, FIXEDVELOCITY keeps its velocity (restrained or not), a restrained FREE bead does not
        frozen, fixed = kinds == M.FROZEN, kinds == M.FIXEDVELOCITY
        assert (fg["r"][frozen] == M.wrap64(M.positions(s), box, s.pbc)[frozen]).all() and (fg["v"][fixed] == v0[fixed]).all()
        # unforced beads are where the reference has them
        plain = ((kinds == M.FREE) | fixed)
        if s.nrest:
            plain[np.asarray(s.rest_bead)] &= fixed[np.asarray(s.rest_bead)]
        assert (fg["r"][plain] == snaps[k][plain]).all(), (label, k)
        if s.nrest and k:
            rb = np.asarray(s.rest_bead)
            rb = rb[(kinds[rb] == M.FREE) & (np.asarray(s.rest_fc) != 0).any(axis=1)]
            assert len(rb) and (fg["v"][rb] != v0[rb]).any(axis=1).all() and (fg["f"][rb] != 0).any(axis=1).all()
        if "vaf" in fg:
            check_vaf(s, fg, fs, k, label)


@pytest.mark.parametrize("grid,pbc", M.GRIDS, ids=IDS)
def test_crossers_through_faces_edges_and_corners(grid, pbc):
    s = M.system("crossers", grid, pbc, passengers=True)
    frames = group_run(s, grid, 2)
    check_frames(s, grid, frames, single_domain(s, 2), s.name)


@pytest.mark.parametrize("grid,pbc", M.GRIDS, ids=IDS)
def test_face_sitters_have_one_owner_beside_their_face(grid, pbc):
    """also: a restrained sitter delivered to either side of its face feels the single domain's force, bit for bit (check_frames
    compares every force), whichever brick's cell grid took it in"""
    s = M.system("face_sitters", grid, pbc, passengers=True)
    frames = group_run(s, grid, 2)
    check_frames(s, grid, frames, single_domain(s, 2), s.name)
    rb = np.asarray(s.rest_bead)
    assert (frames[0]["f"][rb] != 0).any(axis=1).all()


@pytest.mark.parametrize("name,grid,pbc", [("crossers", (2, 2, 2), 7), ("crossers", (3, 2, 1), 6), ("face_sitters", (3, 2, 1), 7), ("face_sitters", (2, 2, 2), 7)],
                         ids=["crossers-222-pbc7", "crossers-321-pbc6", "face_sitters-321-pbc7", "face_sitters-222-pbc7"])
def test_a_decomposed_run_repeats_bit_for_bit(name, grid, pbc):
    """the face sitters among them: whichever side a bead within ulps of a face is given to, it is the same side every time"""
    s = M.system(name, grid, pbc, passengers=True)
    a, b = group_run(s, grid, 2), group_run(s, grid, 2)
    for fa, fb in zip(a, b):
        for key in ("owner", "r", "v", "f", "species", "nlocal"):
            assert (fa[key] == fb[key]).all(), key
        for key in ("state", "prime", "multID"):
            assert (fa["lcg"][key] == fb["lcg"][key]).all()
        assert all((x == y).all() for x, y in zip(fa["vaf"], fb["vaf"]))


@pytest.mark.parametrize("variant,vaf", [("face", False), ("corner", True)])
def test_crowd_overflows_the_first_capacity_and_is_redone(variant, vaf):
    """1100 beads through one direction in one rebuild: the segments of 1024 records overflow and the classification is repeated with
    a larger mig_cap (records 16 wide with VAF tracking on).  The second run in the same group finds the capacity large enough from
    the start: after ddcmi_upload_state of the same beads it takes no redo, and must give the same result bit for bit."""
    import copy
    s = copy.copy(M.system("crowd", variant, passengers=True))
    # (LCG64 streams cannot be set again on a decomposed context that has built a list: this system's LANGEVIN group runs as FREE, the
    # streams ride in every other test of this file)
    s.group_type = np.where(np.asarray(s.group_type) == M.LANGEVIN, M.FREE, np.asarray(s.group_type)).astype(np.int32)
    s.lcg64 = None
    s.name += "-nostreams"
    grid = s.grid
    single = single_domain(s, 1, vaf)
    g = MartiniGroup(s, grid)
    try:
        runs = []
        for attempt in range(2):
            if attempt:
                for r in g.ranks:
                    r.upload_local()
            g.eval_forces()
            if vaf:
                g.vaf_origin()
            frames = [_frame_group(g, s, vaf)]
            g.step(M.UPDATE)
            frames.append(_frame_group(g, s, vaf))
            runs.append(frames)
    finally:
        g.close()
    moved = (runs[0][1]["owner"] != runs[0][0]["owner"]).sum()
    assert moved == M.NCROWD > 1024
    for frames in runs:
        check_frames(s, grid, frames, single, s.name)
    for fa, fb in zip(*runs):
        for key in ("owner", "r", "v", "f", "species"):
            assert (fa[key] == fb[key]).all(), key


@pytest.mark.parametrize("grid,pbc", THREES, ids=ID3)
def test_a_hop_of_two_bricks_is_delivered_or_refused(grid, pbc):
    """Periodic, P = 3: brick 0 -> brick 2 is the other neighbour (dd = 2 folds to -1), delivered, and everything check_frames asks holds.
    Periodic, P = 4, and an open axis (brick 0 -> brick P - 1 and back): no neighbour -- the step must fail with DDCMI_EINVAL and
    "further than one domain" in the last error of EVERY domain's context (the emulation lets every domain classify and leaves the
    message on all of them, as the count round does between processes), and the contexts must still close.  On an open axis the fold by -+P used to turn the hop into a
    direction without destination: the bead was counted as leaving, copied nowhere, and the call SUCCEEDED with a bead gone (found by
    this test at (3,1,1) and (4,1,1) with pbc 6, (1,3,1) with pbc 5, (3,2,1) with pbc 6; k_mig_classify now folds on periodic axes only)."""
    s = M.system("two_hops", grid, pbc, passengers=True)
    if s.legal:
        frames = group_run(s, grid, 1)
        check_frames(s, grid, frames, single_domain(s, 1), s.name)
        assert (frames[1]["owner"] != frames[0]["owner"]).sum() == 16
        return
    g = MartiniGroup(s, grid)
    try:
        g.eval_forces()
        first = _frame_group(g, s, False)
        try:
            g.step(M.UPDATE)
        except DdcmiError as ex:
            assert "error %d:" % DDCMI_EINVAL in str(ex), str(ex)
            msgs = [g.lib.ddcmi_last_error(r.ctx).decode() for r in g.ranks]
            assert all("further than one domain" in m for m in msgs), msgs          # EVERY domain's context says so
        else:
            after = [r.download_particles()["gid"] for r in g.ranks]
            lost = np.setdiff1d(np.asarray(s.gid, np.uint64), np.concatenate(after))
            pytest.fail("the step succeeded after a hop of two bricks; %d of %d beads are gone" % (len(lost), s.natoms))
        assert first["nlocal"].sum() == s.natoms
    finally:
        g.close()          # the contexts of a failed step are destroyed cleanly


def test_crossers_between_real_processes():
    """(2,1,1), crossers with passengers, two processes over the host transport on one GPU: the same ownership and state.  (The refused
    two-hop is not run on this path: nothing here shows that both ranks leave the count round by the launcher's limit on the parent
    commit's behaviour.)"""
    grid = (2, 1, 1)
    s = M.system("crossers", grid, 7, passengers=True)
    single = single_domain(s, 2)
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, os.path.join(ROOT, "tests", "migration_worker.py"), d]
        run_ranks([cmd] * 2, [rank_env(r, 2, d) for r in range(2)], timeout=120, check=True)
        recs = [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(2)]
    box = M.box_of(s)
    snaps = M.snapshots(s, 2 * M.UPDATE)
    back = np.empty(s.natoms, int)
    back[_order(s)] = np.arange(s.natoms)
    for k in range(3):
        gid = np.concatenate([r["gid%d" % k] for r in recs])
        assert len(gid) == s.natoms and (np.sort(gid) == np.sort(np.asarray(s.gid, np.uint64))).all()
        o = np.argsort(gid, kind="stable")
        get = lambda key: np.concatenate([r["%s%d" % (key, k)] for r in recs])[o][back]
        owner = np.concatenate([np.full(len(r["gid%d" % k]), q) for q, r in enumerate(recs)])[o][back]
        pos = M.wrap64(get("r"), box, s.pbc)
        assert (owner == M.owner_exact(pos, box, grid, s.pbc)).all() and (owner == M.owner_exact(snaps[k], box, grid, s.pbc)).all()
        assert (pos == single[k]["r"]).all() and (get("v") == single[k]["v"]).all() and (get("f") == single[k]["f"]).all()
        assert (get("species") == np.asarray(s.species)).all()
        for key in ("state", "prime", "multID"):
            assert (get(key) == single[k]["lcg"][key]).all(), key


def test_crowd_with_streams_overflows_and_is_redone():
    """the redo of the classification with the LCG64 records riding in rec[8] / rec[9] of more than 1024 records in one direction (one
    pass in a fresh group: the first mig_cap is 1024), against the single domain"""
    s = M.system("crowd", "face", passengers=True)
    frames = group_run(s, s.grid, 1)
    assert (frames[1]["owner"] != frames[0]["owner"]).sum() == M.NCROWD > 1024
    check_frames(s, s.grid, frames, single_domain(s, 1), s.name)


@pytest.mark.parametrize("grid,pbc", [((2, 2, 2), 7), ((3, 2, 1), 6)], ids=["222-pbc7", "321-pbc6"])
def test_species_above_255_ride_along(grid, pbc):
    """300 species (the gas's two, repeated), every planted crosser with an id of 256 and more: the 16 bits of the species in the tag
    word of a migration record all count.  A download reads the species out of the tag word itself; what k_unpack_mig decoded shows
    in the physics -- ids of 256 and more are a quarter heavier, so a restrained or LANGEVIN bead taken for species id & 0xff has
    another velocity than the single domain's.  (No VAF here: its classes are limited in number.)"""
    s = M.many_species(M.system("crossers", grid, pbc, passengers=True))
    assert (np.asarray(s.species)[s.planted_all] >= 256).all()
    frames = group_run(s, grid, 2, vaf=False)
    check_frames(s, grid, frames, single_domain(s, 2, False), s.name)


def test_beads_that_crossed_come_back():
    """returners: FIXEDVELOCITY groups whose vectors are reversed after the first period -- every planted bead crosses the face x = 0
    or the periodic face and re-crosses it: the arrivals that k_unpack_mig appended leave again at the next rebuild.  Owners from the
    reference, positions bit for bit the reference's and the single domain's."""
    s = M.system("returners")
    grid = s.grid
    box = M.box_of(s)
    snaps = M.returners_reference(s)
    back = -np.asarray(s.group_v)
    m = MartiniHIP(s)
    g = MartiniGroup(s, grid)
    try:
        m.eval_forces()
        g.eval_forces()
        for k in range(3):
            if k:
                m.step(M.UPDATE)
                g.step(M.UPDATE)
            fg, fs = _frame_group(g, s, False), _frame_single(m, s, False)
            want = M.owner_exact(snaps[k], box, grid, s.pbc)
            assert (fg["owner"] == want).all(), k
            for key in ("r", "v", "f"):
                assert (fg[key] == fs[key]).all(), (k, key)
            assert (fg["r"] == snaps[k]).all() and (fg["species"] == np.asarray(s.species)).all(), k
            if k == 0:
                home = want.copy()
            pl = s.planted_all
            assert ((want[pl] != home[pl]) == (k == 1)).all() and (want == home)[np.setdiff1d(np.arange(s.natoms), pl)].all()
            if k == 1:
                m.set_group_velocity(s.group_vset, back)
                g.set_group_velocity(s.group_vset, back)
    finally:
        g.close()
        m.close()

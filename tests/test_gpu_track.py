"""GPU tests (-m gpu) of the FORCE_AVERAGE pass (ddcmi_track_set / _accumulate / _read): running sums of tracked beads that stay on
the device.  One domain bit for bit against the host's running sum of downloads, for every kind of list and at the bead counts
around a wave and a workgroup; nothing of the run changes on the lean, the fused and the unfused step path; reset, a new list and the
refusals; decomposed runs -- in-process bricks and two real processes -- whose tracked beads cross faces, an edge and the corner and
one of whose ranks empties, against a longdouble reference within the bound of the roundings."""
import os
import subprocess
import sys

import numpy as np
import pytest

import migration_systems as M
import restraint_systems as R
import track_systems as T
import track_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
# (beads, listed gids): every bead count with a list of its own size; one, two and more ids than beads; 1025 unique ids and more do not
# fit the staged pivots whole (stride 2, stride 4)
SHAPES = [(1, 1), (1, 2), (1, 9), (63, 63), (64, 64), (65, 65), (65, 2), (65, 200), (1025, 1), (1025, 64), (1025, 1025), (1025, 1500), (1025, 5000)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("update_rate", [10, 20])
@pytest.mark.parametrize("nbeads, nlist", SHAPES)
def test_one_domain_is_the_hosts_running_sum_bit_for_bit(nbeads, nlist, update_rate):
    """7 accumulations over 45 steps for each quantity; the cell sort of the rebuilds reorders the beads in between.  One add per sample
    and component in time order on the device, the same adds in float64 on the host: every bit agrees.  hits: 7 or 0."""
    from ddcmd_amd.martini import MartiniHIP
    s = T.gas(nbeads, update_rate)
    gids, present = T.tracked_list(s, nlist)
    idx = T.index_of(s, gids)
    assert np.array_equal(idx >= 0, present) and (present.any() or nlist < 2)
    m = MartiniHIP(s)
    try:
        m.eval_forces()
        rebuilds0 = m.list_stats()["rebuilds"]
        for what in T.WHATS:
            m.track_set(gids)
            ref = np.zeros((nlist, 3))
            for k in T.SCHEDULE:
                if k:
                    m.step(k)
                m.track_accumulate(what)
                ref += T.values(m.download(), what, idx)
            tot, hits = m.track_read()
            assert np.array_equal(hits, np.where(present, len(T.SCHEDULE), 0))
            assert np.array_equal(bits(tot), bits(ref)), (what, np.abs(tot - ref).max())
            if present.any() and (what != "force" or nlist >= nbeads):      # (force: of the restraints, on a few beads only)
                assert np.any(tot[present] != 0.0)
            assert np.all(tot[~present] == 0.0)
            again, _ = m.track_read()      # a read without reset changes nothing
            assert np.array_equal(bits(again), bits(tot))
        assert m.list_stats()["rebuilds"] - rebuilds0 >= 135 // update_rate - 1
    finally:
        m.close()


def _assert_twins(a, b, want_plan):
    assert a["en"].tobytes() == b["en"].tobytes()
    for k in ("r", "v", "f"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert [tuple(p) for p in a["plans"]] == [tuple(p) for p in b["plans"]] == [want_plan]
    assert set(np.unique(a["hits"])) <= {0, 2, 3} and a["hits"].max() == 3      # three accumulations, reset, two


@pytest.mark.parametrize("path", ["lean", "fused"])
def test_nothing_of_the_run_changes(path, monkeypatch):
    """energies behind every call and the download 20 steps later, byte for byte those of a twin that never tracked"""
    import ddcmd_amd
    if path == "fused":
        monkeypatch.setenv("DDCMI_NO_LEAN_STEP", "1")      # read when the context is made
    s = ddcmd_amd.make_water_setup(6)
    gids = T.tracked_list(s, 65)[0]
    _assert_twins(T.twin_run(s, True, gids), T.twin_run(s, False), (1, 1) if path == "lean" else (1, 0))


def test_nothing_of_the_run_changes_on_the_unfused_path(tmp_path):
    """DDCMI_NO_FUSED_STEP is read once per process: a child process, as tests/integrator_paths_worker.py"""
    out = str(tmp_path / "paths.npz")
    env = dict(os.environ, DDCMI_NO_FUSED_STEP="1")
    res = subprocess.run([sys.executable, os.path.join(HERE, "track_worker.py"), "paths", out], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "track_worker ok" in res.stdout, res.stderr[-3000:]
    d = dict(np.load(out))
    _assert_twins({k[2:]: v for k, v in d.items() if k.startswith("a_")}, {k[2:]: v for k, v in d.items() if k.startswith("b_")}, (0, 0))


def test_reset_new_list_and_refusals():
    from ddcmd_amd.martini import MartiniHIP, DdcmiError
    s = T.gas(65)
    gids, present = T.tracked_list(s, 65)
    m = MartiniHIP(s)
    try:
        m.track_set(gids)
        with pytest.raises(DdcmiError, match="ddcmi_track_accumulate needs forces"):      # no force evaluation yet
            m.track_accumulate("force")
        m.track_accumulate("velocity")      # (velocities and positions need none)
        assert np.array_equal(m.track_read()[1], present.astype(np.int64))
        m.eval_forces()
        with pytest.raises(DdcmiError, match="a window averages one quantity"):
            m.track_accumulate("force")
        with pytest.raises(DdcmiError, match="what = 3"):
            m.track_accumulate(3)
        tot, hits = m.track_read(reset=True)      # the refusals changed nothing; reset zeroes
        assert np.array_equal(hits, present.astype(np.int64)) and np.any(tot != 0.0)
        tot, hits = m.track_read()
        assert not hits.any() and not bits(tot).any()
        m.track_accumulate("force")      # the next window may hold another quantity
        m.track_accumulate("force")
        assert np.array_equal(m.track_read()[1], 2 * present)
        m.track_set(gids[:7])      # a new list zeroes
        tot, hits = m.track_read()
        assert tot.shape == (7, 3) and not hits.any() and not bits(tot).any()
        with pytest.raises(DdcmiError, match="n = 65, the tracked list has 7 gids"):
            m._ntrack = 65
            m.track_read()
        cap = 1 << 20
        with pytest.raises(DdcmiError, match="at most %d are tracked" % cap):
            m.track_set(np.zeros(cap + 1, np.uint64))
        assert m.lib.ddcmi_track_set(m.ctx, -1, None) == -2 and b"n = -1" in m.lib.ddcmi_last_error(m.ctx)
        assert m.lib.ddcmi_track_set(m.ctx, 3, None) == -2 and b"NULL gid" in m.lib.ddcmi_last_error(m.ctx)
        m._ntrack = 7
        m.track_accumulate("position")      # the refused lists left the list of seven in place
        assert np.array_equal(m.track_read()[1], present[:7].astype(np.int64))
        m.track_set([])      # n = 0 removes the list: an accumulation is a no-op that succeeds
        m.track_accumulate("force")
        assert m.track_read()[0].shape == (0, 3)
        m.step(12)      # the context still works
        m.track_set(gids)
        m.track_accumulate("position")
        d = m.download()
        assert np.array_equal(bits(m.track_read()[0]), bits(T.values(d, "position", T.index_of(s, gids)) + 0.0))
    finally:
        m.close()


# ---- decomposed ------------------------------------------------------------------------------------------------------------------
def _single_domain_reference(s, gids, what, schedule):
    """longdouble sums of the single-domain run's downloads at the samples, and the sums of the magnitudes"""
    from ddcmd_amd.martini import MartiniHIP
    idx = T.index_of(s, gids)
    ref, mag = np.zeros((len(gids), 3), np.longdouble), np.zeros((len(gids), 3), np.longdouble)
    m = MartiniHIP(s)
    try:
        m.eval_forces()
        for k in schedule:
            if k:
                m.step(k)
            x = T.values(m.download(), what, idx, np.longdouble)
            ref += x
            mag += np.abs(x)
    finally:
        m.close()
    return ref, mag, idx >= 0


def _group_window(s, grid, gids, what, schedule):
    from ddcmd_amd.martini import MartiniGroup
    g = MartiniGroup(s, grid)
    try:
        g.eval_forces()
        g.track_set(gids)
        owned = []
        for k in schedule:
            if k:
                g.step(k)
            g.track_accumulate(what)
            owned.append([int(r.lib.ddcmi_nlocal(r.ctx)) for r in g.ranks])
        tot, hits = g.track_read(per_rank=True)
        summed, _ = g.track_read()
        return tot, hits, summed, np.array(owned)
    finally:
        g.close()


def _assert_window(tot, hits, summed, ref, mag, present, nsamples, nranks, label):
    assert np.array_equal(hits.sum(axis=0), np.where(present, nsamples, 0)), label      # every gid: one owner at every sample
    acc = tot[0].copy()
    for r in range(1, nranks):
        acc += tot[r]
    assert np.array_equal(bits(acc), bits(summed))      # the rank-ordered sum
    err, bound = np.abs(summed.astype(np.longdouble) - ref), (nsamples + nranks) * U * mag      # that many roundings: derived, not measured
    print(label, "largest error / bound", float(np.max(err[mag > 0] / bound[mag > 0])) if (mag > 0).any() else 0.0)
    assert np.all(err <= bound), label
    return (hits > 0).sum(axis=0)      # ranks that owned the bead at some sample


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("what", ["position", "velocity"])
def test_bricks_whose_tracked_beads_cross_faces_edges_and_the_corner(grid, what):
    s = M.crossers(grid)
    gids = W.planted_list(s)
    sched = W.RANK_SCHEDULE
    nranks = grid[0] * grid[1] * grid[2]
    ref, mag, present = _single_domain_reference(s, gids, what, sched)
    tot, hits, summed, _ = _group_window(s, grid, gids, what, sched)
    nown = _assert_window(tot, hits, summed, ref, mag, present, len(sched), nranks, "%s %s" % (grid, what))
    # the planted movers changed owner inside the window: across a face, and on the 2x2x2 grid across an edge and the corner too
    idx = T.index_of(s, gids)
    for (rank, d, wave), beads in s.planted.items():
        moved = nown[np.isin(idx, beads)]
        assert moved.size == len(beads) and np.all(moved == 2), (rank, d, wave)
    kinds = {sum(1 for c in d if c) for (_, d, _) in s.planted}
    assert kinds == ({1} if nranks == 2 else {1, 2, 3})
    again = _group_window(s, grid, gids, what, sched)      # repeating the run gives identical bits
    assert again[0].tobytes() == tot.tobytes() and again[1].tobytes() == hits.tobytes()


def test_a_rank_that_empties_keeps_its_sums_and_adds_nothing_more():
    """(2, 1, 1), tests/restraint_systems.py's emptying system: the first domain hands its last bead over at the rebuild of step 20.  Forces
    (of the restraints) are tracked; the emptied rank's partial sums stay, and the window still adds up"""
    s = R.emptying(True)
    gid = np.asarray(s.gid, np.uint64)
    gids = np.concatenate([gid[s.cluster], gid[s.rest_bead[s.rest_bead >= 0]][:60], np.array([gid.max() + np.uint64(9)], np.uint64)])
    sched = (0, 5, 5, 10, 5, 10)
    ref, mag, present = _single_domain_reference(s, gids, "force", sched)
    tot, hits, summed, owned = _group_window(s, (2, 1, 1), gids, "force", sched)
    _assert_window(tot, hits, summed, ref, mag, present, len(sched), 2, "emptying force")
    assert owned[0, 0] > 0 and owned[-1, 0] == 0 and owned[-2, 0] == 0      # two samples on an empty rank
    k = np.isin(gids, gid[s.cluster])
    assert np.all(hits[0][k] > 0) and np.all(hits[1][k] > 0) and np.any(tot[0][k] != 0.0)


def test_two_processes_over_the_host_transport(tmp_path):
    from ranks import rank_env, run_ranks
    grid = (2, 1, 1)
    s = M.crossers(grid)
    gids = W.planted_list(s)
    d = str(tmp_path)
    cmd = [sys.executable, os.path.join(HERE, "track_worker.py"), "rank", "2x1x1", d]
    run_ranks([cmd] * 2, [rank_env(r, 2, d) for r in range(2)], timeout=300, check=True)
    out = [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(2)]
    tot, hits = np.stack([o["tot"] for o in out]), np.stack([o["hits"] for o in out])
    n = len(gids)
    summed = out[0]["both"][:3 * n].reshape(n, 3)
    assert np.array_equal(out[0]["both"], out[1]["both"]) and np.array_equal(out[0]["both"][3 * n:], hits.sum(axis=0))
    ref, mag, present = _single_domain_reference(s, gids, "position", W.RANK_SCHEDULE)
    nown = _assert_window(tot, hits, summed, ref, mag, present, len(W.RANK_SCHEDULE), 2, "two processes")
    assert (nown == 2).sum() >= len(s.planted_all)

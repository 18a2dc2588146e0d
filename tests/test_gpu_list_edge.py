"""GPU tests (-m gpu) of the list search's single-precision filter on the systems of tests/list_edge_systems.py: pairs within 3e-14 ... 1e-3
of the list radius on both sides, at both edges of the band of the exact test, at cell faces with partners two cells away, in the outer
ring of a tile's staged region, across periodic and domain faces, outside an open box.  k_tile_build drops a pair for a whole rebuild
period without a word; here the list is known pair by pair (tests/test_list_edge_systems_host.py proves that of the inputs) and is
compared as an exact set.  docs/list_edge_variants.md lists the systems, the instantiations reached and the mutations tried."""
import numpy as np
import pytest

import approach_systems as A
import list_edge_systems as E

pytestmark = pytest.mark.gpu
TIGHT = 1e-10       # max |f - f_ref| / max |f_ref| (tests/test_gpu_molecules.py)
CASES = [(n, "one_type") for n in E.GAS] + [("sweep", "types20"), ("sweep", "mol"), ("nudged_water", "one_type")]


def device_list(m):
    start, j = m.get_list(0)
    i = np.repeat(np.arange(m.n), np.diff(start))
    return set(zip(i.tolist(), j.tolist()))


def assert_list(s, m, name, variant, tag=""):
    ref = E.exact_list(name, variant)
    got = device_list(m)
    missing, extra = ref - got, got - ref
    if missing or extra:
        print("%s %s %s: %d missing\n%s\n%d extra\n%s" % (name, variant, tag, len(missing), E.describe(s, missing), len(extra), E.describe(s, extra)))
    assert not missing and not extra, (name, variant, tag, len(missing), len(extra))
    st = m.list_stats()
    assert st["entries"] == len(ref), (st["entries"], len(ref))
    assert st["excluded"] == 2 * E.excluded_pairs(s), (st["excluded"], E.excluded_pairs(s))
    return st


@pytest.mark.parametrize("name,variant", CASES)
def test_list_is_the_exact_list(name, variant):
    """one domain: the restated grid is the device's (cells), the pair set equals the reference set, entries = twice the pairs, excluded = the
    molecules' pairs.  A failure prints family, e, direction and cell offset of every missing or extra pair"""
    from ddcmd_amd.martini import MartiniHIP
    s = E.system(name, variant)
    m = MartiniHIP(s)
    m.eval_forces()
    st = assert_list(s, m, name, variant)
    assert st["cells"] == E.grid_of(s).ncell, (st["cells"], E.grid_of(s).ncell)
    m.close()


@pytest.mark.parametrize("name,variant", [("sweep", "one_type"), ("sweep", "types20"), ("prune_exact", "one_type"), ("noncubic", "one_type"), ("open", "one_type")])
def test_forces_of_the_gas(name, variant):
    """after the same build: forces against the all-pairs longdouble reference (LJ + reaction field) within 1e-10 of the largest"""
    from ddcmd_amd.martini import MartiniHIP
    s = E.system(name, variant)
    m = MartiniHIP(s)
    m.eval_forces()
    f = np.stack(m.download()["f"], 1)
    m.close()
    ref = np.asarray(reference_forces(s), np.float64)
    scale = np.abs(ref).max()
    err = np.abs(f - ref).max() / scale
    print("%s %s: max |f - f_ref| / max |f_ref| = %.2e" % (name, variant, err))
    assert scale > 0 and err <= TIGHT, (name, err)


def reference_forces(s):
    """approach_systems.reference_forces under the box's own periodicity mask (it takes every axis for periodic: an open axis is given a
    period no pair can reach)"""
    import copy
    t = copy.copy(s)
    r = E.positions(s)
    h = np.array(s.h, float)
    for a in range(3):
        if not (s.pbc >> a) & 1:
            h[4 * a] = 4.0 * (np.abs(r[:, a]).max() + s.rmax)
    t.h = h
    return A.reference_forces(t, r)


def test_list_after_a_build_started_over(monkeypatch, capfd):
    """a clump of 448 beads in a dilute gas: the rows (24 words) and the staging (384 beads) the build starts with are too small, it grows
    both and starts over -- more launches of the build (phase 11) than builds completed (phase 13); the build's report names the capacities
    it ended with: staging beyond the clump's 448 beads, rows that hold the longest row of the exact list, in the range of k_tile_transpose<6, true> -- and the list is exact on the restated grid"""
    from ddcmd_amd.martini import MartiniHIP
    from test_gpu_molecules import build_attempts
    s = E.system("crowded")
    monkeypatch.setenv("DDCMI_DEBUG_PHASES", "1")
    monkeypatch.setenv("DDCMI_DEBUG_SCHED", "1")
    m = MartiniHIP(s)
    m.eval_forces()
    monkeypatch.delenv("DDCMI_DEBUG_PHASES")
    monkeypatch.delenv("DDCMI_DEBUG_SCHED")
    st = assert_list(s, m, "crowded", "one_type", "started over")
    assert st["cells"] == E.grid_of(s).ncell
    report = [l for l in capfd.readouterr().err.splitlines() if l.startswith("ddcmi build:")]
    m.close()
    launches, builds = build_attempts(capfd.readouterr().err)
    print("crowded: %d launches of the build for %d build; %s" % (launches, builds, report))
    assert builds == 1 and launches >= 3, (launches, builds)
    assert len(report) == 1, report
    w = report[0].split()
    stage_cap, tmpw, pack = (int(w[w.index(k) + 1]) for k in ("stage_cap", "tmpw", "pack_type"))
    longest = int(np.bincount([i for i, _ in E.exact_list("crowded")]).max())          # the longest row of the exact list
    assert stage_cap > 448 and 192 < longest <= tmpw <= 384 and pack == 2, (report, longest)


def domain_counts(s, grid):
    """ordered pairs of the exact list by the domain that owns the first bead: what each member's `entries` must be"""
    from ddcmd_amd.martini import domain_of
    owner = domain_of(s, grid)
    out = np.zeros(grid[0] * grid[1] * grid[2], np.int64)
    for i, _ in E.exact_list(s.name):
        out[owner[i]] += 1
    return out


@pytest.mark.parametrize("name", ["sweep", "face_cell"])
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_entries_and_forces_of_a_group(grid, name):
    """in-process domains: pairs straddle every internal face (the partner is a received halo bead, some exactly on the face: halo_cell's side
    forcing places them).  A member's list names a received bead by its place in the receive buffer, a negative number that ddcmi_get_list would
    use as an index: the lists are not read.  Every member's `entries` equals the number of ordered pairs of the exact list whose first bead
    it owns -- the rows of the pairs across a face are one entry short on each side if the partner is lost -- and the gathered forces match.
    "face_cell": the received bead lies exactly on the member's high face and an owned bead sits in the cell next to it: filed without the
    side forcing it shares that cell, the cell keeps its owned range alone, and two rows of the site lose an entry"""
    from ddcmd_amd.martini import MartiniGroup
    s = E.system(name)
    want = domain_counts(s, grid)
    r = E.positions(s)
    for a in range(3):          # every internal face has list pairs across it, in both directions
        if grid[a] == 2:
            assert sum(1 for i, j in E.exact_list(name) if r[i, a] < 0 <= r[j, a] and abs(r[i, a] - r[j, a]) < E.rlist_of(s)) >= (6 if name == "sweep" else 2)
    g = MartiniGroup(s, grid)
    g.eval_forces()
    entries = np.array([m.list_stats()["entries"] for m in g.ranks])
    cells = [m.list_stats()["cells"] for m in g.ranks]
    p = g.gather()
    g.close()
    print("group %s: entries %s, reference %s" % (grid, entries.tolist(), want.tolist()))
    assert np.array_equal(entries, want), (entries.tolist(), want.tolist())
    px, py, pz = grid
    for k, c in enumerate(cells):
        assert c == E.grid_of(s, grid, (k % px, (k // px) % py, k // (px * py))).ncell
    assert np.array_equal(p["gid"], np.asarray(s.gid))
    ref = np.asarray(reference_forces(s), np.float64)
    err = np.abs(np.stack(p["f"], 1) - ref).max() / np.abs(ref).max()
    assert err <= TIGHT, err


def test_entries_and_forces_of_a_loopback_rank(monkeypatch):
    """a single rank behind the RCCL loopback transport: every image is a received bead"""
    from test_gpu_rccl_loopback import _loopback_rank
    s = E.system("sweep")
    m = _loopback_rank(s, monkeypatch)
    m.eval_forces()
    entries = m.list_stats()["entries"]
    p = m.download_particles()
    m.close()
    assert entries == len(E.exact_list("sweep")), (entries, len(E.exact_list("sweep")))
    order = np.argsort(p["gid"], kind="stable")
    ref = np.asarray(reference_forces(s), np.float64)
    err = np.abs(np.stack([p["f"][c][order] for c in range(3)], 1) - ref).max() / np.abs(ref).max()
    assert err <= TIGHT, err

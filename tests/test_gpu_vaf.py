"""GPU tests (-m gpu) of ANALYSIS VELOCITYAUTOCORRELATION on the device (ddcmi_vaf_origin / ddcmi_vaf_sample / ddcmi_vaf_clear and
the in-process group's twins).

The yardstick is velocityAutocorrelation_eval's sums restated in numpy / longdouble (HostRef), fed by trajectories obtained
independently of the records under test: positions and velocities downloaded at every sample, positions unwrapped on the host by
minimum image between consecutive downloads (the sample interval is short: no bead moves half a box side in it).

Tolerance, per class: |got - want| <= 1e-10 * sum |terms| with the terms v0.v or d.d of the longdouble reference.  Differencing
positions of magnitude <= L ~ 1e2..1e3 bohr leaves d with an absolute error of a few 1e-13 bohr per correction, another summation
order adds ~ sqrt(N) eps relatively: both orders below 1e-10.  One missed wrap is an error of ~ L^2 in one term against
sum d^2 ~ N (1 bohr)^2: far above the bound at these sizes.  sum |terms| and not |sum|: the VAF's sum passes through zero."""
import os

import numpy as np
import pytest

from ddcmd_amd.deck import load_deck, units_convert
from ddcmd_amd.synth import make_water_setup

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REF_WATER = os.path.join(HERE, "golden", "ref_waterbox")
LIPID_DIR = os.path.join(HERE, "golden", "lipid_deck")
LIPID_DECK = os.path.join(LIPID_DIR, "object.data")
RTOL = 1e-10
LD = np.longdouble


class HostRef(object):
    """velocityAutocorrelation_eval's sums from downloaded states.  group / species: per bead, in the order of the arrays fed"""

    def __init__(self, ngroup, nspecies, group, species, pbc=7):
        self.ng, self.ns, self.pbc = int(ngroup), int(nspecies), int(pbc)
        self.group, self.species = np.asarray(group, np.int64), np.asarray(species, np.int64)
        self.crossings = 0
        self.rprev = None

    def _min_image(self, step, L):
        for a in range(3):
            if (self.pbc >> a) & 1:
                k = np.rint(step[:, a] / L[a])
                self.crossings += int(np.count_nonzero(k))
                step[:, a] -= L[a] * k
        return step

    def origin(self, r, v):
        self.v0 = np.array(v, dtype=np.float64)
        self.d = np.zeros_like(self.v0)
        self.rprev = np.array(r, dtype=np.float64)

    def advance(self, r, L, lam=None):
        """the drift moves since the last state fed: minimum image of r - lam * r_prev (lam: the barostat's scale factors)"""
        r = np.array(r, dtype=np.float64)
        prev = self.rprev if lam is None else self.rprev * np.asarray(lam)[None, :]
        self.d += self._min_image(r - prev, np.asarray(L, dtype=np.float64))
        self.rprev = r

    def sums(self, v):
        """(vaf, msd, sum |vaf terms|, sum |msd terms|) per class, longdouble"""
        v = np.asarray(v, dtype=np.float64)
        a = (self.v0.astype(LD) * v.astype(LD)).sum(axis=1)
        b = (self.d.astype(LD) * self.d.astype(LD)).sum(axis=1)
        ncl = 1 + self.ng + self.ns
        out = [np.zeros(ncl, LD) for _ in range(4)]
        masks = [np.ones(len(a), bool)] + [self.group == g for g in range(self.ng)] + [self.species == s for s in range(self.ns)]
        for c, m in enumerate(masks):
            out[0][c], out[1][c], out[2][c], out[3][c] = a[m].sum(), b[m].sum(), np.abs(a[m]).sum(), b[m].sum()
        return out


def assert_close(got, ref, what=""):
    vaf, msd = got
    wv, wm, av, am = ref
    assert len(vaf) == len(wv) and len(msd) == len(wm)
    ev, em = np.abs(vaf.astype(LD) - wv), np.abs(msd.astype(LD) - wm)
    print("%s vaf err/bound %.3e msd err/bound %.3e" % (what, float(np.max(ev / np.maximum(RTOL * av, 1e-300))), float(np.max(em / np.maximum(RTOL * am, 1e-300)))))
    assert np.all(ev <= RTOL * av), (what, vaf, wv)
    assert np.all(em <= RTOL * am), (what, msd, wm)


def _state(m):
    d = m.download()
    return np.stack(d["r"], axis=1), np.stack(d["v"], axis=1)


def _gstate(g):
    d = g.gather()
    return np.stack(d["r"], axis=1), np.stack(d["v"], axis=1), d


def _two_groups(s, gtype, split_species):
    """two groups of the given type: beads of species >= split_species form group 1"""
    s.ngroup = 2
    s.group = (np.asarray(s.species) >= split_species).astype(np.int32)
    s.group_type = np.array([gtype, gtype], np.int32)
    s.group_Teq = np.array([units_convert(310.0, "K")] * 2)
    s.group_tau = np.array([units_convert(1.0, "ps")] * 2)
    s.group_interval = np.ones(2, np.int32)
    s.group_vcm = None
    s.npt_beta = 0.0      # the thermostat alone: the box stays
    return s


def _windowed_run(m, s, nsamples, every, length, ref=None, state=_state, box=None):
    """origin, then a sample every `every` steps, a new origin after `length` samples; every sample held against HostRef"""
    ref = ref or HostRef(max(1, s.ngroup), s.nspecies, s.group, s.species, s.pbc)
    box = box or (lambda: s.h[[0, 4, 8]])
    r, v = state(m)[:2]
    m.vaf_origin()
    ref.origin(r, v)
    vaf, msd = m.vaf_sample()
    assert np.all(msd == 0.0)
    assert_close((vaf, msd), ref.sums(v), "origin")
    k = 0
    for it in range(nsamples):
        m.step(every)
        r, v = state(m)[:2]
        ref.advance(r, box())
        k += 1
        assert_close(m.vaf_sample(), ref.sums(v), "sample %d k=%d" % (it, k))
        if k == length:
            m.vaf_origin()
            ref.origin(r, v)
            assert_close(m.vaf_sample(), ref.sums(v), "re-origin %d" % it)
            k = 0
    return ref


def test_reference_waterbox_nglf_windows_over_rebuilds(monkeypatch):
    from ddcmd_amd.martini import MartiniHIP
    monkeypatch.chdir(REF_WATER)
    s = load_deck("object.data")
    s.npt_beta = 0.0      # NGLF: no barostat
    m = MartiniHIP(s)
    m.eval_forces()
    r0 = m.list_stats()["rebuilds"]
    ref = _windowed_run(m, s, 20, 10, 5)
    assert m.list_stats()["rebuilds"] > r0
    assert ref.crossings > 0      # a bead crossed a periodic face: the wrap correction was exercised
    m.close()


def test_lipid_deck_groups_and_species_berendsen():
    from ddcmd_amd.martini import MartiniHIP
    s = _two_groups(load_deck(LIPID_DECK), 1, 9)
    assert s.nspecies == 19 and len(np.unique(s.species)) >= 10 and len(np.unique(s.group)) == 2
    m = MartiniHIP(s)
    m.eval_forces()
    m.group_temperatures()
    ref = _windowed_run(m, s, 8, 5, 4)
    # class order: 0 the system, 1 + g, 1 + ngroup + s -- classes without beads are zero, the groups' and the species' blocks add up to the system
    vaf, msd = m.vaf_sample()
    assert len(vaf) == 1 + 2 + 19
    present = np.bincount(s.species, minlength=19) > 0
    assert np.all((msd[3:] > 0) == present) or np.all(msd == 0)
    m.step(3)
    vaf, msd = m.vaf_sample()
    assert np.all((msd[3:] > 0) == present)
    assert abs(msd[1:3].sum() - msd[0]) <= 1e-12 * msd[0] and abs(msd[3:].sum() - msd[0]) <= 1e-12 * msd[0]
    m.close()


def test_nglfconstraint_barostat_scaling_is_no_displacement():
    from ddcmd_amd.martini import MartiniHIP
    from test_oracle import CONSTRAINT_X
    s = load_deck(os.path.join(LIPID_DIR, "object_nvt.data"), restart_file=os.path.join(LIPID_DIR, "relaxed", "restart"), extra_objects=CONSTRAINT_X)
    s.npt_T = units_convert(310.0, "K")
    s.npt_P0 = units_convert(1.0, "bar")
    s.npt_beta = units_convert(3.0e-4, "1/bar") * 50.0      # exaggerated compressibility: the box moves visibly
    s.npt_tau = units_convert(1.0, "ps")
    m = MartiniHIP(s, constraints=True)
    m.eval_forces()
    m.group_temperatures()
    ref = HostRef(max(1, s.ngroup), s.nspecies, s.group, s.species, s.pbc)
    r, v = _state(m)
    m.vaf_origin()
    ref.origin(r, v)
    L0 = m.box().copy()
    for it in range(40):
        Lb = m.box().copy()
        m.step(1)
        La = m.box().copy()
        r, v = _state(m)
        ref.advance(r, La, lam=La / Lb)
        if it % 4 == 3:
            assert_close(m.vaf_sample(), ref.sums(v), "step %d" % it)
    assert np.abs(m.box() - L0).max() > 1e-5 * L0.max()      # the box really changed
    m.close()


def test_langevin_group_counter_based_stream():
    from ddcmd_amd.martini import MartiniHIP
    s = make_water_setup(10)
    s.group_type = np.array([2], np.int32)
    s.group_Teq = np.array([units_convert(310.0, "K")])
    s.group_tau = np.array([units_convert(1.0, "ps")])
    m = MartiniHIP(s)
    m.eval_forces()
    _windowed_run(m, s, 10, 10, 5)
    m.close()


def test_host_integrator_mode_upload_positions():
    """origin, then upload_positions with positions wrapped into the box by the host: the MSD is the host's unwrapped displacement"""
    from ddcmd_amd.martini import MartiniHIP
    s = make_water_setup(8)
    L = s.h[[0, 4, 8]]
    m = MartiniHIP(s)
    m.eval_forces()
    r, v = _state(m)
    m.vaf_origin()
    ref = HostRef(1, s.nspecies, s.group, s.species, s.pbc)
    ref.origin(r, v)
    rng = np.random.RandomState(7)
    unwrapped = r.copy()
    for it in range(6):
        # a common move of a good tenth of the box (faces are crossed, no two beads approach each other) and a small one of each bead
        unwrapped += np.array([0.13, -0.07, 0.11])[None, :] * L[None, :] + rng.uniform(-0.05, 0.05, size=r.shape)
        w = unwrapped - L[None, :] * np.rint(unwrapped / L[None, :])
        m.upload_positions([np.ascontiguousarray(w[:, a]) for a in range(3)])
        ref.advance(w, L)
        m.eval_forces()      # (a rebuild may follow: the wrap of the new positions is no displacement either)
        got = m.vaf_sample()
        assert_close(got, ref.sums(v), "upload %d" % it)
        want = ((unwrapped - r) ** 2).sum()
        assert abs(got[1][0] - want) <= 1e-9 * want
    assert ref.crossings > 0
    m.close()


@pytest.mark.parametrize("grid", [(2, 2, 2), (2, 2, 1)])
def test_decomposed_records_migrate_with_their_beads(grid):
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP
    s = make_water_setup(15)
    by_gid = np.argsort(s.gid, kind="stable")
    g = MartiniGroup(s, grid)
    m = MartiniHIP(s)
    g.eval_forces()
    m.eval_forces()
    ref = HostRef(1, s.nspecies, np.asarray(s.group)[by_gid], np.asarray(s.species)[by_gid], s.pbc)
    r, v, d0 = _gstate(g)
    g.vaf_origin()
    m.vaf_origin()
    ref.origin(r, v)
    L = s.h[[0, 4, 8]]
    k = 0
    for it in range(8):
        g.step(10)
        m.step(10)
        r, v, d = _gstate(g)
        ref.advance(r, L)
        k += 1
        pv, pm = g.vaf_sample(per_rank=True)
        tot = g.vaf_sample()
        one = m.vaf_sample()
        assert pv.shape == (g.n, 1 + 1 + s.nspecies)
        assert np.allclose(pv.sum(axis=0), tot[0], rtol=1e-13, atol=0) and np.allclose(pm.sum(axis=0), tot[1], rtol=1e-13, atol=0)
        want = ref.sums(v)
        assert_close(tot, want, "group %d" % it)
        assert_close(one, want, "one domain %d" % it)      # (same tolerance: both within it of the reference, and of each other within twice it)
        assert np.all(np.abs(tot[0] - one[0]) <= 2 * RTOL * want[2].astype(np.float64)) and np.all(np.abs(tot[1] - one[1]) <= 2 * RTOL * want[3].astype(np.float64))
        if k == 4:
            g.vaf_origin()
            m.vaf_origin()
            ref.origin(r, v)
            k = 0
    assert d["nlocal"] != d0["nlocal"]      # beads migrated
    assert ref.crossings > 0
    g.close()
    m.close()


def test_records_through_rccl_loopback(monkeypatch):
    """one rank whose periodic neighbours are reached through RCCL: the wrap of the migration round corrects the records, the
    exchange runs for real"""
    import ctypes
    from ddcmd_amd.martini import MartiniRank, _declare_domains
    s = make_water_setup(12)
    monkeypatch.setenv("DDCMI_RCCL_LOOPBACK", "1")
    m = MartiniRank(s, np.arange(s.natoms))
    _declare_domains(m.lib)
    buf = ctypes.create_string_buffer(128)
    assert m.lib.ddcmi_comm_unique_id(buf) == 0
    m.comm_init(0, 1, buf.raw, (1, 1, 1))
    m.upload_local()
    m.eval_forces()
    by_gid = np.argsort(s.gid, kind="stable")

    def state(mm):
        p = mm.download_particles()
        o = np.argsort(p["gid"], kind="stable")
        return np.stack([p["r"][c][o] for c in range(3)], axis=1), np.stack([p["v"][c][o] for c in range(3)], axis=1)

    ref = HostRef(1, s.nspecies, np.asarray(s.group)[by_gid], np.asarray(s.species)[by_gid], s.pbc)
    ref = _windowed_run(m, s, 8, 10, 4, ref=ref, state=state)
    assert ref.crossings > 0
    m.close()


def test_records_between_two_processes_over_the_host_transport():
    """two real processes (tests/mp_vaf_worker.py), the migration records carried by the host-staged TCP transport: windows over
    rebuilds, beads change rank; the ranks' sums against the numpy reference and the one-domain run"""
    import sys
    import tempfile
    from ddcmd_amd.martini import MartiniHIP
    from ranks import rank_env, run_ranks
    nsamples, every, length = 12, 10, 4
    with tempfile.TemporaryDirectory() as d:
        cmd = [sys.executable, os.path.join(HERE, "mp_vaf_worker.py"), "2x1x1", d, str(nsamples), str(every), str(length)]
        run_ranks([cmd] * 2, [rank_env(r, 2, d) for r in range(2)], timeout=600, check=True)
        ranks = [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(2)]
    s = make_water_setup(12)
    by_gid = np.argsort(s.gid, kind="stable")
    assert all(int(rk["rebuilds"][0]) > 1 for rk in ranks)

    def merged(tag):
        gid = np.concatenate([rk["gid_" + tag] for rk in ranks])
        o = np.argsort(gid, kind="stable")
        assert np.array_equal(gid[o], np.sort(s.gid))
        r = np.concatenate([rk["r_" + tag] for rk in ranks], axis=1)[:, o].T
        v = np.concatenate([rk["v_" + tag] for rk in ranks], axis=1)[:, o].T
        tot = (ranks[0]["vaf_" + tag] + ranks[1]["vaf_" + tag], ranks[0]["msd_" + tag] + ranks[1]["msd_" + tag])
        return r, v, tot

    ref = HostRef(1, s.nspecies, np.asarray(s.group)[by_gid], np.asarray(s.species)[by_gid], s.pbc)
    L = s.h[[0, 4, 8]]
    m = MartiniHIP(s)
    m.eval_forces()
    m.vaf_origin()
    r, v, tot = merged("o0")
    ref.origin(r, v)
    assert np.all(tot[1] == 0.0)
    assert_close(tot, ref.sums(v), "two ranks, origin")
    k = 0
    for it in range(nsamples):
        m.step(every)
        r, v, tot = merged("s%d" % it)
        ref.advance(r, L)
        k += 1
        want = ref.sums(v)
        assert all(len(rk["gid_s%d" % it]) > 0 for rk in ranks)      # both ranks own beads
        assert_close(tot, want, "two ranks, sample %d" % it)
        one = m.vaf_sample()
        assert_close(one, want, "one domain, sample %d" % it)
        if k == length:
            m.vaf_origin()
            r, v, tot = merged("o%d" % (it + 1))
            ref.origin(r, v)
            assert_close(tot, ref.sums(v), "two ranks, re-origin %d" % it)
            k = 0
    m.close()
    for rk in ranks:      # beads changed rank
        assert not np.array_equal(np.sort(rk["gid_o0"]), np.sort(rk["gid_s%d" % (nsamples - 1)]))
    assert ref.crossings > 0


def _snapshot(m):
    d = m.download()
    e, vir, rk, tion = m.energies()
    return [np.concatenate(d["r"]), np.concatenate(d["v"]), np.concatenate(d["f"]), np.array([e[k] for k in sorted(e)]), vir, np.array([rk]), tion]


@pytest.mark.parametrize("kind", ["water", "lipid"])
def test_tracking_leaves_the_run_unchanged_one_domain(kind):
    """water: the lean, fused step; lipid: bonded terms.  And two identical tracked runs give identical sums"""
    from ddcmd_amd.martini import MartiniHIP
    s = make_water_setup(8) if kind == "water" else load_deck(LIPID_DECK)
    runs, sums = [], []
    for tracked in (False, True, True):
        m = MartiniHIP(s)
        m.eval_forces()
        got = []
        for k in range(6):
            if tracked and k % 3 == 0:
                m.vaf_origin()
            m.step(7)
            if tracked:
                got.append(np.concatenate(m.vaf_sample()))
        runs.append(_snapshot(m))
        sums.append(got)
        m.close()
    for x, y, z in zip(*runs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))
    assert len(sums[1]) == 6
    for a, b in zip(sums[1], sums[2]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_tracking_leaves_the_run_unchanged_2x2x2():
    from ddcmd_amd.martini import MartiniGroup
    s = make_water_setup(15)
    runs, sums = [], []
    for tracked in (False, True, True):
        g = MartiniGroup(s, (2, 2, 2))
        g.eval_forces()
        got = []
        if tracked:
            g.vaf_origin()
        for k in range(5):
            g.step(9)
            if tracked:
                got.append(np.concatenate([a.ravel() for a in g.vaf_sample(per_rank=True)]))
        d = g.gather()
        e, vir, rk, tion = g.energies()
        runs.append([np.concatenate(d["r"]), np.concatenate(d["v"]), np.concatenate(d["f"]), np.array([e[k] for k in sorted(e)]), vir, np.array([rk])])
        sums.append(got)
        g.close()
    for x, y, z in zip(*runs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))
    for a, b in zip(sums[1], sums[2]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_clear_and_upload_state_drop_the_records():
    from ddcmd_amd.martini import MartiniHIP, DdcmiError
    s = make_water_setup(6)
    m = MartiniHIP(s)
    m.eval_forces()
    m.vaf_origin()
    m.step(3)
    vaf, msd = m.vaf_sample()
    assert msd[0] > 0
    m.vaf_clear()
    with pytest.raises(DdcmiError, match="no time origin"):
        m.vaf_sample()
    m.vaf_origin()
    assert np.all(m.vaf_sample()[1] == 0.0)
    m.upload(s.rx, s.ry, s.rz, s.vx, s.vy, s.vz)
    with pytest.raises(DdcmiError, match="no time origin"):
        m.vaf_sample()
    m.eval_forces()
    m.vaf_origin()
    m.step(2)
    assert m.vaf_sample()[1][0] > 0
    m.close()


def test_wrong_arguments_are_refused_and_the_context_stays_usable():
    from ddcmd_amd.martini import MartiniHIP, MartiniGroup, DdcmiError, _d
    s = make_water_setup(6)
    m0 = MartiniHIP(s, upload=False)
    with pytest.raises(DdcmiError, match="uploaded state"):
        m0.vaf_origin()
    with pytest.raises(DdcmiError, match="uploaded state"):
        m0.vaf_sample()
    m0.close()
    m = MartiniHIP(s)
    m.eval_forces()
    with pytest.raises(DdcmiError, match="no time origin"):
        m.vaf_sample()
    m.vaf_origin()
    m.step(2)
    before = np.concatenate(m.vaf_sample())
    vaf, msd = np.zeros(8), np.zeros(8)
    for args, msg in (((2, s.nspecies, _d(vaf), _d(msd)), b"ngroup = 2"), ((1, s.nspecies + 1, _d(vaf), _d(msd)), b"nspecies"),
                      ((1, s.nspecies, None, _d(msd)), b"NULL"), ((1, s.nspecies, _d(vaf), None), b"NULL")):
        rc = m.lib.ddcmi_vaf_sample(m.ctx, *args)
        assert rc != 0 and msg in m.lib.ddcmi_last_error(m.ctx), (args, m.lib.ddcmi_last_error(m.ctx))
        assert np.all(vaf == 0.0) and np.all(msd == 0.0)
    assert m.lib.ddcmi_vaf_origin(None) != 0 and m.lib.ddcmi_vaf_sample(None, 1, 1, _d(vaf), _d(msd)) != 0 and m.lib.ddcmi_vaf_clear(None) != 0
    after = np.concatenate(m.vaf_sample())      # a refused call changed nothing
    assert np.array_equal(before.view(np.uint8), after.view(np.uint8))
    m.step(2)
    assert m.vaf_sample()[1][0] > before[len(before) // 2]
    m.close()
    g = MartiniGroup(make_water_setup(15), (2, 1, 1))
    g.eval_forces()
    r0 = g.ranks[0]
    with pytest.raises(DdcmiError, match="in-process group"):
        r0.vaf_origin()
    g.vaf_origin()
    with pytest.raises(DdcmiError, match="in-process group"):
        r0.vaf_sample()
    assert np.all(g.vaf_sample()[1] == 0.0)
    with pytest.raises(DdcmiError, match="in-process group"):      # one domain alone must not drop its records
        r0.vaf_clear()
    g.step(25)
    assert g.vaf_sample()[1][0] > 0
    g.vaf_clear()
    with pytest.raises(DdcmiError, match="no time origin"):
        g.vaf_sample()
    g.step(25)      # and the run goes on, with the plain migration records
    g.close()

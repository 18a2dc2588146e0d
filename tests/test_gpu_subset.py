"""GPU tests (-m gpu) of subsetWrite's binaryCharmm records on the device: ddcmi_subset_records and the in-process group's twin, on
small synthetic states uploaded directly (internal units; no list is built), on a water box that runs, and on the lipid deck.

The expected records are an independent numpy restatement (`expect`) of rejectParticle (subsetWrite.c:532-564) and of the record
arithmetic (subsetWrite.c:497-507: the difference and the product in double, one rounding to float), applied to what
ddcmi_download_particles returns; the device's bytes must equal them, record for record and in that order.

Bead counts: 1, 63, 64, 65 (a wave and its edges), 255, 256, 257 (a workgroup and its edges), 549 (three workgroups, the last one
ragged), and 262444: above 262144 beads a workgroup's range is more than one block of 256, the only size at which the offset carried
from block to block inside a workgroup, and a scan lane with more than one workgroup, are exercised."""
import ctypes

import numpy as np
import pytest

from ddcmd_amd.deck import Setup, units_convert
from ddcmd_amd.synth import water_forcefield, splitmix64

pytestmark = pytest.mark.gpu
EINVAL = -2
BOX = (64.0, 72.0, 96.0)
COUNTS = [1, 63, 64, 65, 255, 256, 257, 549, 262444]
REC = np.dtype([("id", "<u8"), ("pinfo", "<u4"), ("r", "<f4", (3,))])
GID_MAX = 2 ** 64 - 1


def _rand(n, stream):
    bits = splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(1000003 * (stream + 1))) >> np.uint64(11)
    return bits.astype(np.float64) / 9007199254740992.0


def synthetic(n, box=BOX, pbc=7):
    """n beads of two species and two groups in an orthorhombic box; gids 3 i + 1 (odd and even, multiples of 2 and not), not in slot order"""
    s = water_forcefield(Setup())
    s.h = np.diag(box).ravel().astype(np.float64)
    s.pbc = pbc
    s.nspecies = 2
    s.species_name = ["S0", "S1"]
    s.mass = units_convert(72.0, "M_p") * np.ones(2)
    s.charge = np.zeros(2)
    s.ljtype = s.moltype = s.resitype = np.zeros(2, np.int32)
    s.atomoffset = np.zeros(2, np.int32)
    s.ngroup = 2
    s.group_name = ["G0", "G1"]
    s.group_type = np.zeros(2, np.int32)
    s.group_Teq = np.zeros(2)
    s.group_tau = np.zeros(2)
    s.group_interval = np.ones(2, np.int32)
    s.natoms = n
    i = np.arange(n)
    s.species = ((i * 7 + i // 5) % 2).astype(np.int32)
    s.group = ((i // 3) % 2).astype(np.int32)
    s.gid = (3 * ((i * 7919) % n) + 1).astype(np.uint64) if n % 7919 else (3 * i + 1).astype(np.uint64)
    assert len(np.unique(s.gid)) == n
    s.rx, s.ry, s.rz = ((_rand(n, k) - 0.5) * box[k] for k in range(3))
    s.vx, s.vy, s.vz = ((_rand(n, 3 + k) - 0.5) * 2e-3 for k in range(3))
    return s


def particles(m):
    from ddcmd_amd.martini import DomainMixin
    return DomainMixin.download_particles(m)


def expect(p, group_of_gid, corner, cL=1.0, idmin=0, idmax=GID_MAX, modulus=1, odd=False, rmin=None, rmax=None, vmin=None, vmax=None, species=None,
           id_list=None, group_term=None, species_term=None, ngroup=2):
    """the records of the beads p (download_particles) the filter keeps, in p's order"""
    gid = np.asarray(p["gid"], np.uint64)
    r, v, sp = [np.asarray(a, np.float64) for a in p["r"]], [np.asarray(a, np.float64) for a in p["v"]], np.asarray(p["species"])
    reject = (gid < np.uint64(idmin)) | (gid > np.uint64(idmax)) | (gid % np.uint64(modulus) != 0)
    if odd:
        reject |= gid % np.uint64(2) == 0
    with np.errstate(invalid="ignore"):
        for a in range(3):      # (strict comparisons: a bead on a bound stays, a NaN passes)
            if rmax is not None:
                reject |= r[a] > rmax[a]
            if rmin is not None:
                reject |= r[a] < rmin[a]
            if vmax is not None:
                reject |= v[a] > vmax[a]
            if vmin is not None:
                reject |= v[a] < vmin[a]
    if species is not None:
        reject |= np.asarray(species)[sp] == 0
    if id_list is not None:
        ids = np.asarray(id_list, np.uint64)
        hit = np.zeros(len(gid), bool)
        if len(ids):      # bsearch in the ascending list
            k = np.searchsorted(ids, gid)
            hit = (k < len(ids)) & (ids[np.minimum(k, len(ids) - 1)] == gid)
        reject |= ~hit
    keep = ~reject
    out = np.zeros(int(keep.sum()), REC)
    out["id"] = gid[keep]
    gt = np.arange(ngroup) if group_term is None else np.asarray(group_term)
    st = np.arange(int(sp.max()) + 1 if len(sp) else 1) * ngroup if species_term is None else np.asarray(species_term)
    out["pinfo"] = (gt[group_of_gid(gid[keep])] + st[sp[keep]]).astype(np.uint32)
    for a in range(3):
        out["r"][:, a] = ((r[a][keep] - corner[a]) * cL).astype(np.float32)      # double, double, one rounding
    return out


class Case(object):
    def __init__(self, n):
        from ddcmd_amd.martini import MartiniHIP
        self.n, self.s = n, synthetic(n)
        self.m = MartiniHIP(self.s)
        self.p = particles(self.m)
        order = np.argsort(self.s.gid)
        self.sorted_gid, self.sorted_group = self.s.gid[order], self.s.group[order]
        self.corner = [-0.5 * x for x in BOX]

    def group_of(self, gid):
        return self.sorted_group[np.searchsorted(self.sorted_gid, gid)]

    def selections(self):
        p, n = self.p, self.n
        lane = np.arange(n) % 64
        ends = np.sort(p["gid"][(lane == 0) | (lane == 63)])      # the first and the last lane of every wave
        xs = np.sort(p["r"][0])
        lo, hi = xs[n // 4], xs[(3 * n) // 4]      # bounds exactly on two beads' coordinates: both stay
        vs = np.sort(p["v"][1])
        return {"none": dict(idmin=1, idmax=0), "all": dict(), "every second gid": dict(modulus=2), "odd": dict(odd=True),
                "wave ends": dict(id_list=ends), "one species": dict(species=[0, 1]),
                "x slab": dict(rmin=[lo, -1e9, -1e9], rmax=[hi, 1e9, 1e9]), "vy bound": dict(vmin=[-1.0, vs[n // 3], -1.0], vmax=[1.0, 1.0, 1.0]),
                "mixed": dict(modulus=5, odd=True, idmin=int(p["gid"].min()) + 1, idmax=int(p["gid"].max()) - 1, species=[1, 0], cL=0.0529177, rmax=[hi, 1e9, 1e9])}


@pytest.fixture(scope="module", params=COUNTS)
def case(request):
    c = Case(request.param)
    yield c
    c.m.close()


def test_records_are_the_restatements_bytes_in_order(case):
    c = case
    assert c.p["gid"].tolist() != sorted(c.p["gid"].tolist()) or c.n < 3      # slot order is not gid order: the order is tested
    seen = {}
    for name, f in c.selections().items():
        want = expect(c.p, c.group_of, c.corner, **f)
        got = c.m.subset_records(**f)
        seen[name] = len(got)
        assert got.dtype == REC and got.dtype.itemsize == 24
        assert len(got) == len(want), (c.n, name, len(got), len(want))
        assert got.tobytes() == want.tobytes(), (c.n, name, np.flatnonzero(got["id"] != want["id"])[:5])
        assert c.m.subset_records(**f).tobytes() == got.tobytes(), (c.n, name)      # a second call: the same bytes
        assert c.m.subset_records(count_only=True, **f) == len(want), (c.n, name)
    print(c.n, seen)
    assert seen["none"] == 0 and seen["all"] == c.n
    if c.n >= 63:
        assert 0 < seen["every second gid"] < c.n and 0 < seen["odd"] < c.n and 0 < seen["one species"] < c.n
        assert seen["wave ends"] == len(np.flatnonzero((np.arange(c.n) % 64 == 0) | (np.arange(c.n) % 64 == 63)))
        assert seen["x slab"] == (3 * c.n) // 4 - c.n // 4 + 1 and seen["vy bound"] == c.n - c.n // 3


def test_a_buffer_one_too_small_is_refused_and_left_alone(case):
    c = case
    n = c.m.subset_records(count_only=True)
    assert n == c.n
    out = np.zeros(n, REC)
    out["id"], out["pinfo"], out["r"] = 77, 7, 7.0
    before = out.tobytes()
    from ddcmd_amd.martini import DdcmiError
    with pytest.raises(DdcmiError, match="capacity %d < %d" % (n - 1, n)):
        c.m.subset_records(cap=n - 1, out=out)
    assert out.tobytes() == before
    got = c.m.subset_records(cap=n, out=out)      # the context goes on working
    assert got.tobytes() == expect(c.p, c.group_of, c.corner).tobytes()


@pytest.mark.parametrize("nid", [1, 2, 1000])
def test_id_lists_with_absent_ids(nid):
    c = Case(549)
    have = np.sort(c.s.gid)
    rng = np.random.default_rng(nid)
    present = rng.choice(have, size=max(1, nid // 2), replace=False)
    absent = (3 * rng.choice(5000, nid - len(present), replace=False) + 2).astype(np.uint64)      # 2 mod 3: no bead has such a gid
    ids = np.sort(np.concatenate([present, absent]))
    assert len(ids) == nid
    want = expect(c.p, c.group_of, c.corner, id_list=ids)
    got = c.m.subset_records(id_list=ids)
    assert len(want) == len(present) and got.tobytes() == want.tobytes()
    assert set(got["id"].tolist()) == set(ids.tolist()) & set(have.tolist())
    if nid == 1:      # a list of one absent id, and a list without a member: nothing
        assert len(c.m.subset_records(id_list=[5])) == 0 and len(c.m.subset_records(id_list=[])) == 0
    c.m.close()


def test_nan_and_beads_outside_the_box_follow_c():
    """a NaN velocity passes every comparison, as in C; a bead outside a periodic box is taken where the download puts it"""
    from ddcmd_amd.martini import MartiniHIP
    s = synthetic(130)
    s.vy[70] = np.nan
    s.ry[5], s.rx[70] = 1.25 * BOX[1], 0.0
    m = MartiniHIP(s)
    p = particles(m)
    assert np.isnan(p["v"][1][70]) and p["r"][1][5] == 0.25 * BOX[1]
    order = np.argsort(s.gid)
    gof = lambda g: s.group[order][np.searchsorted(s.gid[order], g)]
    f = dict(rmin=[-20.0, -1e9, -1e9], rmax=[20.0, 0.26 * BOX[1], 1e9], vmin=[-1.0, 0.0, -1.0], vmax=[1.0, 1.0, 1.0])
    want = expect(p, gof, [-0.5 * x for x in BOX], **f)
    got = m.subset_records(**f)
    assert got.tobytes() == want.tobytes()
    assert int(s.gid[70]) in got["id"].tolist()      # vy = NaN is neither below vmin nor above vmax
    five = m.subset_records(id_list=[int(s.gid[5])])
    assert len(five) == 1 and five["r"][0, 1] == np.float32((0.25 * BOX[1] + 0.5 * BOX[1]) * 1.0)
    m.close()


def test_the_run_is_not_changed_by_the_call():
    """state and energies of a run with calls between the steps equal those of a run without"""
    import ddcmd_amd
    from ddcmd_amd.martini import MartiniHIP
    s = ddcmd_amd.make_water_setup(6)
    outs = []
    for calls in (False, True):
        m = MartiniHIP(s)
        m.eval_forces()
        m.step(7)
        if calls:
            p = particles(m)
            order = np.argsort(s.gid)
            gof = lambda g: np.asarray(s.group)[order][np.searchsorted(s.gid[order], g)]
            got = m.subset_records(modulus=2, cL=units_convert(1.0, None, "Ang"))
            want = expect(p, gof, [-0.5 * s.h[0], -0.5 * s.h[4], -0.5 * s.h[8]], cL=units_convert(1.0, None, "Ang"), modulus=2, ngroup=max(1, s.ngroup))
            assert len(got) > 0 and got.tobytes() == want.tobytes()
            assert m.subset_records(count_only=True) == s.natoms
        m.step(13)
        e, vir, rk, t = m.energies()
        d = m.download()
        outs.append((sorted(e.items()), vir.tobytes(), rk, t.tobytes(), np.concatenate(d["r"] + d["v"] + d["f"]).tobytes()))
        m.close()
    assert outs[0] == outs[1]


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_in_process_domains_hold_every_selected_bead_once(grid):
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP, DdcmiError
    s = synthetic(1021)
    one = MartiniHIP(s)
    g = MartiniGroup(s, grid)
    order = np.argsort(s.gid)
    gof = lambda x: s.group[order][np.searchsorted(s.gid[order], x)]
    corner = [-0.5 * x for x in BOX]
    for f in (dict(), dict(modulus=2, species=[0, 1]), dict(idmin=1, idmax=0), dict(rmin=[0.0, -1e9, -1e9], rmax=[1e9, 1e9, 0.0])):
        want = one.subset_records(**f)
        rec, cnt = g.subset_records(per_rank=True, **f)
        assert cnt.shape == (g.n,) and cnt.sum() == len(rec) == len(want)
        assert len(np.unique(rec["id"])) == len(rec)      # no bead twice
        assert np.sort(rec, order="id").tobytes() == np.sort(want, order="id").tobytes()
        off = 0
        for r, rk in enumerate(g.ranks):      # every domain's block: its own beads in its own download order
            pr = rk.download_particles()
            assert rec[off:off + cnt[r]].tobytes() == expect(pr, gof, corner, **f).tobytes(), (grid, r)
            off += int(cnt[r])
    tot = int(g.subset_records(per_rank=True)[1].sum())
    out = np.full(24 * tot, 9, np.uint8).view(REC)
    before = out.tobytes()
    with pytest.raises(DdcmiError, match="capacity"):
        g.subset_records(cap=tot - 1, out=out)
    assert out.tobytes() == before
    # the single-context form refuses a context of a group and says where to go
    with pytest.raises(DdcmiError, match="ddcmi_group_subset_records"):
        g.ranks[0].subset_records()
    g.close()
    one.close()


def test_pinfo_on_the_lipid_deck():
    import os
    from ddcmd_amd.analysis import SubsetWrite
    from ddcmd_amd.deck import load_deck
    from ddcmd_amd.martini import MartiniHIP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = load_deck(os.path.join(root, "tests", "golden", "lipid_deck", "object.data"))
    assert s.nspecies > 2
    sw = SubsetWrite(s.group_name, s.species_name, species=[s.species_name[1], s.species_name[-1]], modulus=1, h=s.h, length_unit="nm")
    m = MartiniHIP(s, constraints=s.integrator_type.upper().startswith("NGLFCONSTRAINT") and s.nresicons > 0)
    p = particles(m)
    order = np.argsort(s.gid)
    gof = lambda x: np.asarray(s.group)[order][np.searchsorted(s.gid[order], x)]
    ng = max(1, s.ngroup)
    sel = [int(k in (1, s.nspecies - 1)) for k in range(s.nspecies)]
    # pinfo.c with one type and distinct names: group + species * ngroups
    want = expect(p, gof, [-0.5 * s.h[0], -0.5 * s.h[4], -0.5 * s.h[8]], cL=units_convert(1.0, None, "nm"), species=sel, ngroup=ng,
                  rmin=sw.rmin, rmax=sw.rmax, vmin=sw.vmin, vmax=sw.vmax, species_term=np.arange(s.nspecies) * ng)
    got = m.subset_records(**sw.filter())
    assert len(got) == int(np.isin(s.species, [1, s.nspecies - 1]).sum()) > 0
    assert got.tobytes() == want.tobytes()
    assert set(got["pinfo"].tolist()) <= {g + k * ng for g in range(ng) for k in (1, s.nspecies - 1)} and len(set(got["pinfo"].tolist())) >= 2
    m.close()


def test_refused_arguments_leave_a_message_and_a_usable_context():
    from ddcmd_amd.martini import MartiniHIP, DdcmiError
    s = synthetic(100)
    m = MartiniHIP(s)
    want = m.subset_records()
    for kw, word in ((dict(modulus=0), "modulus = 0"), (dict(modulus=-1), "modulus = -1"), (dict(id_list=[5, 4]), "not ascending"),
                     (dict(species_term=[0]), "nspecies = 1"), (dict(group_term=[0]), "ngroup = 1"), (dict(cL=float("inf")), "cL = inf"),
                     (dict(cL=float("nan")), "cL = nan")):
        with pytest.raises(DdcmiError, match=word):
            m.subset_records(**kw)
        assert m.subset_records().tobytes() == want.tobytes()
    n = np.zeros(1, np.int64)
    assert m.lib.ddcmi_subset_records(m.ctx, None, 0, None, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == EINVAL
    m.close()
    e = MartiniHIP(s, upload=False)
    with pytest.raises(DdcmiError, match="needs an uploaded state"):
        e.subset_records()
    e.close()

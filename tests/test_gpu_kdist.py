"""GPU tests (-m gpu) of the ANALYSIS type KINETICENERGYDISTN on the device: ddcmi_kinetic_energy_distn and the in-process group's
twin, on small synthetic states uploaded directly (internal units; no list is built except in the run test).

The yardstick is kineticEnergyDistn_eval's loop (kineticEnergyDistn.c:157-188) restated below in numpy float64, operation by
operation as the reference has them (numpy fuses nothing): v2 = (vx vx + vy vy) + vz vz, K = (0.5 mass) v2, K < emin, K >= emax,
(int)((K - emin) / delta) with delta = (emax - emin) / nBins.  Where the reference asserts, the device's definitions hold: a
quotient that truncates to nBins goes to the last bin; a NaN K is counted in cntTotal and the sum only.

Counts, tallies, minima and maxima are held to equality.  Sum K: the device adds in a fixed tree -- 6 levels inside a wave
(wave_sum_dpp), one addition into the wave's row of the group per pass over the workgroup's range (PASSES(n) = per_wg / 256 with
per_wg = 256 ceil(ceil(n / 1024) / 256): one pass up to 262144 beads), 3 for the four waves' rows, and the workgroups one after the
other: NWG(n) - 1 = ceil(n / per_wg) - 1.  A term passes through at most DEPTH(n) = 9 + PASSES(n) + NWG(n) - 1 additions, each with
a relative error of at most u = 2^-53, so |sum - exact| <= DEPTH(n) u sum K to first order (Higham, Accuracy and Stability of
Numerical Algorithms, ch. 4.2; K >= 0, so sum |K| = sum K); the K themselves are the same float64 numbers on both sides.  The
longdouble reference's own error (n 2^-64 sum K) is covered by using DEPTH + 1; combining r domains on the host adds r."""
import ctypes

import numpy as np
import pytest

from ddcmd_amd.deck import Setup, units_convert
from ddcmd_amd.synth import water_forcefield, make_water_setup, splitmix64

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
EINVAL, EUNSUPPORTED = -2, -4
MAX_LDS = 65536        # one workgroup's LDS: 4 B per bin, and per group 3 tallies of 4 B and 4 waves x {sum, min, max} x 8 B = 108 B
MAX_ONE = (MAX_LDS - 108) // 4      # 16357 bins for a single group
LBOX = 64.0
NBINS = (1, 7, 1000, 5)
SDIST = np.array([0, 1, 2, -1, 3, 2, 1, -1, -1], np.int32)      # species 5 and 6 share groups 2 and 1; 3, 7, 8 in none; 4 (group 3) has no members


def cdiv(a, b):
    return (a + b - 1) // b


def depth(n):
    per_wg = cdiv(cdiv(n, 1024), 256) * 256
    return 9 + per_wg // 256 + cdiv(n, per_wg) - 1 + 1


def _rand(n, stream):
    bits = splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(1000003 * (stream + 1))) >> np.uint64(11)
    return bits.astype(np.float64) / 9007199254740992.0


def synthetic(n, nspecies=9, L=LBOX, empty_species=4):
    """n beads in a cubic box of side L: the species changes from bead to bead (i * 7 % ns: any 64 consecutive beads hold every
    species that has members), one species without members, masses by species"""
    s = water_forcefield(Setup())
    s.h = np.diag([L, L, L]).ravel().astype(np.float64)
    s.pbc = 7
    s.nspecies = nspecies
    s.species_name = ["S%d" % k for k in range(nspecies)]
    s.mass = units_convert(72.0, "M_p") * (1.0 + 0.37 * np.arange(nspecies))
    s.charge = np.zeros(nspecies)
    s.ljtype = (np.arange(nspecies) % 2).astype(np.int32)
    s.moltype = (np.arange(nspecies) % 2).astype(np.int32)
    s.resitype = (np.arange(nspecies) % 2).astype(np.int32)
    s.atomoffset = np.zeros(nspecies, np.int32)
    s.ngroup = 1
    s.group_name = ["G0"]
    s.group_type = np.zeros(1, np.int32)
    s.group_Teq = np.zeros(1)
    s.group_tau = np.zeros(1)
    s.group_interval = np.ones(1, np.int32)
    s.natoms = n
    i = np.arange(n)
    sp = (i * 7) % nspecies
    sp[sp == empty_species] = (empty_species + 1) % nspecies
    s.species, s.group = sp.astype(np.int32), np.zeros(n, np.int32)
    s.gid = (i.astype(np.uint64) << np.uint64(32))
    s.rx, s.ry, s.rz = ((_rand(n, k) - 0.5) * L for k in range(3))
    s.vx, s.vy, s.vz = ((_rand(n, 3 + k) - 0.5) * 2e-3 for k in range(3))
    return s


# ---- the restatement --------------------------------------------------------
def kinetic(s, v, index=None):
    """K of every bead, float64, and its species"""
    sp = np.asarray(s.species)
    vx, vy, vz = (np.asarray(a, np.float64) for a in v)
    if index is not None:
        sp, vx, vy, vz = sp[index], vx[index], vy[index], vz[index]
    mass = np.asarray(s.mass, np.float64)[sp]
    with np.errstate(all="ignore"):
        v2 = (vx * vx + vy * vy) + vz * vz
        return (0.5 * mass) * v2, sp


def ref_kdist(K, sp, emin, emax, nbins, sdist):
    """(counts[sum nbins], tallies[nd, 3], sum K[nd] longdouble, min[nd], max[nd], beads whose quotient truncated to nbins)"""
    nd = len(nbins)
    g_of = np.asarray(sdist)[sp]
    counts, tallies, sums, mins, maxs, clamped = [], np.zeros((nd, 3), np.int64), np.zeros(nd, LD), np.full(nd, 1e300), np.zeros(nd), 0
    for g in range(nd):
        Kg = K[g_of == g]
        delta = (emax[g] - emin[g]) / int(nbins[g])
        sub, sup = Kg < emin[g], Kg >= emax[g]
        inside = ~sub & ~sup & ~np.isnan(Kg)
        with np.errstate(all="ignore"):
            ib = np.trunc((Kg[inside] - emin[g]) / delta).astype(np.int64)
        assert np.all((ib >= 0) & (ib <= nbins[g]))
        clamped += int((ib == nbins[g]).sum())
        counts.append(np.bincount(np.minimum(ib, nbins[g] - 1), minlength=int(nbins[g])).astype(np.int64))
        tallies[g] = len(Kg), sub.sum(), sup.sum()
        with np.errstate(all="ignore"):
            sums[g] = Kg.astype(LD).sum()
        ok = Kg[~np.isnan(Kg)]
        if len(ok):
            mins[g], maxs[g] = min(1e300, ok.min()), max(0.0, ok.max())
    return np.concatenate(counts), tallies, sums, mins, maxs, clamped


def edges(K, sp, sdist, nd):
    """emin and emax of every group from the K of two of its beads (the ones at the 10th and the 90th percentile): a bead with
    K == emin, one with K == emax, beads below and above; a group with fewer than four beads gets [0, 1)"""
    emin, emax = np.zeros(nd), np.ones(nd)
    for g in range(nd):
        Kg = np.sort(K[(np.asarray(sdist)[sp] == g) & np.isfinite(K)])
        if len(Kg) >= 4 and Kg[-1 - len(Kg) // 10] > Kg[len(Kg) // 10]:
            emin[g], emax[g] = Kg[len(Kg) // 10], Kg[-1 - len(Kg) // 10]
    return emin, emax


def _ctx(s):
    from ddcmd_amd.martini import MartiniHIP
    return MartiniHIP(s)


def assert_kdist(got, ref, n, what="", extra=0):
    counts, tallies, stats = got
    wc, wt, ws, wmin, wmax, _ = ref
    assert np.array_equal(counts, wc), (what, np.flatnonzero(counts != wc)[:10])
    assert np.array_equal(tallies, wt), (what, tallies, wt)
    assert np.array_equal(stats[:, 1], wmin) and np.array_equal(stats[:, 2], wmax), (what, stats, wmin, wmax)
    d = depth(n) + extra
    for g in range(len(ws)):
        if np.isfinite(ws[g]):
            err = abs(LD(stats[g, 0]) - ws[g])
            print("%s n=%d depth=%d group %d: sum K err/bound %.3f" % (what, n, d, g, float(err / max(d * U * ws[g], LD(1e-300)))))
            assert err <= d * U * ws[g], (what, g, stats[g, 0], ws[g])
        else:
            assert (np.isnan(stats[g, 0]) and np.isnan(ws[g])) or stats[g, 0] == ws[g], (what, g, stats[g, 0], ws[g])


# ---- against the restatement ------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1021, 262147])
def test_histograms_tallies_and_extremes_equal_the_restatement(n):
    s = synthetic(n)
    if n >= 63:
        assert len(np.unique(s.species[:63])) == 8      # several groups inside every single wave
    m = _ctx(s)
    K, sp = kinetic(s, m.download()["v"])
    assert np.array_equal(K, kinetic(s, (s.vx, s.vy, s.vz))[0])      # the pass reads the velocities as uploaded
    emin, emax = edges(K, sp, SDIST, 4)
    ref = ref_kdist(K, sp, emin, emax, NBINS, SDIST)
    got = m.kinetic_energy_distn(emin, emax, NBINS, SDIST)
    assert got[0].shape == (sum(NBINS),) and got[0].dtype == np.int64 and got[1].shape == (4, 3) and got[2].shape == (4, 3)
    assert_kdist(got, ref, n, "one domain")
    c, t, st = got
    assert t[:, 0].sum() == int((SDIST[sp] >= 0).sum())      # a species without a group is skipped
    assert np.all(t[3] == 0) and np.all(c[1008:] == 0) and st[3].tolist() == [0.0, 1e300, 0.0]      # the group without members: the initial values
    off = np.concatenate([[0], np.cumsum(NBINS)])
    for g in range(4):
        assert c[off[g]:off[g + 1]].sum() + t[g, 1] + t[g, 2] == t[g, 0]
    if n >= 255:      # the edges: the bead with K == emin sits in bin 0 (it is the lowest inside), the one with K == emax is a supCnt
        for g in range(3):
            Kg = K[SDIST[sp] == g]
            assert (Kg == emin[g]).sum() >= 1 and (Kg == emax[g]).sum() >= 1
            assert t[g, 1] == (Kg < emin[g]).sum() > 0 and t[g, 2] == (Kg >= emax[g]).sum() > 0 and c[off[g]] >= 1
            assert st[g, 1] < emin[g] and st[g, 2] > emax[g]
    again = m.kinetic_energy_distn(emin, emax, NBINS, SDIST)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))      # bit for bit
    m.close()


def test_a_quotient_that_truncates_to_nbins_goes_to_the_last_bin():
    """emax = nextafter(K_b, inf): bead b is the highest inside; with delta rounded down, (K_b - emin) / delta reaches nbins"""
    n = 1021
    s = synthetic(n)
    K, sp = kinetic(s, (s.vx, s.vy, s.vz))
    mine = np.flatnonzero(SDIST[sp] == 0)
    found = None
    for b in mine[np.argsort(K[mine])[len(mine) // 2:]]:      # candidates: the upper half of the group
        emax = np.nextafter(K[b], np.inf)
        for nb in range(3, 400):
            if int(np.trunc((K[b] - 0.0) / ((emax - 0.0) / nb))) == nb:
                found = (b, nb, emax)
                break
        if found:
            break
    assert found, "no bead / nbins pair whose quotient truncates to nbins"
    b, nb, emax = found
    nbins, emin, emaxs = (nb, 7, 1000, 5), np.zeros(4), np.array([emax, 1.0, 1.0, 1.0])
    ref = ref_kdist(K, sp, emin, emaxs, nbins, SDIST)
    assert ref[5] >= 1      # the case occurred in the restatement
    m = _ctx(s)
    got = m.kinetic_energy_distn(emin, emaxs, nbins, SDIST)
    assert_kdist(got, ref, n, "last bin")
    assert got[0][nb - 1] >= 1 and got[1][0, 2] == (K[mine] >= emax).sum() == (K[mine] > K[b]).sum()
    m.close()


def test_one_nan_and_one_inf_velocity():
    n = 1021
    s = synthetic(n)
    a, b = np.flatnonzero(s.species == 0)[5], np.flatnonzero(s.species == 1)[7]
    s.vx, s.vy = s.vx.copy(), s.vy.copy()
    s.vx[a], s.vy[b] = np.nan, np.inf
    m = _ctx(s)
    K, sp = kinetic(s, m.download()["v"])
    assert np.isnan(K[a]) and K[b] == np.inf
    emin, emax = edges(K, sp, SDIST, 4)
    ref = ref_kdist(K, sp, emin, emax, NBINS, SDIST)
    c, t, st = got = m.kinetic_energy_distn(emin, emax, NBINS, SDIST)
    assert_kdist(got, ref, n, "nan, inf")
    # the NaN: counted, in the sum, nowhere else; the inf: a supCnt, the sum and the maximum
    assert np.isnan(st[0, 0]) and c[0] + t[0, 1] + t[0, 2] == t[0, 0] - 1 and np.isfinite(st[0, 1]) and np.isfinite(st[0, 2])
    assert st[1, 0] == np.inf and st[1, 2] == np.inf and c[1:8].sum() + t[1, 1] + t[1, 2] == t[1, 0]
    assert np.isfinite(st[2]).all()
    m.close()


def test_the_cap_and_two_species_in_one_group():
    from ddcmd_amd.martini import DdcmiError
    n = 1021
    s = synthetic(n)
    m = _ctx(s)
    K, sp = kinetic(s, (s.vx, s.vy, s.vz))
    sd = np.array([0, 0, 0, -1, 0, 0, 0, 0, -1], np.int32)      # seven species, seven masses, one group
    emin, emax = edges(K, sp, sd, 1)
    got = m.kinetic_energy_distn(emin, emax, [MAX_ONE], sd)
    assert_kdist(got, ref_kdist(K, sp, emin, emax, [MAX_ONE], sd), n, "largest")
    assert got[1][0, 0] == (sd[sp] == 0).sum() and (got[0] > 0).sum() > 300
    with pytest.raises(DdcmiError, match="16358 bins in 1 groups need 65540 bytes of LDS, at most 65536"):
        m.kinetic_energy_distn(emin, emax, [MAX_ONE + 1], sd)
    # two groups: 4 (8192 + 8138) + 216 = 65536 fits, one bin more does not
    sd2 = np.array([0, 1, 0, -1, 0, 1, 0, 1, -1], np.int32)
    e0, e1 = edges(K, sp, sd2, 2)
    got = m.kinetic_energy_distn(e0, e1, [8192, 8138], sd2)
    assert_kdist(got, ref_kdist(K, sp, e0, e1, [8192, 8138], sd2), n, "two large")
    with pytest.raises(DdcmiError, match="16331 bins in 2 groups"):
        m.kinetic_energy_distn(e0, e1, [8192, 8139], sd2)
    assert m.lib.ddcmi_last_error(m.ctx).startswith(b"ddcmi_kinetic_energy_distn:")
    again = m.kinetic_energy_distn(e0, e1, [8192, 8138], sd2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    m.close()


# ---- refusals ---------------------------------------------------------------
def test_refused_arguments_leave_a_message_and_a_usable_context():
    from ddcmd_amd.martini import MartiniHIP
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
    s = synthetic(100)
    m = _ctx(s)
    lib, ctx = m.lib, m.ctx
    fn = lib.ddcmi_kinetic_energy_distn
    emin, emax, nb, sd = np.zeros(2), np.ones(2), np.array([4, 6], np.int32), np.array([0, 1, -1, -1, -1, -1, -1, -1, -1], np.int32)
    cnt, tal, st = np.zeros(10, np.int64), np.zeros(6, np.int64), np.zeros(6)
    D, I, Lp = (lambda a: a.ctypes.data_as(dp)), (lambda a: a.ctypes.data_as(ip)), (lambda a: a.ctypes.data_as(lp))

    def call(nspecies=9, ndist=2, emin=emin, emax=emax, nb=nb, sd=sd, outs=(True, True, True)):
        return fn(ctx, nspecies, ndist, D(emin) if emin is not None else None, D(emax) if emax is not None else None, I(nb) if nb is not None else None,
                  I(sd) if sd is not None else None, Lp(cnt) if outs[0] else None, Lp(tal) if outs[1] else None, D(st) if outs[2] else None)

    def sdv(k, v):
        a = sd.copy()
        a[k] = v
        return a

    cases = [
        (lambda: call(emin=None), EINVAL, b"NULL"), (lambda: call(emax=None), EINVAL, b"NULL"), (lambda: call(nb=None), EINVAL, b"NULL"),
        (lambda: call(sd=None), EINVAL, b"NULL"), (lambda: call(outs=(False, True, True)), EINVAL, b"NULL"),
        (lambda: call(outs=(True, False, True)), EINVAL, b"NULL"), (lambda: call(outs=(True, True, False)), EINVAL, b"NULL"),
        (lambda: call(nspecies=8), EINVAL, b"nspecies = 8, the context has 9"), (lambda: call(nspecies=10), EINVAL, b"nspecies = 10"),
        (lambda: call(ndist=-1), EINVAL, b"ndist = -1"),
        (lambda: call(nb=np.array([4, 0], np.int32)), EINVAL, b"nbins[1] = 0"), (lambda: call(nb=np.array([-2, 6], np.int32)), EINVAL, b"nbins[0] = -2"),
        (lambda: call(emin=np.array([np.nan, 0.0])), EINVAL, b"not finite"), (lambda: call(emax=np.array([1.0, np.inf])), EINVAL, b"not finite"),
        (lambda: call(emin=np.array([-np.inf, 0.0])), EINVAL, b"not finite"),
        (lambda: call(emax=np.array([1.0, 0.0])), EINVAL, b"emax[1] = 0 <= emin[1] = 0"), (lambda: call(emin=np.array([2.0, 0.0])), EINVAL, b"emax[0] = 1 <= emin[0] = 2"),
        (lambda: call(sd=sdv(3, 2)), EINVAL, b"species_dist[3] = 2, outside [-1, 2)"), (lambda: call(sd=sdv(0, -2)), EINVAL, b"species_dist[0] = -2"),
        (lambda: call(nb=np.array([MAX_ONE, 6], np.int32)), EUNSUPPORTED, b"at most 65536"),
    ]
    want = m.kinetic_energy_distn(emin, emax, nb, sd)
    assert want[1][:, 0].sum() > 0
    for k, (c, code, word) in enumerate(cases):
        before = (cnt.tobytes(), tal.tobytes(), st.tobytes())
        rc = c()
        msg = lib.ddcmi_last_error(ctx)
        assert rc == code and word in msg and msg.startswith(b"ddcmi_kinetic_energy_distn"), (k, rc, msg)
        assert before == (cnt.tobytes(), tal.tobytes(), st.tobytes())      # nothing written
        got = m.kinetic_energy_distn(emin, emax, nb, sd)      # the context goes on working
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert fn(None, 9, 2, D(emin), D(emax), I(nb), I(sd), Lp(cnt), Lp(tal), D(st)) == EINVAL
    # two species mapped to one group: allowed, the call follows the map
    both = m.kinetic_energy_distn(emin, emax, nb, sdv(2, 0))
    assert both[1][0, 0] == want[1][0, 0] + (s.species == 2).sum()
    # no group at all: valid, nothing is touched (the arrays may be absent)
    cnt[:] = 7
    assert fn(ctx, 9, 0, None, None, None, I(np.full(9, -1, np.int32)), None, None, None) == 0 and np.all(cnt == 7)
    c0, t0, s0 = m.kinetic_energy_distn([], [], [], np.full(9, -1, np.int32))
    assert c0.shape == (0,) and t0.shape == (0, 3) and s0.shape == (0, 3)
    m.close()
    # no uploaded state
    e = MartiniHIP(s, upload=False)
    assert e.lib.ddcmi_kinetic_energy_distn(e.ctx, 9, 2, D(emin), D(emax), I(nb), I(sd), Lp(cnt), Lp(tal), D(st)) == EINVAL
    assert b"needs an uploaded state" in e.lib.ddcmi_last_error(e.ctx)
    e.upload(s.rx, s.ry, s.rz, s.vx, s.vy, s.vz)
    got = e.kinetic_energy_distn(emin, emax, nb, sd)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    e.close()


# ---- no effect on the run ---------------------------------------------------
def test_the_call_reads_only():
    s = synthetic(1021)
    m = _ctx(s)
    K, sp = kinetic(s, (s.vx, s.vy, s.vz))
    emin, emax = edges(K, sp, SDIST, 4)
    d0 = m.download()
    a = m.kinetic_energy_distn(emin, emax, NBINS, SDIST)
    b = m.kinetic_energy_distn(emin, emax, NBINS, SDIST)
    d1 = m.download()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert np.concatenate(d0["r"] + d0["v"] + d0["f"]).tobytes() == np.concatenate(d1["r"] + d1["v"] + d1["f"]).tobytes()
    m.close()


def test_calls_between_steps_change_nothing_of_the_run():
    s = make_water_setup(6)
    sd = np.full(s.nspecies, -1, np.int32)
    sd[0] = 0
    kT = 310.0 * units_convert(1.0, "K", None)
    out = []
    for calls in (True, False):
        m = _ctx(s)
        m.eval_forces()
        for _ in range(20):
            m.step(1)
            if calls:
                got = m.kinetic_energy_distn([0.0], [6 * kT], [50], sd)
        d = m.download()
        e, vir, rk, tion = m.energies()
        out.append((np.concatenate(d["r"] + d["v"]).tobytes(), np.array([e[k] for k in sorted(e)] + [rk]).tobytes() + np.asarray(vir).tobytes() + np.asarray(tion).tobytes()))
        if calls:      # and the histogram is that of the state at hand
            K, sp = kinetic(s, d["v"])
            assert_kdist(got, ref_kdist(K, sp, [0.0], [6 * kT], [50], sd), s.natoms, "after 20 steps")
            assert got[1][0, 0] == (s.species == 0).sum() > 0
        m.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]


# ---- decomposed -------------------------------------------------------------
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_in_process_groups_combine_to_the_one_domain_result(grid):
    from ddcmd_amd.martini import MartiniGroup, domain_of
    n = 1021
    s = synthetic(n)
    owner = domain_of(s, grid)
    last = grid[0] * grid[1] * grid[2] - 1
    s.rx = np.where(owner == last, -np.abs(s.rx), s.rx)      # the last domain is left empty
    K, sp = kinetic(s, (s.vx, s.vy, s.vz))
    emin, emax = edges(K, sp, SDIST, 4)
    one = _ctx(s)
    want = one.kinetic_energy_distn(emin, emax, NBINS, SDIST)
    g = MartiniGroup(s, grid)
    nloc = [int(g.lib.ddcmi_nlocal(r.ctx)) for r in g.ranks]
    assert nloc[last] == 0 and sum(nloc) == n
    # the single-context form refuses a context of a group and says where to go
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
    nb = np.array(NBINS, np.int32)
    cnt, tal, st = np.zeros(sum(NBINS), np.int64), np.zeros(12, np.int64), np.zeros(12)
    rc = g.lib.ddcmi_kinetic_energy_distn(g.ranks[0].ctx, 9, 4, emin.ctypes.data_as(dp), emax.ctypes.data_as(dp), nb.ctypes.data_as(ip), SDIST.ctypes.data_as(ip),
                                          cnt.ctypes.data_as(lp), tal.ctypes.data_as(lp), st.ctypes.data_as(dp))
    assert rc == EINVAL and b"ddcmi_group_kinetic_energy_distn" in g.lib.ddcmi_last_error(g.ranks[0].ctx)
    pc, pt, ps = g.kinetic_energy_distn(emin, emax, NBINS, SDIST, per_rank=True)
    assert pc.shape == (len(nloc), sum(NBINS)) and pt.shape == (len(nloc), 4, 3) and ps.shape == (len(nloc), 4, 3)
    assert not pc[last].any() and not pt[last].any() and ps[last].tolist() == [[0.0, 1e300, 0.0]] * 4      # the empty domain: zeros and the initial extremes
    for r, rk in enumerate(g.ranks):      # every rank against the restatement over its own beads
        if nloc[r]:
            Kr, spr = kinetic(s, (s.vx, s.vy, s.vz), index=rk.index)
            assert_kdist((pc[r], pt[r], ps[r]), ref_kdist(Kr, spr, emin, emax, NBINS, SDIST), nloc[r], "rank %d" % r)
    tot = g.kinetic_energy_distn(emin, emax, NBINS, SDIST)
    assert np.array_equal(tot[0], want[0]) and np.array_equal(tot[1], want[1])
    assert np.array_equal(tot[2][:, 1:], want[2][:, 1:])      # minimum of minima, maximum of maxima: exact
    assert_kdist(tot, ref_kdist(K, sp, emin, emax, NBINS, SDIST), n, "group total", extra=len(nloc))
    g.close()
    one.close()

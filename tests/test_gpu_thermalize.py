"""GPU tests (-m gpu) of ddcmi_thermalize on a dilute gas whose forces play no part (no list is ever built): 1 to 20 011 beads of three
species (masses 72, 36, 1 M_p) in two groups interleaved bead by bead, with sparse gids -- 0, values above 2^32, two equal in their low 16
bits.  The yardstick is tests/thermalize_reference.py (Python integers and numpy.longdouble); its docstring derives the bounds used here.

BOLTZMANN: the set of beads written, the rejected draws of every bead (ddcmi_debug_thermalize_rejects) and the untouched velocities are
held exactly, the values to 10 + 1 / |ln rsq| ulps; the same call repeats its bits, loop and seed change every written bead (but gid 0
under another loop: its label (loop % 10000000 + 1) * gid is 0 at every loop, in the reference too), loop + 10000000 changes none; 2, 4 and 8 in-process domains give every gid the bits of one domain; at 20 011 beads the species' <m v^2> / 3
lie within 5 standard errors of T and a 20-bin histogram of ddcmi_kinetic_energy_distn passes chi-square at the 1e-4 level.  The seed is
the deck's default, 385212586; the test first holds the reference's own velocities to the same chi-square level (another seed would have
to be chosen, and recorded here, if they failed it) and prints both values: 20.60 for the reference and 20.60 for the device's histogram
on an MI355X, against the critical 52.39 -- no other seed was needed.

RESCALE: against the longdouble reference to rescale_bound for the three selects and both keep_vcm; the class temperature and centre of
mass afterwards; T <= 0 scales by 1; a class of one bead and a class of equal velocities keep their bits; repeats and 1, 2, 4 domains."""
import ctypes

import numpy as np
import pytest

import restraint_systems as R
import thermalize_reference as TR
from ddcmd_amd.deck import Setup, units_convert

pytestmark = pytest.mark.gpu
MP = units_convert(1.0, "M_p")
T0 = 310.0 * units_convert(1.0, "K")
SIZES = (1, 63, 64, 65, 1025, 20011)
SEED = TR.DEFAULT_SEED
_DP = ctypes.POINTER(ctypes.c_double)
_cache = {}


def gas(n, equal_group=False):
    """module docstring.  equal_group: the beads of group 1 all move alike (dyadic components: their sums are exact), and species 2 has one bead"""
    rng = np.random.RandomState(20261021 + n)
    s = Setup()
    R._forcefield(s, 20)
    s.nspecies, s.species_name = 3, ["WxW", "WFxWF", "L"]
    s.mass = np.array([72.0, 36.0, 1.0]) * MP
    s.charge = np.zeros(3)
    s.ljtype, s.moltype, s.resitype, s.atomoffset = (np.array(a, np.int32) for a in ([1, 0, 0], [0, 1, 2], [0, 1, 2], [0, 0, 0]))
    s.nmoltype, s.mol_nspecies, s.bpair_off = 3, np.ones(3, np.int32), np.zeros(4, np.int32)
    s.nresi, s.resi_natoms = 3, np.ones(3, np.int32)
    s.bond_off = s.angle_off = s.tors_off = np.zeros(4, np.int32)
    L = np.array(R.BOX_A)
    r = rng.uniform(-0.5, 0.5, (n, 3)) * L
    species = rng.randint(0, 3, n).astype(np.int32)
    if equal_group:
        species[species == 2] = 0
        species[min(5, n - 1)] = 2
    v = rng.normal(size=(n, 3)) * np.sqrt(T0 / s.mass[species])[:, None] * 1.3 + np.array([0.4, -0.25, 0.1]) * np.sqrt(T0 / (72.0 * MP))
    R._finish(s, r, v, rng, species)
    s.group = (np.arange(n) % 2).astype(np.int32)
    if equal_group:
        for a, c in zip((s.vx, s.vy, s.vz), (0.25, -0.5, 1.0)):
            a[s.group == 1] = c * 2.0 ** -10
    s.ngroup, s.group_name = 2, ["even", "odd"]
    s.group_type, s.group_Teq, s.group_tau, s.group_interval = np.zeros(2, np.int32), np.zeros(2), np.zeros(2), np.ones(2, np.int32)
    gid = np.unique(rng.randint(1, 2 ** 44, 2 * n + 8, dtype=np.int64).astype(np.uint64))
    gid = gid[rng.permutation(len(gid))][:n]
    gid[0] = 0
    if n > 2:
        gid[2] = (gid[1] & np.uint64(0xFFFF)) | np.uint64(0x123400000000 + (7 << 16))      # the low 16 bits of gid[1], above 2^32
        gid[1] |= np.uint64(1 << 40)
    assert len(np.unique(gid)) == n and (n < 3 or (gid.max() > 2 ** 32 and (gid[1] ^ gid[2]) & np.uint64(0xFFFF) == 0))
    s.gid = gid
    s.nrest = 0
    return s


def make(s, **kw):
    from ddcmd_amd.martini import MartiniHIP
    return MartiniHIP(s, test_api=True, **kw)


def vel(m):
    return np.stack(m.download()["v"], 1)


def by_gid(g):
    return np.stack(g["v"], 1)      # MartiniGroup.gather: ordered by gid


def class_T(s, select, temps):
    """(class of every bead, its temperature)"""
    cls = {"global": np.zeros(s.natoms, int), "species": np.asarray(s.species, int), "group": np.asarray(s.group, int)}[select]
    return cls, np.asarray(temps, float)[cls]


def reference(n, select, temps, loop=0):
    key = (n, select, tuple(temps), loop)
    if key not in _cache:
        s = gas(n)
        _, Tb = class_T(s, select, temps)
        _cache[key] = TR.boltzmann(s.gid, s.mass[s.species], Tb, SEED, loop)
    return _cache[key]


def rejects(m, select, temps, seed, loop):
    lib = m.lib
    lib.ddcmi_debug_thermalize_rejects.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _DP, ctypes.c_uint64, ctypes.c_int64,
                                                   ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
    t = np.ascontiguousarray(temps, dtype=np.float64)
    n = m.n
    nout, gid, rej = ctypes.c_int(0), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    m._chk(lib.ddcmi_debug_thermalize_rejects(m.ctx, {"global": 0, "species": 1, "group": 2}[select], t.size, t.ctypes.data_as(_DP), seed, loop,
                                              n, ctypes.byref(nout), gid.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), rej.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    assert nout.value == n
    return dict(zip(gid.tolist(), rej.tolist()))


@pytest.mark.parametrize("n", SIZES)
def test_boltzmann_written_set_rejected_draws_and_values(n):
    select, temps = ("species", (T0, 0.5 * T0, -1.0)) if n != 20011 else ("global", (T0,))
    s = gas(n)
    m = make(s)
    before = vel(m)
    rj = rejects(m, select, temps, SEED, 0)
    assert np.array_equal(vel(m), before)      # the probe writes nothing
    m.thermalize("BOLTZMANN", temps, select=select, seed=SEED, loop=0)
    after = vel(m)
    m.close()
    ref, nrej, rsq = reference(n, select, temps)
    _, Tb = class_T(s, select, temps)
    written = Tb >= 0.0
    assert np.array_equal(after[~written].view(np.uint64), before[~written].view(np.uint64))      # every other velocity keeps its bits
    assert np.all(np.any(after[written] != before[written], axis=1))
    assert [rj[int(g)] for g in s.gid] == nrej.tolist()
    err = np.abs(after[written].astype(TR.LD) - ref[written])
    ulp = np.spacing(np.abs(ref[written].astype(np.float64)))
    ratio = (err / ulp).astype(np.float64) / TR.boltzmann_bound_ulps(rsq[written])
    print("n = %d: %d written, %d rejected draws, largest error / bound %.3f" % (n, written.sum(), nrej[written].sum(), ratio.max() if written.any() else 0.0))
    assert np.all(np.isfinite(after)) and (not written.any() or ratio.max() <= 1.0)


def test_boltzmann_repeats_and_depends_on_loop_and_seed():
    s = gas(1025)
    temps = (T0, -1.0)
    out = {}
    for key, (seed, loop) in dict(a=(SEED, 3), b=(SEED, 3), loop=(SEED, 4), seed=(SEED + 1, 3), wrap=(SEED, 3 + 10000000)).items():
        m = make(s)
        m.thermalize("BOLTZMANN", temps, select="group", seed=seed, loop=loop)
        if key == "b":
            m.thermalize("BOLTZMANN", temps, select="group", seed=seed, loop=loop)      # twice on one context
        out[key] = vel(m)
        m.close()
    w = s.group == 0
    assert np.array_equal(out["a"], out["b"]) and np.array_equal(out["a"], out["wrap"])
    # gid 0 is the one bead whose stream no loop can change: its label (loop % 10000000 + 1) * gid is 0 at every loop (thermalize.c:118-119)
    zero = np.asarray(s.gid)[w] == 0
    assert zero.sum() == 1
    for key in ("loop", "seed"):
        differs = np.all(out[key][w] != out["a"][w], axis=1)
        assert np.all(differs[~zero]) and np.array_equal(out[key][~w], out["a"][~w])
        assert differs[zero][0] == (key == "seed")


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1), (2, 2, 2)], ids=["2", "4", "8"])
def test_boltzmann_domains_give_every_gid_the_same_bits(grid):
    from ddcmd_amd.martini import MartiniGroup
    n, temps = 1025, (T0, 0.5 * T0, -1.0)
    s = gas(n)
    m = make(s)
    m.thermalize("BOLTZMANN", temps, select="species", seed=SEED, loop=17)
    one = vel(m)[np.argsort(s.gid, kind="stable")]
    m.close()
    g = MartiniGroup(s, grid)
    g.thermalize("BOLTZMANN", temps, select="species", seed=SEED, loop=17)
    out = g.gather()
    g.close()
    assert np.array_equal(out["gid"], np.sort(s.gid)) and min(out["nlocal"]) > 0
    assert np.array_equal(by_gid(out).view(np.uint64), one.view(np.uint64))


def test_boltzmann_statistics():
    n, nb, top = 20011, 20, 6.0
    s = gas(n)
    ref, _, _ = reference(n, "global", (T0,))
    mass = s.mass[s.species]
    edges = np.linspace(0.0, top, nb + 1)
    Kref = 0.5 * mass * (ref.astype(np.float64) ** 2).sum(axis=1) / T0
    cref = np.concatenate([np.histogram(Kref, edges)[0], [(Kref >= top).sum()]])
    chi_ref = TR.chi2_maxwell(cref, n, edges)
    print("chi-square of the reference's own velocities: %.2f (critical %.2f)" % (chi_ref, TR.CHI2_CRIT_20_1E4))
    assert chi_ref < TR.CHI2_CRIT_20_1E4      # else: another seed, recorded here
    m = make(s)
    m.thermalize("BOLTZMANN", (T0,), seed=SEED, loop=0)
    v = vel(m)
    counts, tallies, stats = m.kinetic_energy_distn([0.0], [top * T0], [nb], [0, 0, 0])
    m.close()
    for sp in range(3):
        k = s.species == sp
        x = (mass[k] * (v[k] ** 2).sum(axis=1) / 3.0).mean()
        se = T0 * np.sqrt(2.0 / (3.0 * k.sum()))      # m v^2 / 3 = T chi^2_3 / 3: variance 2 T^2 / 3
        print("species %d: <m v^2> / 3 = %.6f T, %.2f standard errors" % (sp, x / T0, (x - T0) / se))
        assert abs(x - T0) < 5.0 * se
    assert tallies[0, 0] == n and tallies[0, 1] == 0
    chi = TR.chi2_maxwell(np.concatenate([counts, [tallies[0, 2]]]), n, edges)
    print("chi-square of the device's histogram: %.2f" % chi)
    assert chi < TR.CHI2_CRIT_20_1E4


RESCALE_CASES = {"global": (0.8 * T0,), "species": (T0, 2.0 * T0, -1.0), "group": (0.0, 1.5 * T0)}


def _check_rescale(s, select, temps, keep, got, what):
    cls, _ = class_T(s, select, temps)
    v0 = np.stack([s.vx, s.vy, s.vz], 1)
    mass = s.mass[s.species]
    ref, info = TR.rescale(v0, mass, cls, temps, keep)
    bound, tb = TR.rescale_bound(v0, mass, info)
    err = np.abs(got.astype(TR.LD) - ref)
    ok = bound > 0
    print("%s %s keep_vcm %d: largest error / bound %.3g" % (what, select, keep, float((err[ok] / bound[ok]).max()) if ok.any() else 0.0))
    assert np.all(err <= bound)
    for c, d in enumerate(info):
        k = d["idx"]
        if not d["applied"]:
            assert np.array_equal(got[k].view(np.uint64), v0[k].view(np.uint64))      # N <= 1 or no spread: the class keeps its bits
            continue
        Tc, vcm = TR.class_temperature(got, mass, cls, c)
        if temps[c] > 0.0:
            assert abs(float(Tc / TR.LD(temps[c])) - 1.0) <= tb[c], (c, float(Tc), temps[c])
        else:
            assert d["scale"] == 1      # T <= 0: scaled by exactly 1 -- the velocities are the input's to the roundings of (v - vcm) + vcm
            assert np.all(np.abs(got[k] - v0[k]) <= 4 * TR.U * (np.abs(v0[k]) + np.abs(d["vcm"].astype(np.float64))))
        want = d["vcm"] if (keep or temps[c] <= 0.0) else d["vcm"] * d["scale"]
        vb = (mass[k, None].astype(TR.LD) * bound[k]).sum(axis=0) / d["M"]      # the mass-weighted mean of the beads' bounds
        assert np.all(np.abs(vcm - want) <= vb + 4 * TR.U * np.abs(want))
    return ref


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("select", ["global", "species", "group"])
@pytest.mark.parametrize("n", [65, 1025])
def test_rescale_against_the_longdouble_reference(n, select, keep):
    s = gas(n)
    temps = RESCALE_CASES[select]
    m = make(s)
    m.thermalize("RESCALE", temps, select=select, keep_vcm=keep)
    a = vel(m)
    m.close()
    _check_rescale(s, select, temps, keep, a, "n = %d" % n)
    m = make(s)
    m.thermalize("RESCALE", temps, select=select, keep_vcm=keep)
    assert np.array_equal(vel(m).view(np.uint64), a.view(np.uint64))      # repeating the call (from the same state) gives the same bits
    m.close()


def test_rescale_one_bead_and_equal_velocities_keep_their_bits():
    s = gas(65, equal_group=True)
    v0 = np.stack([s.vx, s.vy, s.vz], 1)
    assert (s.species == 2).sum() == 1
    m = make(s)
    m.thermalize("RESCALE", (T0, T0, T0), select="species")
    a = vel(m)
    lone = s.species == 2
    assert np.array_equal(a[lone].view(np.uint64), v0[lone].view(np.uint64)) and np.all(np.any(a[~lone] != v0[~lone], axis=1))
    m.close()
    _check_rescale(s, "species", (T0, T0, T0), 0, a, "one bead")
    m = make(s)
    m.thermalize("RESCALE", (T0, T0), select="group")
    a = vel(m)
    m.close()
    eq = s.group == 1
    assert np.array_equal(a[eq].view(np.uint64), v0[eq].view(np.uint64)) and np.all(np.any(a[~eq] != v0[~eq], axis=1))
    _check_rescale(s, "group", (T0, T0), 0, a, "equal velocities")


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1)], ids=["2", "4"])
def test_rescale_domains_agree_and_repeat(grid):
    from ddcmd_amd.martini import MartiniGroup
    s = gas(1025)
    order = np.argsort(s.gid, kind="stable")
    for select, keep in (("species", 0), ("group", 1), ("global", 0)):
        temps = RESCALE_CASES[select]
        outs = []
        for _ in range(2):
            g = MartiniGroup(s, grid)
            g.thermalize("RESCALE", temps, select=select, keep_vcm=keep)
            outs.append(by_gid(g.gather()))
            g.close()
        assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
        back = np.empty_like(outs[0])
        back[order] = outs[0]
        _check_rescale(s, select, temps, keep, back, "%d domains" % (grid[0] * grid[1] * grid[2]))


def _call(m, *a):
    return m.lib.ddcmi_thermalize(m.ctx, *a)


def test_refuses_a_context_without_state():
    m = make(gas(65), upload=False)
    t = np.array([T0])
    assert _call(m, 0, 0, 1, t.ctypes.data_as(_DP), 1, 0, 0) == -2
    m.close()


def test_refuses_bad_arguments_and_changes_nothing():
    from ddcmd_amd.martini import DdcmiError
    EINVAL, EUNSUPPORTED = -2, -4
    m = make(gas(65))
    v0 = vel(m)
    t = np.array([T0, T0, T0])
    p = t.ctypes.data_as(_DP)
    assert _call(m, -1, 0, 1, p, 1, 0, 0) == EINVAL and _call(m, 3, 0, 1, p, 1, 0, 0) == EINVAL      # method out of range
    assert _call(m, 0, -1, 1, p, 1, 0, 0) == EINVAL and _call(m, 0, 3, 1, p, 1, 0, 0) == EINVAL      # select out of range
    assert _call(m, 0, 1, 2, p, 1, 0, 0) == EINVAL and _call(m, 1, 2, 1, p, 1, 0, 0) == EINVAL       # fewer temperatures than classes
    assert _call(m, 0, 0, 1, None, 1, 0, 0) == EINVAL
    bad = np.array([T0, np.nan, T0])
    assert _call(m, 0, 1, 3, bad.ctypes.data_as(_DP), 1, 0, 0) == EINVAL      # a NaN temperature
    assert _call(m, 2, 0, 1, p, 1, 0, 0) == EUNSUPPORTED and b"JUTTNER" in m.lib.ddcmi_last_error(m.ctx)
    assert np.array_equal(vel(m), v0)      # a refused call changes nothing
    with pytest.raises(DdcmiError):
        m.thermalize("JUTTNER", T0)
    m.close()


def test_rescale_refuses_more_than_512_classes():
    """1 + groups + species > 512: RESCALE is refused (its sums are ddcmi_momentum_by_class's), BOLTZMANN, which sums nothing, runs"""
    s = gas(65)
    ns = 520
    s.nspecies, s.species_name = ns, ["S%d" % k for k in range(ns)]
    s.mass = np.resize(s.mass, ns)
    s.charge = np.zeros(ns)
    s.ljtype, s.moltype, s.resitype, s.atomoffset = np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
    s.nmoltype = 0
    m = make(s)
    v0 = vel(m)
    t = np.full(ns, T0)
    p = t.ctypes.data_as(_DP)
    assert _call(m, 1, 0, ns, p, 1, 0, 0) == -4 and np.array_equal(vel(m), v0)
    assert _call(m, 0, 1, ns, p, 1, 0, 0) == 0 and np.all(np.any(vel(m) != v0, axis=1))
    m.close()

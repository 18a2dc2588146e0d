"""One NGLF step in plain numpy, given the forces -- written from the formulas of nglf.c:74-108 (half kick, drift, forces, half
kick, kinetic terms, group update), free.c, berendsen.c:30-89 and langevin.c:92-128, not from the oracle's C restatement and not from
the device code.  Forces are an input: they are tested elsewhere.

    ref = NGLFReference(setup)          # positions, velocities, species masses, group table, clock of the Setup
    ref.publish()                       # eval_energyInfo's group branch: the temperatures BERENDSEN reads (energyInfo.c:139)
    ref.front(f); ref.back(f_new)       # one step: f the forces at the old positions, f_new those at the drifted ones

A group is FREE (v += dt/2 f/m), BERENDSEN (v *= lambda at the FRONT kick of a step whose predecessor set doScaling; lambda from the
average of the temperatures PUBLISHED since the last scaling: a batch of steps without a publication adds the same one again) or
LANGEVIN (a = exp(-dt/2 / tau), c = dt/2 / m, d = sqrt(2 dt/2 kB Teq / (m tau)), kB = 1;
FRONT v = vcm + a (v - vcm) + c f + d g, BACK v = vcm + a ((v - vcm) + c f + d g), g three unit normals per bead and half kick).
The normals come from the counter-based stream of ddcmi.h (key smix64(seed ^ smix64(gid)) + 4 counter, counter 2 loop on FRONT with
the loop count before the step's increment and 2 loop + 1 on BACK with the one after it, Box-Muller) or from the beads' own LCG64
streams (pyoracle.gasdev3d, pinned by test_lcg64_streams_known_answers).

State and updates are float64 like the code under test (about ten roundings per bead and step); every sum over beads is formed in
np.longdouble.  The second half of the module builds the systems and group tables the integrator tests share."""
import copy

import numpy as np

from ddcmd_amd.deck import units_convert
from ddcmd_amd.synth import make_water_setup

FREE, BERENDSEN, LANGEVIN = 0, 1, 2
_LD = np.longdouble


def smix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def counter_normals(seed, gid, counter):
    """[3, n] unit normals of the counter-based stream: u_k = ((smix64(key + k) >> 11) + 1/2) 2^-53, k = 0..3;
    g0 = r cos t, g1 = r sin t with r = sqrt(-2 ln u0), t = 2 pi u1; g2 = sqrt(-2 ln u2) cos(2 pi u3)"""
    gid = np.asarray(gid, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = smix64(np.uint64(seed) ^ smix64(gid)) + np.uint64(4) * np.uint64(counter)
        u = [((smix64(key + np.uint64(k)) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0) for k in range(4)]
    twopi = 6.283185307179586476925
    r, t = np.sqrt(-2.0 * np.log(u[0])), twopi * u[1]
    return np.stack([r * np.cos(t), r * np.sin(t), np.sqrt(-2.0 * np.log(u[2])) * np.cos(twopi * u[3])])


def class_sums(cls, ncl, m, v):
    """[ncl, 12] = {rk, tion xx yy zz xy xz yz, mass, number, J x y z} per class (energy.c:104-147; per-atom U and S are zero on
    this path, so J = sum K v), in long double"""
    m, v = m.astype(_LD), v.astype(_LD)
    K = 0.5 * m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    cols = [K, m * v[0] * v[0], m * v[1] * v[1], m * v[2] * v[2], m * v[0] * v[1], m * v[0] * v[2], m * v[1] * v[2],
            m, np.ones_like(m), K * v[0], K * v[1], K * v[2]]
    out = np.zeros((ncl, 12), _LD)
    for c in range(ncl):
        sel = cls == c
        for k, col in enumerate(cols):
            out[c, k] = col[sel].sum()
    return out


def class_scale(m, v):
    """the size every column of class_sums is measured against (tests/test_integrator_closed_forms.py check_kinetic_detail): the
    system's kinetic energy, sum m v^2, mass, 1 for the count, sum K max|v| for the flux"""
    K = 0.5 * m * (v ** 2).sum(axis=0)
    return np.array([K.sum()] + [np.sum(m * (v ** 2).sum(axis=0))] * 6 + [m.sum(), 1.0] + [np.abs(K * np.abs(v).max()).sum()] * 3)


class NGLFReference(object):
    def __init__(self, s, lcg=None):
        self.n = int(s.natoms)
        self.dt = float(s.dt)
        self.loop = int(s.loop)
        self.m = np.asarray(s.mass, dtype=np.float64)[np.asarray(s.species)]
        self.species, self.nspecies = np.asarray(s.species), int(s.nspecies)
        self.group, self.ngroup = np.asarray(s.group), int(s.ngroup)
        self.gid = np.asarray(s.gid, dtype=np.uint64)
        self.r = np.stack([np.array(x, dtype=np.float64) for x in (s.rx, s.ry, s.rz)])
        self.v = np.stack([np.array(x, dtype=np.float64) for x in (s.vx, s.vy, s.vz)])
        self.kind = np.asarray(s.group_type).astype(int)
        self.Teq = np.asarray(s.group_Teq, dtype=np.float64)
        self.tau = np.asarray(s.group_tau, dtype=np.float64)
        self.interval = np.maximum(1, np.asarray(s.group_interval).astype(int))
        vcm = getattr(s, "group_vcm", None)
        self.vcm = np.zeros((self.ngroup, 3)) if vcm is None else np.asarray(vcm, dtype=np.float64).reshape(self.ngroup, 3)
        self.seed = int(getattr(s, "rng_seed", 0))
        self.lcg = None if lcg is None else np.array(lcg, copy=True)      # LCG64 records, advanced by the draws
        # berendsen.c's per-group scalars and the temperature last published
        self.lam = np.ones(self.ngroup)
        self.Tsum = np.zeros(self.ngroup)
        self.nT = np.zeros(self.ngroup, int)
        self.doScaling = np.zeros(self.ngroup, int)
        self.T = np.zeros(self.ngroup)
        self.rk, self.tion = 0.0, np.zeros(6)
        self._lang = self.kind[self.group] == LANGEVIN

    # -- publications ---------------------------------------------------------------------------------------------------------
    def publish(self):
        """T_g = 2 rk_g / (3 n_g) of the groups that hold a bead; an empty group keeps what it had (0 from the start)"""
        cs = class_sums(self.group, self.ngroup, self.m, self.v)
        for g in range(self.ngroup):
            if cs[g, 8] > 0:
                self.T[g] = float(2.0 * cs[g, 0] / (3.0 * cs[g, 8]))
        return self.T.copy()

    def kinetic_detail(self, by_species):
        if by_species:
            return class_sums(self.species, self.nspecies, self.m, self.v)
        return class_sums(self.group, self.ngroup, self.m, self.v)

    def scale(self):
        return class_scale(self.m, self.v)

    # -- the two halves of a step ---------------------------------------------------------------------------------------------
    def _normals(self, counter):
        idx = np.flatnonzero(self._lang)
        if self.lcg is None:
            return idx, counter_normals(self.seed, self.gid[idx], counter)
        import pyoracle
        g = np.zeros((3, idx.size))
        for q, i in enumerate(idx):
            g[:, q] = pyoracle.gasdev3d(self.lcg[i:i + 1])
        return idx, g

    def _langevin(self, f, counter, back):
        idx, g = self._normals(counter)
        if idx.size == 0:
            return
        gr = self.group[idx]
        dth = 0.5 * self.dt
        a = np.exp(-dth / self.tau[gr])
        c = dth / self.m[idx]
        d = np.sqrt(2.0 * dth * self.Teq[gr] / (self.m[idx] * self.tau[gr]))
        w = self.vcm[gr].T
        u = self.v[:, idx] - w
        if back:
            self.v[:, idx] = w + a * (u + c * f[:, idx] + d * g)
        else:
            self.v[:, idx] = w + a * u + c * f[:, idx] + d * g

    def front(self, f):
        """nglf.c:74-95: FRONT velocityUpdate(dt/2) of every bead's group, drift, clock"""
        f = np.asarray(f, dtype=np.float64)
        scaled = (self.kind[self.group] == BERENDSEN) & (self.doScaling[self.group] == 1)
        self.v[:, scaled] *= self.lam[self.group[scaled]]
        plain = ~self._lang
        self.v[:, plain] += (0.5 * self.dt / self.m[plain]) * f[:, plain]
        self._langevin(f, 2 * self.loop, False)
        self.r += self.dt * self.v
        self.loop += 1

    def back(self, f):
        """nglf.c:98-108: BACK velocityUpdate(dt/2), kinetic_terms, the groups' Update(FRONT_TIMESTEP)"""
        f = np.asarray(f, dtype=np.float64)
        plain = ~self._lang
        self.v[:, plain] += (0.5 * self.dt / self.m[plain]) * f[:, plain]
        self._langevin(f, 2 * self.loop + 1, True)
        tot = class_sums(np.zeros(self.n, int), 1, self.m, self.v)[0]
        self.rk, self.tion = float(tot[0]), tot[1:7].astype(np.float64)
        dth = 0.5 * self.dt
        for g in np.flatnonzero(self.kind == BERENDSEN):
            self.Tsum[g] += self.T[g]
            self.nT[g] += 1
            Tave = self.Tsum[g] / self.nT[g]
            ratio = 0.0 if Tave == 0 else self.Teq[g] / Tave
            self.lam[g] = np.sqrt(1.0 + (2.0 * dth / self.tau[g]) * (ratio - 1.0)) if self.tau[g] != 0 else np.sqrt(ratio)
            self.doScaling[g] = 0
            if self.loop % self.interval[g] == 0:
                self.Tsum[g], self.nT[g], self.doScaling[g] = 0.0, 0, 1


# ---- the systems and group tables of the integrator tests -----------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)      # either side of 64 (wave), 256 and 1024 (the kick kernels' blocks)
TABLE_SIZES = (65, 257, 1025)
_K = units_convert(1.0, "K")
_PS = units_convert(1.0, "ps")
_MP = units_convert(1.0, "M_p")
_VTH = float(np.sqrt(50.0 * _K / (72.0 * _MP)))      # thermal speed of the boxes' start


def _six(g):
    """the six kinds of the `mixed` table, constants varied with the group id g so that no two slots hold the same numbers"""
    w = 1.0 + 0.03 * (g // 6)
    return [dict(kind=FREE),
            dict(kind=BERENDSEN, Teq=310.0 * w * _K, tau=1.0 * w * _PS, interval=1),
            dict(kind=BERENDSEN, Teq=150.0 * w * _K, tau=0.3 * w * _PS, interval=3),
            dict(kind=LANGEVIN, Teq=310.0 * w * _K, tau=1.0 * w * _PS),
            dict(kind=LANGEVIN, Teq=200.0 * w * _K, tau=0.25 * w * _PS, vcm=(0.5 * w * _VTH, -0.25 * _VTH, 0.75 * _VTH)),
            dict(kind=BERENDSEN, Teq=100.0 * w * _K, tau=0.0, interval=1)][g % 6]


def group_table(name, n):
    """(list of groups, group of every bead) of the named table for n beads"""
    i = np.arange(n)
    if name == "mixed":
        return [_six(g) for g in range(6)], i % 6
    if name == "all-32":
        return [_six(g) for g in range(32)], (7 * i) % 32
    if name == "holes":
        # groups 2 (BERENDSEN) and 5 (LANGEVIN) hold no bead
        kinds = [_six(0), _six(1), _six(2), _six(3), _six(4), _six(9), _six(5), _six(6)]
        return kinds, np.array([0, 1, 3, 4, 6, 7])[i % 6]
    if name == "free+equal-berendsen":
        # every factor is 1 on the steps whose loop count is a multiple of neither interval (1, 5, 7): those a batch may fuse
        b = dict(kind=BERENDSEN, Teq=310.0 * _K, tau=1.0 * _PS)
        return [dict(kind=FREE), dict(b, interval=2), dict(b, interval=3)], i % 3
    if name == "free":
        return [dict(kind=FREE)] * 3, i % 3
    if name == "two-berendsen":
        return [_six(1), _six(8)], i % 2
    raise ValueError(name)


_BOXES = {}


def _box(nbox):
    if nbox not in _BOXES:
        _BOXES[nbox] = make_water_setup(nbox)
    return _BOXES[nbox]


def make_system(n, table, interacting, loop=0, lcg=False, nbox=None):
    """the first n beads of a water box (nbox = 7, 1372 beads; 9 above that; 33 for the 131 073 of the stride case): three species of
    different mass on the one LJ type, species i % 3, the named group table; not interacting: eps = 0, beads fly freely"""
    nbox = nbox or (7 if n <= 1372 else 9 if n <= 2916 else 33)
    s = copy.copy(_box(nbox))
    for k in ("rx", "ry", "rz", "vx", "vy", "vz", "gid"):
        setattr(s, k, np.array(getattr(s, k)[:n]))
    s.natoms = n
    s.nspecies = 3
    s.species_name = ["A", "B", "C"]
    s.mass = np.array([72.0, 36.0, 110.0]) * _MP
    s.charge = np.zeros(3)
    s.ljtype = np.array([1, 1, 1], np.int32)
    s.moltype = np.zeros(3, np.int32)
    s.resitype = np.zeros(3, np.int32)
    s.atomoffset = np.zeros(3, np.int32)
    s.species = (np.arange(n) % 3).astype(np.int32)
    if not interacting:
        s.eps = np.zeros_like(s.eps)
        s.shift = np.zeros_like(s.shift)
    groups, gr = group_table(table, n)
    s.ngroup = len(groups)
    s.group_name = ["g%d" % g for g in range(s.ngroup)]
    s.group = gr.astype(np.int32)
    s.group_type = np.array([g["kind"] for g in groups], np.int32)
    s.group_Teq = np.array([g.get("Teq", 0.0) for g in groups])
    s.group_tau = np.array([g.get("tau", 0.0) for g in groups])
    s.group_interval = np.array([g.get("interval", 1) for g in groups], np.int32)
    s.group_vcm = np.array([g.get("vcm", (0.0, 0.0, 0.0)) for g in groups])
    s.rng_seed = 20261018
    s.loop = int(loop)
    s.lcg64 = None
    if lcg:
        import pyoracle
        s.lcg64 = pyoracle.lcg64_default(s.gid)
    return s


def gates(ref):
    """the tolerances of one comparison: (v, r, per-column scale of the sums)"""
    return 1e-12 * np.abs(ref.v).max(), 1e-10, 1e-12 * ref.scale()


def compare(ref, s, r, v, rk, tion, T, det_group, det_species, worst=None, what=""):
    """hold one engine's state and sums against the reference's; worst (a dict) collects the largest deviation per gate, as a
    fraction of the gate"""
    L = np.array([s.h[0], s.h[4], s.h[8]])[:, None]
    gv, gr, gs = gates(ref)
    dev = {}
    dev["v"] = np.abs(np.asarray(v) - ref.v).max() / gv
    d = np.asarray(r) - ref.r
    d -= L * np.rint(d / L)
    dev["r"] = np.abs(d).max() / gr
    if rk is not None:
        dev["rk"] = abs(rk - ref.rk) / gs[0]
        dev["tion"] = np.abs(np.asarray(tion) - ref.tion).max() / gs[1]
    if T is not None:
        cnt = np.bincount(ref.group, minlength=ref.ngroup).astype(float)
        # a temperature is 2 rk_g / (3 n_g): its error, brought back to the group's kinetic energy, against the system's
        dev["T"] = float(np.max(np.abs(np.asarray(T) - ref.T) * 1.5 * np.maximum(cnt, 1.0) / gs[0]))
    for key, got, by_species in (("detail_group", det_group, 0), ("detail_species", det_species, 1)):
        if got is not None:
            want = ref.kinetic_detail(by_species)
            assert got.shape == want.shape, (key, got.shape, want.shape)
            dev[key] = float(np.max(np.abs(got - want.astype(np.float64)) / gs[None, :]))
    if worst is not None:
        for k, x in dev.items():
            worst[k] = max(worst.get(k, 0.0), float(x))
    bad = {k: float(x) for k, x in dev.items() if not x < 1.0}
    assert not bad, "%s: deviation / gate %r" % (what, bad)
    return dev

"""Systems for the GROUP kinds that are no thermostat -- FROZEN, FIXEDVELOCITY, QUENCH (helper module, no tests in here).

The idea of tests/restraint_systems.py: a gas whose pair terms vanish identically (eps = 0, shift = 0, no charge) in a box of three
unequal sides, with harmonic restraints as the only force -- the force on every bead is known in closed form
(restraint_systems.reference, restraint.c:297-354 in longdouble), so the integrator's kinds can be held bead by bead against a
reference that owes nothing to the device code.

  * `gas(n, table)`: n beads on a jittered lattice, thermal velocities, every bead of a group that feels forces restrained to an
    anchor up to 3 A away in every component (periods of 40 ... 60 steps; QUENCH beads: 160 ... 240).  n sits at the edges of the kick kernels' tiling: SIZES
    (64 = a wave, 256 = a block of k_kick_drift, 1024 = a block of k_kick_ke x KE_PER, 4097 = four of those and one bead).
  * the group tables (`table(name, n)`): "all": the six kinds, group = bead index % 8 (two QUENCH groups and two FIXEDVELOCITY groups: one with a
    vector, one without), so that every wave holds every kind; "last:<kind>": everybody FREE but the bead of the last index;
    "frozen-fast": the frozen beads store velocities a hundred times thermal; "old": FREE, BERENDSEN, LANGEVIN only, and
    "old+empty-frozen": the same with a FROZEN group that holds no bead; "pull": FIXEDVELOCITY groups whose vectors take the beads across every periodic face within 60
    steps (and across every face of a grid of twos).
  * `quench_cases()`: hand-placed QUENCH beads, one per case and component: v f < 0, v f > 0, f = 0 (fc = 0 in that component), v = +0.0,
    v = -0.0, and a product that underflows to zero (|v| = 1e-200 against a force of 1e-160 internal units).

Units: internal (the Setup's)."""
import numpy as np

import restraint_systems as R
from ddcmd_amd.deck import Setup, units_convert

FREE, BERENDSEN, LANGEVIN, OTHER, FROZEN, FIXEDVELOCITY, QUENCH = range(7)
KIND_NAMES = {FROZEN: "FROZEN", FIXEDVELOCITY: "FIXEDVELOCITY", QUENCH: "QUENCH"}
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
ANG = R.ANG
_K = units_convert(1.0, "K")
_PS = units_convert(1.0, "ps")
_MP = units_convert(1.0, "M_p")
T0 = 310.0 * _K
VTH = float(np.sqrt(T0 / (72.0 * _MP)))          # thermal speed of the heavier species
DIMS = (17, 17, 15)


def _lattice(rng, n):
    """n beads on a jittered 17 x 17 x 15 lattice of the 48 x 56 x 64 A box (cells of 2.8 ... 4.3 A, jitter of a quarter cell), A; the
    order is shuffled so that the first n beads of any n fill the box"""
    L = np.array(R.BOX_A)
    dims = np.array(DIMS)
    assert n <= dims.prod()
    k = rng.permutation(dims.prod())[:n]
    ijk = np.stack([k % dims[0], (k // dims[0]) % dims[1], k // (dims[0] * dims[1])], 1)
    return -0.5 * L + (ijk + 0.5) * L / dims + rng.uniform(-0.25, 0.25, (n, 3)) * L / dims


def table(name, n):
    """(list of group dicts, group of every bead)"""
    i = np.arange(n)
    lang = dict(kind=LANGEVIN, Teq=T0, tau=1.0 * _PS)
    ber = dict(kind=BERENDSEN, Teq=T0, tau=1.0 * _PS, interval=1)
    if name == "all":
        groups = [dict(kind=FREE), ber, lang, dict(kind=FROZEN), dict(kind=FIXEDVELOCITY, v=(0.7 * VTH, -0.4 * VTH, 0.55 * VTH)),
                  dict(kind=QUENCH), dict(kind=QUENCH), dict(kind=FIXEDVELOCITY)]
        return groups, i % 8
    if name.startswith("last:"):
        kind = int(name[5:])
        g1 = dict(kind=kind)
        if kind == FIXEDVELOCITY:
            g1["v"] = (-0.3 * VTH, 0.8 * VTH, 0.1 * VTH)
        return [dict(kind=FREE), g1], (i == n - 1).astype(int)
    if name == "frozen-fast":
        return [dict(kind=FREE), dict(kind=FROZEN), dict(kind=QUENCH)], np.array([0, 1, 2, 0, 1])[i % 5]
    if name == "old":
        return [dict(kind=FREE), ber, lang], i % 3
    if name == "old+empty-frozen":
        return [dict(kind=FREE), ber, lang, dict(kind=FROZEN)], i % 3
    if name == "free+berendsen":
        return [dict(kind=FREE), ber], i % 2
    if name == "free+berendsen+empty-frozen":
        return [dict(kind=FREE), ber, dict(kind=FROZEN)], i % 2
    if name == "pull":
        # 60 steps of 20 fs: 0.45 ... 0.6 A per step is 27 ... 36 A, more than half of every side (24, 28, 32 A): every bead crosses a
        # periodic face or the mid plane (the internal face of a grid of twos) or both, in + and in - direction
        a = ANG / units_convert(20.0, "fs")
        return [dict(kind=FIXEDVELOCITY, v=(0.45 * a, 0.5 * a, 0.6 * a)), dict(kind=FIXEDVELOCITY, v=(-0.45 * a, -0.5 * a, -0.6 * a)),
                dict(kind=FIXEDVELOCITY), dict(kind=FREE)], i % 4
    raise ValueError(name)


def gas(n, tab="all", seed=20261020, update_rate=20, v_frozen=1.0):
    """module docstring.  s.feels[i]: bead i is restrained; s.kind_of[i]: its group's kind"""
    rng = np.random.RandomState(seed + n)
    s = Setup()
    R._forcefield(s, update_rate)
    groups, gr = table(tab, n)
    r = _lattice(rng, n)
    species = (np.arange(n) // 8 % 2).astype(np.int32)
    mass = s.mass[species]
    v = rng.normal(size=(n, 3)) * np.sqrt(T0 / mass)[:, None]
    kind_of = np.array([g["kind"] for g in groups])[gr]
    if tab == "frozen-fast":
        v[kind_of == FROZEN] *= 100.0 * v_frozen
    if tab == "pull":
        v[gr == 2] = rng.choice([-1.0, 1.0], ((gr == 2).sum(), 3)) * np.array([0.45, 0.5, 0.6]) * ANG / s.dt      # the unset form coasts across the faces
    R._finish(s, r, v, rng, species)
    s.group = gr.astype(np.int32)
    s.ngroup = len(groups)
    s.group_name = ["g%d" % g for g in range(s.ngroup)]
    s.group_type = np.array([g["kind"] for g in groups], np.int32)
    s.group_Teq = np.array([g.get("Teq", 0.0) for g in groups])
    s.group_tau = np.array([g.get("tau", 0.0) for g in groups])
    s.group_interval = np.array([g.get("interval", 1) for g in groups], np.int32)
    s.group_vcm = np.zeros((s.ngroup, 3))
    s.group_vset = np.array([1 if "v" in g else 0 for g in groups], np.int32)
    s.group_v = np.array([g.get("v", (0.0, 0.0, 0.0)) for g in groups], float).ravel()
    s.rng_seed = 20261020
    # restraints on every bead -- but none in "pull" (the anchors would be left tens of A behind)
    free = np.full(n, tab == "pull")
    bead = np.flatnonzero(~free)
    bead = bead[rng.permutation(len(bead))]
    nb = len(bead)
    s.feels = ~free
    s.kind_of = kind_of
    if nb > 0:
        disp = rng.uniform(0.5, 3.0, (nb, 3)) * rng.choice([-1.0, 1.0], (nb, 3))
        period = rng.uniform(40.0, 60.0, nb)
        # QUENCH beads: 160 ... 240 steps.  A quenched oscillator closes in on its anchor by a constant factor per crossing, speed and
        # force shrinking together; with a quarter period of 40 steps and more, 40 steps hold one crossing at most, and no product
        # v f comes near the roundings (group_kind_reference: margin)
        period = np.where(kind_of[bead] == QUENCH, rng.uniform(160.0, 240.0, nb), period)
        w = 2.0 * np.pi / (period * s.dt)
        kb = mass[bead] * w * w / 2.0 / R.KB_UNIT
        R._set_restraints(s, bead, np.ones((nb, 3), np.int32), r[bead] - disp, kb)
    else:
        s.nrest = 0
    s.name = "kinds_gas%d_%s" % (n, tab)
    return s


CASES = ("vf<0", "vf>0", "f=0", "v=+0", "v=-0", "underflow")


def quench_cases(seed=7):
    """18 hand-placed QUENCH beads (case x component; the other two components of a bead are plain v f > 0 motion) among 110 more
    QUENCH and FREE beads.  s.case[k] = (bead, component, case name).  The underflow bead carries a restraint of kb so small that
    |f| = 2 kb |d| is about 1e-160 internal units, and |v| = 1e-200: the product is below the smallest subnormal and rounds to zero
    with either sign"""
    rng = np.random.RandomState(seed)
    n = 128
    s = gas(n, "last:%d" % QUENCH, seed=seed)
    gr = (np.arange(n) % 2).astype(np.int32)          # QUENCH on the odd beads, the last bead among them
    s.group = gr
    s.kind_of = np.where(gr == 1, QUENCH, FREE)
    r = R.positions(s) / ANG
    v = np.stack([s.vx, s.vy, s.vz], 1).copy()
    L = np.array(R.BOX_A)
    x0 = np.asarray(s.rest_r0).reshape(-1, 3).copy() * L - 0.5 * L          # anchors, A
    kb = np.asarray(s.rest_kb).copy()
    fc = np.asarray(s.rest_fc).reshape(-1, 3).copy()
    slot = {int(b): k for k, b in enumerate(s.rest_bead)}
    cases = []
    beads = np.flatnonzero(gr == 1)[:18]
    for q, b in enumerate(beads):
        comp, case = q % 3, CASES[q // 3]
        k = slot[int(b)]
        d = r[b] - x0[k]                              # f = -2 kb d
        for c in range(3):                            # plain components: moving towards the anchor, v f > 0
            v[b, c] = -np.sign(d[c]) * abs(v[b, c])
        if case == "vf<0":
            v[b, comp] = np.sign(d[comp]) * abs(v[b, comp])
        elif case == "f=0":
            fc[k, comp] = 0                           # (f = -2 kb fc d: an exact zero, of either sign)
        elif case == "v=+0":
            v[b, comp] = 0.0
        elif case == "v=-0":
            v[b, comp] = -0.0
        elif case == "underflow":
            kb[k] = 1e-160 / (2.0 * 2.0 * ANG)
            for c in range(3):
                x0[k, c] = r[b, c] - 2.0 * (1 if c % 2 else -1)      # |d| = 2 A in every component: |f| = 1e-160
                v[b, c] = 1e-200 * (1.0 if (q + c) % 2 else -1.0) * np.sign(r[b, c] - x0[k, c])      # + and - products: both round to zero
        cases.append((int(b), comp, case))
    s.vx, s.vy, s.vz = (np.ascontiguousarray(v[:, c]) for c in range(3))
    s.rest_r0 = np.ascontiguousarray((x0 + 0.5 * L) / L)
    s.rest_kb = kb
    s.rest_fc = np.ascontiguousarray(fc, np.int32)
    s.case = cases
    s.name = "quench_cases"
    return s


_made = {}


def system(name, *args):
    """the named builder's Setup, made once and left unchanged"""
    key = (name,) + args
    if key not in _made:
        _made[key] = globals()[name](*args)
    return _made[key]

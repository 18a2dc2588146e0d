"""GPU tests (-m gpu) of the GROUP kinds FROZEN, FIXEDVELOCITY and QUENCH in the split integrator kernels (k_kick_drift,
k_kick_ke, k_kick_ke_drift) on the systems of tests/group_kind_systems.py: a gas whose only force is a harmonic restraint per bead,
held bead by bead against the longdouble reference of tests/group_kind_reference.py (itself held against closed forms by
tests/test_group_kinds_host.py).  docs/group_kind_variants.md lists the mutations of the kernels these tests catch.

Bounds, derived once (u = 2^-53):
  * a force component: restraint_systems.force_bound -- eight roundings at the size of the box side in the displacement, 4 u of the force;
  * one half kick v = fma(a, f, v): one rounding, u |v|, plus a times the force's error; one drift r = fma(dt, v, r): one rounding,
    u |r|, plus dt times the velocity's error; a rebuild wraps a coordinate: one more rounding at the size of the box side;
  * a harmonic well under the leapfrog carries an error (dr, dv) on without growth in the norm sqrt(dr^2 + dv^2 / w^2) (up to the
    factor 1 + w dt / 2 between that norm and the one the leapfrog conserves), and QUENCH's zeroing -- taken at the same steps by both,
    see `margin` -- only removes error.  After N steps, with w the slowest frequency of the system's wells:
        |dr| <= (1 + w dt) N (e_r + e_v / w),   |dv| <= w_max (the same),   e_r = 2 u L,  e_v = 2 (u v_max + a e_f).
    FIXEDVELOCITY with a vector has no force and no velocity error: |dr| <= N u max|r| (one ulp of the coordinate per step; the
    reference's own longdouble roundings are 2^-11 of that).  The positions leave the box by at most a few A between rebuilds, so max|r| is taken
    as the longest side."""
import copy
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import group_kind_systems as G
import restraint_systems as R
from group_kind_reference import KindReference
from restraint_systems import LD, U
from ranks import ROOT, rank_env, run_ranks

pytestmark = pytest.mark.gpu
_IP = ctypes.POINTER(ctypes.c_int)
_DP = ctypes.POINTER(ctypes.c_double)


def make(s, **kw):
    from ddcmd_amd.martini import MartiniHIP
    return MartiniHIP(s, **kw)


def state(m):
    d = m.download()
    return {k: np.stack(d[k], 1) for k in ("r", "v", "f")}


def bits(m):
    st = state(m)
    e, vir, rk, tion = m.energies()
    return [st["r"], st["v"], st["f"], np.array([e[k] for k in sorted(e)]), np.asarray(vir), np.array([rk]), np.asarray(tion)]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def set_groups(m, kinds):
    k = np.ascontiguousarray(kinds, np.int32)
    z = np.zeros(len(k))
    one = np.ones(len(k), np.int32)
    tau = np.ones(len(k))
    return m.lib.ddcmi_set_groups(m.ctx, len(k), k.ctypes.data_as(_IP), z.ctypes.data_as(_DP), tau.ctypes.data_as(_DP), one.ctypes.data_as(_IP))


def traj_bound(s, nsteps, nrebuild):
    """module docstring: (|dr|, |dv|) bounds after nsteps for the restrained beads"""
    L = float(R.box_of(s).max())
    m = np.asarray(s.mass)[np.asarray(s.species)]
    kb = np.asarray(s.rest_kb)
    w = np.sqrt(2.0 * kb / m[np.asarray(s.rest_bead)])          # kb |d|^2: the well's frequency
    w_min, w_max = float(w.min()), float(w.max())
    vmax = float(max(np.abs(np.stack([s.vx, s.vy, s.vz])).max(), 3.5 * G.ANG * w_max))
    fmax = float(2 * kb.max() * 4.0 * G.ANG)
    e_f = 2 * kb.max() * 8 * U * L + 4 * U * fmax
    e_v = 2 * (U * vmax + (0.5 * s.dt / m.min()) * e_f)
    e_r = 2 * U * L
    dr = (1 + w_max * s.dt) * (nsteps * (e_r + e_v / w_min) + nrebuild * U * L)
    return float(dr), float(w_max * dr)


# ---- 1. refusals and acceptance -------------------------------------------------------------------------------------------
def test_set_groups_accepts_the_three_kinds():
    """fails on the code before these kinds: ddcmi_set_groups refused everything but 0, 1, 2"""
    s = G.system("gas", 65, "old")
    m = make(s)
    for kind in (4, 5, 6):
        assert set_groups(m, [0, kind, 0]) == 0, (kind, m.lib.ddcmi_last_error(m.ctx))
    assert set_groups(m, [4, 5, 6, 0, 1, 2]) == 0
    for kind in (3, 7, 8, -1):
        rc = set_groups(m, [0, kind, 0])
        assert rc != 0 and b"group 1" in m.lib.ddcmi_last_error(m.ctx), kind
    m.close()


def test_setters_refuse_and_change_nothing():
    """NaN, a wrong group count, a call before ddcmi_set_groups: refused; the next steps are those of a context never so called"""
    s = G.system("gas", 257, "all")
    ng = s.ngroup
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    clean = make(s)
    clean.eval_forces()
    clean.step(3)
    want = bits(clean)
    clean.close()
    m = make(s)
    lib, ctx = m.lib, m.ctx
    vset, v = i32(s.group_vset), f64(s.group_v)
    bad_v = v.copy()
    bad_v[3 * 4 + 1] = np.nan
    other = f64(np.full(3 * ng, 0.123))
    assert lib.ddcmi_set_group_velocity(ctx, ng, vset.ctypes.data_as(_IP), bad_v.ctypes.data_as(_DP)) != 0
    assert b"not finite" in lib.ddcmi_last_error(ctx)
    for n_bad in (ng - 1, ng + 1, 0, 33):
        assert lib.ddcmi_set_group_velocity(ctx, n_bad, i32(np.ones(40)).ctypes.data_as(_IP), f64(np.full(120, 0.123)).ctypes.data_as(_DP)) != 0
    assert lib.ddcmi_set_group_velocity(ctx, ng, None, other.ctypes.data_as(_DP)) != 0
    m.eval_forces()
    m.step(3)
    assert same(bits(m), want)
    m.close()
    # before ddcmi_set_groups: a fresh context (one FREE group by default)
    from ddcmd_amd import _lib
    from ddcmd_amd.martini import _declare
    lib = _lib.load_library()
    _declare(lib)
    c = ctypes.c_void_p()
    assert lib.ddcmi_create(ctypes.byref(c), 0) == 0
    one_i, three = i32([1]), f64([0.1, 0.2, 0.3])
    assert lib.ddcmi_set_group_velocity(c, 1, one_i.ctypes.data_as(_IP), three.ctypes.data_as(_DP)) != 0
    assert b"after ddcmi_set_groups" in lib.ddcmi_last_error(c)
    lib.ddcmi_destroy(c)


# ---- 2. FROZEN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_rate", [20, 0], ids=["rate20", "neighborCheck"])
def test_frozen(update_rate):
    """60 steps: the frozen beads' positions and velocities are the upload's, bit for bit (in calls of 1 and 9 steps: k_kick_ke_drift
    inside a call, k_kick_ke and k_kick_drift at its ends).  Their stored velocities, a hundred times thermal, are in the kinetic energy and in
    their group's temperature; the displacement bound does not contain them and covers every bead that moves.  updateRate = 0: no
    rebuild is asked for by them -- at their stored speed (several A per step) they would ask for one every step"""
    s = copy.copy(G.system("gas", 1025, "frozen-fast"))
    s.updateRate = update_rate
    m = make(s, test_api=True)
    m.lib.ddcmi_debug_disp.argtypes = [ctypes.c_void_p, _DP, ctypes.POINTER(ctypes.c_float), _IP]
    fr = s.kind_of == G.FROZEN
    r0 = R.positions(s)
    v0 = np.stack([s.vx, s.vy, s.vz], 1)
    L = R.box_of(s)
    assert (np.abs(r0) < 0.5 * L).all() and fr.sum() > 400
    assert np.abs(v0[fr]).max() * s.dt > 5.0 * G.ANG          # several A per step, were they to move
    m.eval_forces()
    moved = np.zeros(s.natoms)
    mass = np.asarray(s.mass)[s.species]
    free = s.kind_of == G.FREE

    def disp_bound():
        D, ring, nr = ctypes.c_double(0), (ctypes.c_float * 32)(), ctypes.c_int(0)
        m._chk(m.lib.ddcmi_debug_disp(m.ctx, ctypes.byref(D), ring, ctypes.byref(nr)))
        return D.value
    for block in range(6):
        m.step(1)
        a, Da = state(m), disp_bound()
        m.step(9)
        b, Db = state(m), disp_bound()
        for st in (a, b):
            assert np.array_equal(st["r"][fr], r0[fr]) and np.array_equal(st["v"][fr], v0[fr]), block
        assert np.abs(b["f"][fr]).min() > 0          # a force acts on them all the same
        d = np.sqrt((R.min_image(b["r"] - a["r"], L) ** 2).sum(axis=1))
        moved = np.maximum(moved, d)
        if update_rate == 20 and block % 2 == 0:
            # no rebuild inside these nine steps: the bound grew by dt max|v| of (at least) the eight drifts behind the call's first,
            # which k_kick_ke_drift makes; the first one's length is known for a FREE bead: dt |v + a f|
            first = s.dt * np.sqrt(((a["v"] + ((0.5 * s.dt) / mass)[:, None] * a["f"]) ** 2).sum(axis=1))
            grew = Db - Da
            assert grew > 0 and (d[free] <= grew * (1 + 1e-6) + first[free] * (1 + 1e-9)).all(), (block, grew)
            assert grew < 0.2 * 8 * s.dt * np.abs(v0[fr]).max(), ("the bound holds the frozen beads' stored speed", grew)
    assert moved[~fr].min() > 0 and (moved[fr] == 0).all()
    e, vir, rk, tion = m.energies()
    st = state(m)
    K = 0.5 * mass * (st["v"] ** 2).sum(axis=1)
    assert abs(rk - K.sum()) <= 1e-12 * K.sum() and K[fr].sum() > 100 * K[~fr].sum()
    T = m.group_temperatures()
    want = 2.0 * K[fr].sum() / (3.0 * fr.sum())
    assert abs(T[1] - want) <= 1e-12 * want and T[1] > 1000 * G.T0
    nreb = m.list_stats()["rebuilds"]
    m.close()
    if update_rate == 20:
        assert nreb == 4
    else:
        # neighborCheck: as many rebuilds as the same system asks for with the frozen beads' stored velocities at zero (the moving
        # beads' paths are the same: nothing couples them)
        z = copy.copy(s)
        z.vx, z.vy, z.vz = (np.where(fr, 0.0, x) for x in (s.vx, s.vy, s.vz))
        mz = make(z)
        mz.eval_forces()
        for block in range(6):
            mz.step(1)
            mz.step(9)
        assert nreb == mz.list_stats()["rebuilds"] and nreb < 40, (nreb, mz.list_stats()["rebuilds"])
        mz.close()


def test_frozen_single_bead_at_the_last_index():
    """bead counts at the edges of the tiling, the one FROZEN bead at the last index: it stays, everybody else moves"""
    for n in G.SIZES:
        s = G.system("gas", n, "last:%d" % G.FROZEN)
        m = make(s)
        m.eval_forces()
        m.step(1)
        m.step(4)
        st = state(m)
        assert np.array_equal(st["r"][-1], R.positions(s)[-1]) and np.array_equal(st["v"][-1], [s.vx[-1], s.vy[-1], s.vz[-1]]), n
        if n > 1:
            assert (np.abs(st["r"][:-1] - R.positions(s)[:-1]).max(axis=1) > 0).all(), n
        m.close()


# ---- 3. FIXEDVELOCITY ------------------------------------------------------------------------------------------------------
def _pull_check(s, r, v, nsteps, what):
    L = R.box_of(s)
    r0 = R.positions(s)
    v0 = np.stack([s.vx, s.vy, s.vz], 1)
    vec = np.asarray(s.group_v).reshape(-1, 3)
    for g in (0, 1, 2):
        sel = s.group == g
        vg = np.broadcast_to(vec[g], (sel.sum(), 3)) if g < 2 else v0[sel]
        assert np.array_equal(v[sel], vg), (what, g)          # the set vector exactly; the unset form: the start's velocity, untouched
        # the reference's chain: r_k+1 = fma(dt, v, r_k) in longdouble; the device's: the same in float64 -- at most one ulp of the
        # coordinate per step (module docstring), the coordinate bounded by the longest side plus what a bead travels between two wraps
        want = r0[sel].astype(LD) + LD(nsteps) * LD(s.dt) * vg.astype(LD)
        d = (r[sel].astype(LD) - want) / L.astype(LD)
        d = (d - np.rint(d)) * L
        bound = nsteps * 2 * U * (L.max() + 20 * s.dt * np.abs(vg).max())
        err = float(np.abs(d).max())
        print("%s group %d: largest |r - r_ref| %.3e, bound %.3e" % (what, g, err, bound))
        assert err <= bound, (what, g, err, bound)
    return r0


def test_fixed_velocity_single_domain():
    """60 steps, one at a time: after EVERY step the velocities of the two groups with a vector are that vector and those of the
    group without one are the start's, exactly; every bead of the three FIXEDVELOCITY groups crosses a periodic face or a mid plane"""
    s = G.system("gas", 1025, "pull")
    m = make(s)
    m.eval_forces()
    vec = np.asarray(s.group_v).reshape(-1, 3)
    v0 = np.stack([s.vx, s.vy, s.vz], 1)
    for k in range(60):
        m.step(1)
        v = state(m)["v"]
        assert np.array_equal(v[s.group == 0], np.broadcast_to(vec[0], ((s.group == 0).sum(), 3))), k
        assert np.array_equal(v[s.group == 1], np.broadcast_to(vec[1], ((s.group == 1).sum(), 3))), k
        assert np.array_equal(v[s.group == 2], v0[s.group == 2]), k
    st = state(m)
    r0 = _pull_check(s, st["r"], st["v"], 60, "one domain")
    L = R.box_of(s)
    travelled = 60 * s.dt * np.abs(vec[0])
    assert (travelled > 0.5 * L).all()          # every bead of groups 0 .. 2 meets a periodic face or the mid plane, in + or in -
    for a in range(3):
        for g in (0, 1):
            x = r0[s.group == g, a]
            sign = 1.0 if g == 0 else -1.0
            assert ((sign * x + travelled[a] > 0.5 * L[a]).sum() > 20) and ((sign * x < 0) & (sign * x + travelled[a] > 0)).sum() > 20
    m.close()


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1), (2, 2, 2)], ids=["2", "4", "8"])
def test_fixed_velocity_domains(grid):
    """the same pull on 2 / 4 / 8 in-process domains: the beads cross every domain face (the mid planes) and every periodic face,
    migrating with their group index; a second run repeats the first bit for bit"""
    from ddcmd_amd.martini import MartiniGroup
    s = G.system("gas", 1025, "pull")
    out = []
    for rep in range(2):
        g = MartiniGroup(s, grid)
        g.eval_forces()
        g.step(60)
        got = g.gather()
        out.append([R.to_setup_order(s, np.stack(got[k], 1)) for k in ("r", "v")])
        g.close()
    _pull_check(s, out[0][0], out[0][1], 60, "grid %s" % (grid,))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 4. QUENCH -------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))          # correctly rounded: what the device's fma gives


def test_quench_first_step_decisions_exact():
    """the hand-placed beads after one step, bit for bit: from the forces the device itself reports before and after the step,
    v1 = kick(kick(v0, f0), f1) with kick(v, f) = fma(a, f, (v f < 0) ? 0 : v) evaluated exactly -- every decision of both half
    kicks, per component: v f < 0, v f > 0, f = 0, v = +0.0, v = -0.0, a product that underflows to zero with either sign"""
    s = G.system("quench_cases")
    m = make(s)
    m.eval_forces()
    f0 = state(m)["f"]
    m.step(1)
    st = state(m)
    f1, v1, r1 = st["f"], st["v"], st["r"]
    v0 = np.stack([s.vx, s.vy, s.vz], 1)
    r0 = R.positions(s)
    mass = np.asarray(s.mass)[s.species]
    ncase = {}
    for b, comp, case in s.case:
        a = (0.5 * s.dt) * (1.0 / mass[b])
        for c in range(3):
            with np.errstate(under="ignore"):
                z0 = v0[b, c] * f0[b, c] < 0.0
            vf = _fma(a, f0[b, c], 0.0 if z0 else v0[b, c])
            assert r1[b, c] == _fma(s.dt, vf, r0[b, c]), (b, c, case)
            with np.errstate(under="ignore"):
                z1 = vf * f1[b, c] < 0.0
            want = _fma(a, f1[b, c], 0.0 if z1 else vf)
            assert v1[b, c] == want and np.signbit(v1[b, c]) == np.signbit(want), (b, c, case, v1[b, c], want)
            if c == comp:
                assert z0 == (case == "vf<0"), (b, c, case)
                ncase[case] = ncase.get(case, 0) + 1
    assert ncase == {c: 3 for c in G.CASES}
    m.close()


@pytest.mark.parametrize("n", [257, 4097])
def test_quench_against_reference(n):
    """the six-kind table: every QUENCH, FROZEN, FIXEDVELOCITY and FREE bead against the longdouble reference after 1 step
    and after 40 (a rebuild at step 20), to the derived bounds; the reference's decisions sit far from a rounding (margin), so the
    device takes the same ones -- a bead that took another would be off by its whole velocity"""
    s = G.system("gas", n, "all")
    ref = KindReference(s)
    m = make(s)
    m.eval_forces()
    held = np.isin(s.kind_of, (G.FREE, G.FROZEN, G.FIXEDVELOCITY, G.QUENCH))
    L = R.box_of(s)
    done = 0
    for nsteps in (1, 39):
        m.step(nsteps)
        ref.step(nsteps)
        done += nsteps
        st = state(m)
        dr, dv = traj_bound(s, done, done // 20 + 1)
        er = np.abs(R.min_image((st["r"] - ref.r.T.astype(np.float64)), L))[held].max()
        ev = float(np.abs(st["v"].astype(LD) - ref.v.T)[held].max())
        print("n %d step %d: |r - r_ref| %.3e (bound %.3e), |v - v_ref| %.3e (bound %.3e), margin %.2e" % (n, done, er, dr, ev, dv, ref.margin))
        assert er <= dr and ev <= dv, (done, er, dr, ev, dv)
        q = s.kind_of == G.QUENCH
        assert np.array_equal(st["v"][q] == 0.0, ref.v.T[q] == 0)
    assert ref.margin > 1e-9, ref.margin
    assert sum(int(d.sum()) for d in ref.decisions) > 10          # components were zeroed on the way
    m.close()


# ---- 5. bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1025, 4097])
def test_batched_steps_equal_single_steps_and_repeat(n):
    """ddcmi_step_nglf with n = 10 (k_kick_ke_drift between the steps) equals ten calls with n = 1 (k_kick_ke, then k_kick_drift) for
    the table with all six kinds, bit for bit; the same setup run twice gives the same bits"""
    s = G.system("gas", n, "all")
    runs = []
    for mode in ("batch", "single", "batch"):
        m = make(s)
        m.eval_forces()
        if mode == "batch":
            m.step(10)
            m.step(10)
            m.step(5)
        else:
            for _ in range(25):
                m.step(1)
        runs.append(bits(m))
        m.close()
    assert same(runs[0], runs[2]), "two runs of the same setup"
    assert same(runs[0], runs[1]), "step(10) against ten step(1)"
    q = s.kind_of == G.QUENCH
    assert (runs[0][1][q] != 0).any()


@pytest.mark.parametrize("pair", [("free+berendsen", "free+berendsen+empty-frozen"), ("old", "old+empty-frozen")], ids=["fused", "langevin"])
def test_empty_frozen_group_changes_nothing(pair):
    """a FROZEN group that holds no bead sends the context down the split kernels (fuse_ok) and sets a kind mask no bead tests
    positive for: positions, velocities, forces and every sum equal, bit for bit, those of the run without it -- for FREE and
    BERENDSEN groups that is the fused pair-kernel epilogue against the split kernels, for a LANGEVIN table the split kernels with
    and without the masks"""
    out = []
    for tab in pair:
        s = G.system("gas", 1025, tab)
        m = make(s)
        m.eval_forces()
        m.group_temperatures()
        m.step(10)
        m.step(1)
        m.step(14)
        out.append(bits(m))
        m.close()
    assert same(out[0], out[1])


def test_domains_repeat_with_all_kinds():
    """4 in-process domains, the six-kind table, 40 steps with two rebuilds: two runs give the same bits; the frozen beads have not
    moved, the dragged ones carry their vector"""
    from ddcmd_amd.martini import MartiniGroup
    s = G.system("gas", 1025, "all")
    out = []
    for rep in range(2):
        g = MartiniGroup(s, (2, 2, 1))
        g.eval_forces()
        g.step(40)
        got = g.gather()
        out.append([R.to_setup_order(s, np.stack(got[k], 1)) for k in ("r", "v", "f")])
        g.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    r, v, _ = out[0]
    fr = s.kind_of == G.FROZEN
    assert np.array_equal(r[fr], R.positions(s)[fr]) and np.array_equal(v[fr], np.stack([s.vx, s.vy, s.vz], 1)[fr])
    assert np.array_equal(v[s.group == 4], np.broadcast_to(np.asarray(s.group_v).reshape(-1, 3)[4], ((s.group == 4).sum(), 3)))
    # the single domain computes the same trajectory (another order of the force's roundings: to the trajectory bound)
    m = make(s)
    m.eval_forces()
    m.step(40)
    st = state(m)
    dr, dv = traj_bound(s, 40, 3)
    det = np.isin(s.kind_of, (G.FREE, G.FROZEN, G.FIXEDVELOCITY, G.QUENCH))
    assert np.abs(R.min_image(st["r"] - r, R.box_of(s)))[det].max() <= 2 * dr and np.abs(st["v"] - v)[det].max() <= 2 * dv
    m.close()


@pytest.mark.parametrize("table, nsteps", [("all", 40), ("pull", 60)])
def test_host_transport_equals_the_in_process_group(tmp_path, table, nsteps):
    """two processes over the host transport (2, 1, 1) against the in-process group of the same grid: positions, velocities and forces
    bit for bit.  Both set new vectors for the FIXEDVELOCITY groups after the contexts exist (MartiniRank / MartiniGroup
    .set_group_velocity: the per-group tables belong to every rank's context), and the dragged beads carry the NEW vector"""
    from ddcmd_amd.martini import MartiniGroup
    import group_kind_worker as W
    s = G.system("gas", 1025, table)
    grid, factor = (2, 1, 1), 0.75
    d = str(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "group_kind_worker.py"), table, "1025", "2x1x1", d, str(nsteps), repr(factor)]
    run_ranks([cmd] * 2, [rank_env(r, 2, d) for r in range(2)], timeout=240, check=True)
    recs = [np.load(os.path.join(d, "rank%d.npz" % r)) for r in range(2)]
    gid = np.concatenate([x["gid"] for x in recs])
    order = np.argsort(gid, kind="stable")
    assert np.array_equal(gid[order], np.sort(np.asarray(s.gid, np.uint64)))
    host = [R.to_setup_order(s, np.concatenate([x[k] for x in recs], 1).T[order]) for k in ("r", "v", "f")]
    g = MartiniGroup(s, grid)
    g.set_group_velocity(*W.new_vectors(s, factor))
    g.eval_forces()
    g.step(nsteps)
    got = g.gather()
    g.close()
    for name, a, b in zip("rvf", host, [R.to_setup_order(s, np.stack(got[k], 1)) for k in ("r", "v", "f")]):
        assert np.array_equal(a, b), "host transport against the in-process group: %s differs" % name
    vec = np.asarray(s.group_v).reshape(-1, 3) * factor
    for grp in np.flatnonzero(np.asarray(s.group_vset)):
        assert np.array_equal(host[1][s.group == grp], np.broadcast_to(vec[grp], ((s.group == grp).sum(), 3))), grp
    assert min(len(x["gid"]) for x in recs) > 100


# ---- 6. the refused pairing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [4, 5, 6])
@pytest.mark.parametrize("with_what", ["barostat", "constraints"])
def test_new_kinds_refuse_constraints_and_barostat(kind, with_what):
    """DDCMI_EUNSUPPORTED (its number is read from include/ddcmi.h) with a message that names the group; the state is what it was"""
    from ddcmd_amd.martini import DdcmiError
    s = G.system("gas", 257, "last:%d" % kind)
    if with_what == "constraints":
        po = np.array([0, 1], np.int32)
        m = make(s, constraint_groups=(po, np.array([0], np.int32), np.array([1], np.int32), np.array([np.linalg.norm(R.positions(s)[0] - R.positions(s)[1])])))
    else:
        m = make(s)
        m.set_barostat(G.T0, 0.0, 1e-6, 1000.0)
    m.eval_forces()
    before = bits(m)
    text = open(os.path.join(ROOT, "include", "ddcmi.h")).read()
    code = int(re.search(r"DDCMI_EUNSUPPORTED\s*=\s*(-?\d+)", text).group(1))
    rc = m.lib.ddcmi_step_nglf(m.ctx, float(s.dt), 3)
    assert rc == code, rc
    msg = m.lib.ddcmi_last_error(m.ctx).decode()
    assert "group 1" in msg and ("constraint" in msg or "barostat" in msg), msg
    with pytest.raises(DdcmiError):
        m.step(1)
    assert same(bits(m), before)
    m.close()

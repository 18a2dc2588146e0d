"""GPU tests (-m gpu) of the RESTRAINT potential -- k_rest_locate, k_restraint and the two places its force lands (the record array in
front of the pair kernel; fx, fy, fz when excludePotentialTerm & 128 switches the pair kernel off) -- on the restraint sets of
tests/restraint_systems.py: a gas in which the restraint force is all the force there is, held bead by bead and sum by sum against a
longdouble reference written from restraint.c:297-354 (tests/test_restraint_systems_host.py holds that reference against its own
finite differences and the oracle).  docs/restraint_variants.md records eleven mutations of the kernel and which of these tests each
turns red.

Tolerances, derived and written once (R.force_bound, R.sum_bound): a displacement component carries at most eight roundings at the
size of the box side (the product r0 L, the - L / 2, the subtraction from the position, the wrap -- a product, a rint and a
subtraction -- and the position itself), hence |f - f_ref| <= 2 kb |fc| 8 u L_a + 4 u |f_ref| per component, u = 2^-53 (a bead with
several restraints: on the sum of the absolute contributions, the atomics may add in any order); the energy and each of the six
virial sums within (n + 16) u of the reference's sum of absolute terms.  Trajectories: 16 times the float64-against-longdouble
difference measured on the CPU (R.TRAJ_R_MEASURED, R.TRAJ_V_MEASURED)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import restraint_systems as R
from restraint_systems import LD, U
from restraint_worker import run_blocks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["-".join(str(x) for x in k) for k in R.STEP0_SETS]
TOL_R = R.TRAJ_FACTOR * R.TRAJ_R_MEASURED
TOL_V = R.TRAJ_FACTOR * R.TRAJ_V_MEASURED


def with_path(s, off):
    """off: excludePotentialTerm bit 128 -- no pair kernel, the restraint force goes to fx, fy, fz"""
    s = copy.copy(s)
    s.excludePotentialTerm = 128 if off else 0
    return s


def state(m):
    d = m.download()
    return {k: np.stack(d[k], 1) for k in ("r", "v", "f")}


def hold(s, r, f, e, vir, box, tag, gas=True, f_extra=None, ref=None):
    """per-bead force, restraint energy and the six virial sums against the reference AT the positions r, to the derived bounds; on
    the gas e[total] - e[restraint] == 0 and a force whose bound is zero (an unrestrained bead, a component with fc = 0) is 0.0"""
    ref = R.reference(s, r, box, s.pbc) if ref is None else ref
    fb = R.force_bound(s, ref, box)
    bound = fb if f_extra is None else fb + f_extra
    err = np.abs(np.asarray(f, LD) - ref["F"])
    eb, vb = R.sum_bound(s, ref)
    de, dv = abs(LD(e["restraint"]) - ref["E"]), np.abs(np.asarray(vir, LD) - ref["V"])
    pos = bound > 0
    print("%s: largest |f - f_ref| / bound %.3f, |E - E_ref| / bound %.3f, virial / bound %s" %
          (tag, float((err[pos] / bound[pos]).max()) if pos.any() else 0.0, float(de / eb) if eb > 0 else 0.0,
           np.array2string(np.asarray(dv / np.where(vb > 0, vb, 1), float), precision=3)))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (tag, "force beyond the bound", bad[:5].tolist(), np.asarray(f)[bad[0][0]], np.asarray(ref["F"][bad[0][0]], float))
    if gas:
        quiet = fb == 0
        assert (np.asarray(f)[quiet] == 0.0).all(), (tag, "a force on an unrestrained bead or on a component with fc = 0")
        assert e["total"] - e["restraint"] == 0.0, (tag, e)
        assert (dv <= vb).all(), (tag, "virial", np.asarray(vir), np.asarray(ref["V"], float))
    assert de <= eb, (tag, "energy", e["restraint"], float(ref["E"]))
    return ref


@pytest.mark.parametrize("off", [False, True], ids=["fb", "pair_off"])
@pytest.mark.parametrize("key", R.STEP0_SETS, ids=IDS)
def test_step0(key, off):
    """every count (1, 255, 256, 257, 600: one, two and a ragged third trip of the kernel's loop) and every edge set, on both paths"""
    from ddcmd_amd.martini import MartiniHIP
    s = with_path(R.system(*key), off)
    m = MartiniHIP(s)
    e, vir = m.eval_forces()
    st = state(m)
    hold(s, st["r"], st["f"], e, vir, m.box(), "%s %s" % (s.name, "pair kernel off" if off else "record array"))
    assert np.array_equal(m.box(), R.box_of(s))
    m.close()


@pytest.mark.parametrize("off", [False, True], ids=["fb", "pair_off"])
def test_duplicates_and_the_unknown_gid(off):
    """two and three restraints on one bead: the bead's force is their sum (bound on the sum of the absolute contributions).  The gid
    no bead carries is accepted and contributes nothing (include/ddcmi.h): a context whose ONLY restraint names it reports an energy,
    a virial and forces of exactly zero"""
    from ddcmd_amd.martini import MartiniHIP
    s = with_path(R.system("duplicates"), off)
    m = MartiniHIP(s)
    e, vir = m.eval_forces()
    st = state(m)
    ref = hold(s, st["r"], st["f"], e, vir, m.box(), "duplicates")
    for b in s.dup_beads:          # (the bead's force is no single restraint's)
        assert all(np.abs(st["f"][b] - np.asarray(ref["f"][k], float)).max() > 1e-3 * np.abs(st["f"][b]).max() for k in np.flatnonzero(s.rest_bead == b))
    m.close()
    k = int(np.flatnonzero(s.rest_bead < 0)[0])
    lone = copy.copy(s)
    lone.nrest = 1
    for name in ("rest_gid", "rest_fc", "rest_r0", "rest_kb", "rest_bead"):
        setattr(lone, name, getattr(s, name)[k:k + 1].copy())
    m = MartiniHIP(lone)
    e, vir = m.eval_forces()
    assert e["restraint"] == 0.0 and e["total"] == 0.0 and (vir == 0.0).all() and (state(m)["f"] == 0.0).all()
    m.close()


@pytest.mark.parametrize("off", [False, True], ids=["fb", "pair_off"])
def test_trajectory(off):
    """60 steps of the oscillators, a rebuild every 10: after every 10 steps the downloaded state against NGLFReference driven by the
    reference's forces (tolerance: module docstring), and the downloaded forces and the sums against the reference at the downloaded
    positions to the step-0 bound -- a slot map that was not refreshed at a rebuild shows there.  step(1) x 10 and step(10) give
    identical bits"""
    s = with_path(R.system("oscillators"), off)
    a = run_blocks(s)
    b = run_blocks(s, single_steps=True)
    assert int(a["rebuilds"][0]) == 7
    run = R.LDReference(s)
    box = R.box_of(s)
    for k in range(6):
        rr, vr = run.step(10)
        r, v, f = a["r%d" % k], a["v%d" % k], a["f%d" % k]
        dr = np.abs(R.min_image(r - rr, box)).max()
        dv = np.abs(v - vr).max()
        print("step %d: largest |r - r_ref| %.3e A (tolerance %.3e), |v - v_ref| %.3e (tolerance %.3e)" % (10 * k + 10, dr / R.ANG, TOL_R / R.ANG, dv, TOL_V))
        assert dr <= TOL_R and dv <= TOL_V, (k, dr, dv)
        e = {"restraint": a["e%d" % k][0], "total": a["e%d" % k][1]}
        hold(s, r, f, e, a["vir%d" % k], box, "oscillators step %d" % (10 * k + 10))
        R.assert_guard(s, r)
    for key in sorted(a):
        assert np.array_equal(a[key], b[key]), ("step(10) against ten step(1)", key)
    moved = np.abs(R.min_image(a["r5"] - R.positions(s), box)).max(axis=1)
    assert (moved[s.rest_bead] > 1.0 * R.ANG).sum() > 250


def test_fused_and_split_step_agree(tmp_path):
    """DDCMI_NO_FUSED_STEP=1 (read once per process: a child process, under a time limit) against this process: identical bits"""
    s = R.system("oscillators")
    a = run_blocks(s)
    env = dict(os.environ)
    env["DDCMI_NO_FUSED_STEP"] = "1"
    out = str(tmp_path / "split.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "restraint_worker.py"), out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "restraint_worker ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    b = dict(np.load(out))
    for key in sorted(a):
        assert np.array_equal(a[key], b[key]), key


def gathered(s, g):
    st = g.gather()
    assert np.array_equal(st["gid"], np.sort(np.asarray(s.gid)))
    return {k: R.to_setup_order(s, np.stack(st[k], 1)) for k in ("r", "v", "f")}, st["nlocal"]


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)], ids=["2x1x1", "2x2x2"])
@pytest.mark.parametrize("name", ["faces", "oscillators"])
def test_decomposed(name, grid):
    """an in-process group of domains: gathered forces, summed restraint energy and virial against the reference at step 0 and after
    the run (every restraint once: a halo copy of a restrained bead is never counted), and the end state against the one-domain
    run of the same system to the trajectory tolerance.  oscillators: 60 steps, beads cross periodic and internal faces with their
    anchors on the far side.  faces: 20 steps; its tolerance is 16 times the same CPU measurement, float64 against longdouble under
    the reference's forces, taken on that system over those steps"""
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP
    s = R.system("faces", 7, 0) if name == "faces" else R.system("oscillators")
    nsteps = 20 if name == "faces" else 60
    if name == "faces":
        mr, mv = R.measure_trajectory_tolerance(s, nsteps)
        tol_r, tol_v = R.TRAJ_FACTOR * mr, R.TRAJ_FACTOR * mv
    else:
        tol_r, tol_v = TOL_R, TOL_V
    box = R.box_of(s)
    g = MartiniGroup(s, grid)
    e, vir = g.eval_forces()
    st, nloc = gathered(s, g)
    tag = "%s %dx%dx%d" % ((name,) + grid)
    hold(s, st["r"], st["f"], e, vir, box, tag + " step 0")
    m = MartiniHIP(s)
    m.eval_forces()
    for _ in range(nsteps // 10):
        g.step(10); m.step(10)
    e, vir, _, _ = g.energies()
    st, nloc2 = gathered(s, g)
    hold(s, st["r"], st["f"], e, vir, box, tag + " step %d" % nsteps)
    one = state(m)
    dr = np.abs(R.min_image(st["r"] - one["r"], box)).max()
    dv = np.abs(st["v"] - one["v"]).max()
    print("%s: against one domain |dr| %.3e A (tolerance %.3e), |dv| %.3e (tolerance %.3e); beads per domain %s -> %s" % (tag, dr / R.ANG, tol_r / R.ANG, dv, tol_v, nloc, nloc2))
    assert dr <= tol_r and dv <= tol_v, (tag, dr, dv)
    if name == "oscillators":
        # (that beads change domains is proved on the host: test_oscillators_swing_through_cells_faces_and_domains)
        assert g.ranks[0].list_stats()["rebuilds"] == 7
    g.close(); m.close()


@pytest.mark.parametrize("no_bead", [False, True], ids=["no_restrained", "no_bead"])
def test_emptied_domain_reports_nothing(no_bead):
    """(2, 1, 1): the cluster of restrained beads drifts out of the first domain (no_bead: nobody else lives there).  After every 10
    steps each domain's own restraint energy and virial against the reference's terms of the beads it owns, the group's against the
    reference; once the first domain holds no restrained bead -- or no bead at all -- its restraint energy and virial are 0.0: not its
    last value"""
    from ddcmd_amd.martini import MartiniGroup
    s = R.system("emptying", no_bead)
    box = R.box_of(s)
    g = MartiniGroup(s, s.grid)
    g.eval_forces()
    index = {int(x): i for i, x in enumerate(np.asarray(s.gid).tolist())}
    first = []
    for call in range(4):
        if call:
            g.step(10)
        e, vir, _, _ = g.energies()
        st, nloc = gathered(s, g)
        ref = hold(s, st["r"], st["f"], e, vir, box, "%s step %d" % (s.name, 10 * call))
        for rank, ctx in enumerate(g.ranks):
            own = np.zeros(s.natoms, bool)
            own[[index[int(x)] for x in ctx.download_particles()["gid"].tolist()]] = True
            mine = own[s.rest_bead]
            er, vr, _, _ = ctx.energies()
            k = (s.nrest + 16) * U
            E, V = ref["e"][mine].sum(), ref["vir"][mine].sum(axis=0)
            print("%s step %d rank %d: %d beads, %d restrained, restraint energy %.6e (reference %.6e)" % (s.name, 10 * call, rank, own.sum(), mine.sum(), er["restraint"], float(E)))
            assert abs(er["restraint"] - E) <= k * np.abs(ref["e"][mine]).sum(), (call, rank, er["restraint"], float(E))
            assert (np.abs(vr - V) <= k * np.abs(ref["vir"][mine]).sum(axis=0)).all(), (call, rank, vr, np.asarray(V, float))
            if rank == 0:
                first.append((int(own.sum()), int(mine.sum()), er["restraint"], vr.copy()))
    assert first[0][1] == len(s.cluster) and first[0][2] > 0
    assert first[-1][1] == 0 and (first[-1][0] == 0) == bool(no_bead)
    assert first[-1][2] == 0.0 and (first[-1][3] == 0.0).all(), first[-1]
    g.close()


def test_box_change_moves_the_anchors():
    """five NGLFCONSTRAINT barostat steps (the exaggerated compressibility of test_nglfconstraint_barostat_matches_oracle) on the gas
    with weak restraints: forces and sums against the reference at the downloaded positions and m.box() -- the anchors are r0 L of
    the CURRENT box; the box moved by more than 1e-4 relative"""
    from ddcmd_amd.deck import units_convert
    from ddcmd_amd.martini import MartiniHIP
    s = copy.copy(R.system("soft_gas"))
    s.npt_T = units_convert(310.0, "K")
    s.npt_P0 = units_convert(1.0, "bar")
    s.npt_beta = units_convert(3.0e-4, "1/bar") * 50.0
    s.npt_tau = units_convert(1.0, "ps")
    m = MartiniHIP(s)
    e, vir = m.eval_forces()
    L0 = m.box().copy()
    st = state(m)
    hold(s, st["r"], st["f"], e, vir, L0, "soft gas step 0")
    m.step(1)
    m.step(4)
    e, vir, _, _ = m.energies()
    L1 = m.box().copy()
    st = state(m)
    print("box %s -> %s A" % (L0 / R.ANG, L1 / R.ANG))
    assert (np.abs(L1 - L0) > 1e-4 * L0).all() and (np.abs(L1 - L0) < 0.2 * L0).all()
    hold(s, st["r"], st["f"], e, vir, L1, "soft gas after 5 barostat steps")
    m.close()


def census(m):
    import ctypes
    out = ((ctypes.c_int * 12) * 2)()
    m.lib.ddcmi_debug_bonded_layout.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert m.lib.ddcmi_debug_bonded_layout(m.ctx, ctypes.byref(out)) == 0
    return np.array([list(out[0]), list(out[1])])


@pytest.mark.parametrize("lds", [True, False], ids=["lds_tables", "no_lds_tables"])
def test_lipid(lds, monkeypatch):
    """the relaxed lipid deck, a restraint on every seventh bead: the forces with the restraints minus the forces without them equal the
    reference's restraint forces, per bead, for beads of the light bonded launch (it STORES its beads' records: the restraints must come
    behind it), of the heavy one and for beads without bonded rows -- within 8 u of the bead's total |f| plus the step-0 bound;
    restraint energy and the difference of the virials as on the gas.  With the bonded tables in LDS and without"""
    from ddcmd_amd.martini import MartiniHIP
    if lds:
        monkeypatch.delenv("DDCMI_NO_BONDED_LDS_TABLES", raising=False)
    else:
        monkeypatch.setenv("DDCMI_NO_BONDED_LDS_TABLES", "1")
    s, s0 = R.system("lipid")
    m1, m0 = MartiniHIP(s, test_api=True), MartiniHIP(s0, test_api=True)
    e1, v1 = m1.eval_forces()
    e0, v0 = m0.eval_forces()
    a, b = state(m1), state(m0)
    assert np.array_equal(a["r"], b["r"])
    cen = census(m1)
    assert cen[0][0] > 0 and cen[1][0] > 0 and [int(cen[0][10]), int(cen[1][10])] == [int(lds)] * 2, cen
    kind = R.bonded_kinds(s)
    assert np.bincount(kind[s.rest_bead], minlength=3).min() >= 5
    box = m1.box()
    ref = R.reference(s, a["r"], box, s.pbc)
    df = np.asarray(a["f"], LD) - np.asarray(b["f"], LD)
    ftot = np.sqrt((a["f"] ** 2).sum(axis=1))
    bound = R.force_bound(s, ref, box) + 8 * U * ftot[:, None]
    err = np.abs(df - ref["F"])
    for q, what in enumerate(("no bonded rows", "light launch only", "heavy launch")):
        sel = np.zeros(s.natoms, bool)
        sel[s.rest_bead[kind[s.rest_bead] == q]] = True
        print("lipid, %s: %d restrained beads, largest error / bound %.3f" % (what, sel.sum(), float((err[sel] / bound[sel]).max())))
        assert (err[sel] <= bound[sel]).all(), what
    assert (err <= bound).all()
    eb, vb = R.sum_bound(s, ref)
    dv = np.abs((np.asarray(v1, LD) - np.asarray(v0, LD)) - ref["V"])
    print("lipid: |E - E_ref| / bound %.3f, virial difference / bound %s" % (float(abs(e1["restraint"] - ref["E"]) / eb), np.asarray(dv / vb, float)))
    assert abs(e1["restraint"] - ref["E"]) <= eb and e0["restraint"] == 0.0
    assert (dv <= vb).all()
    m1.close(); m0.close()

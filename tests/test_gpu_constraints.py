"""GPU tests (-m gpu) of k_constrain and of the molecular virial (k_mol_virial, k_mol_virial_gid, k_mol_split_term) on the groups and
molecules of tests/constraint_systems.py: a gas without forces, where the constraint impulse is all that changes a velocity, held bead
by bead against a longdouble reference written from nglfconstraint.c:180-264; and molecules whose only forces are the RESTRAINT
potential's, where pmol V - N kT must equal the device's virial minus the reference's molecular term to a derived bound
(C.pressure_bound).  Tolerances: 16 times the float64-against-longdouble difference measured on the CPU
(tests/test_constraint_systems_host.py).  docs/constraint_variants.md records what mutations of the kernels these tests catch."""
import copy
import ctypes

import numpy as np
import pytest

import constraint_systems as C
from constraint_systems import LD

pytestmark = pytest.mark.gpu
IDS = ["-".join(str(x) for x in k) for k in C.CONSTRAINT_SETS]
TOL_V1, TOL_R1 = C.FACTOR * C.VEL_MEASURED, C.FACTOR * C.POS_MEASURED
TOL_V, TOL_R = C.FACTOR * C.TRAJ_V_MEASURED, C.FACTOR * C.TRAJ_R_MEASURED


def state(m):
    d = m.download()
    return {k: np.stack(d[k], 1) for k in ("r", "v", "f")}


def hold(s, t, st, ref, box, dt, tol_r, tol_v, tag, v_before=None, sweeps=1):
    """positions and velocities against the reference bead by bead, every healthy pair at its length and at rest along itself, every
    group's momentum unchanged"""
    r, v, bx = ref[0], ref[1], np.asarray(ref[2], float)
    keep, ok = np.ones(s.natoms, bool), np.ones(len(t[1]), bool)
    for g in getattr(s, "stuck_groups", ()):
        keep[s.groups[g]] = False
        ok[t[0][g]:t[0][g + 1]] = False
    dr = np.abs(C.min_image((st["r"] - r).astype(float), bx, s.pbc))[keep].max()
    dv = float(np.abs(st["v"] - v)[keep].max())
    res_r, res_v = C.pair_residuals(st["r"], st["v"], t, dt, box, s.pbc)
    print("%s: |r - r_ref| %.3e A (tolerance %.3e), |v - v_ref| %.3e (tolerance %.3e), residuals %.3f %.3f tol" %
          (tag, dr / C.ANG, tol_r / C.ANG, dv, tol_v, float(res_r[ok].max() / C.TOL), float(res_v[ok].max() / C.TOL)))
    assert dr <= tol_r and dv <= tol_v, (tag, dr / C.ANG, dv)
    assert res_r[ok].max() <= C.LEN_MULT * C.TOL and res_v[ok].max() <= C.VEL_MULT * C.TOL, (tag, float(res_r[ok].max()), float(res_v[ok].max()))
    if v_before is not None:
        # every pair update adds +c to one bead's momentum and -c to the other's: what is left is rounding, two roundings of the size
        # of a bead's momentum per pair update and bead
        p0, p1 = C.group_momenta(s, v_before), C.group_momenta(s, st["v"])
        m = C.masses(s)
        for g, idx in enumerate(s.groups):
            bound = 4 * C.U * (2 * sweeps + 2) * len(idx) * np.abs(m[idx, None] * st["v"][idx]).max()
            assert (np.abs(p1[g] - p0[g]) <= bound).all(), (tag, "momentum of group", g, p1[g] - p0[g], bound)


@pytest.mark.parametrize("key", C.CONSTRAINT_SETS, ids=IDS)
def test_one_step(key):
    from ddcmd_amd.martini import MartiniHIP
    s, t = C.system(*key)
    m = MartiniHIP(s, constraint_groups=t)
    m.eval_forces()
    m.step(1)
    st = state(m)
    ref = C.reference_run(key, 1)
    most, unconv = m.constraint_stats()
    print("%s: %d sweeps (reference %d), %d unconverged" % (s.name, most, ref[3], unconv))
    hold(s, t, st, ref, m.box(), s.dt, TOL_R1, TOL_V1, s.name + " step 1", v_before=C.velocities(s), sweeps=most)
    assert abs(most - ref[3]) <= 1
    if key[0] == "slow":
        assert most >= 50 and unconv == 0
    elif key[0] == "stuck":
        # two groups, and the device counts a group once per solve it leaves unconverged: the FRONT solve cannot converge on the two
        # triangles, and what it leaves behind -- all but collinear -- defeats the BACK solve of the same step too, in the reference
        # as on the device: 2 groups x 2 solves.  The healthy groups were held to the tolerance above
        assert unconv == ref[5] == 2 * len(s.stuck_groups) and most == C.MAXIT
    else:
        assert unconv == 0
    m.close()


@pytest.mark.parametrize("key", C.TRAJ_SETS, ids=IDS)
def test_forty_steps(key):
    """every builder: 40 steps, a rebuild every 10 (slots are re-sorted); mixed-65 halves dt after 20.  stuck: its two triangles are left
    out of the comparison, as after one step, and every one of their 2 x 2 x 40 solves is counted"""
    from ddcmd_amd.martini import MartiniHIP
    s, t = C.system(*key)
    dts = C.traj_dts(s, key)
    m = MartiniHIP(s, constraint_groups=t)
    m.eval_forces()
    for k in range(0, C.NSTEPS, 10):
        m.step(10, dt=dts[k])
    st = state(m)
    ref = C.reference_run(key, C.NSTEPS)
    most, unconv = m.constraint_stats()
    print("%s: %d sweeps (reference %d), %d unconverged" % (s.name, most, ref[3], unconv))
    hold(s, t, st, ref, m.box(), dts[-1], TOL_R, TOL_V, s.name + " step 40")
    assert abs(most - ref[3]) <= 1 and unconv == ref[5] and m.list_stats()["rebuilds"] >= 4
    assert unconv == (2 * 2 * C.NSTEPS if key[0] == "stuck" else 0)
    m.close()


def test_barostat_scales_the_images():
    """faces(7) under a barostat that moves the box by about 3e-3 per step: partners that are periodic images are scaled by k_scale_pos"""
    from ddcmd_amd.martini import MartiniHIP
    s0, t = C.system("faces", 7)
    s = C.with_barostat(s0)
    m = MartiniHIP(s, constraint_groups=t)
    m.eval_forces()
    assert m.list_stats()["images"] > 0
    m.step(1)
    ref = C.step(s, t, 1, barostat=True)
    box = m.box()
    assert (np.abs(box / C.box_of(s) - 1) > 5e-4).all() and (np.abs(box - np.asarray(ref[2], float)) <= 8 * C.U * box).all(), box / C.box_of(s)
    hold(s, t, state(m), ref, box, s.dt, TOL_R1, TOL_V1, "faces(7) barostat step 1")
    m.step(9); m.step(10); m.step(20)
    ref = C.reference_run(("faces", 7), C.NSTEPS, True)
    box = m.box()
    assert (np.abs(box - np.asarray(ref[2], float)) <= 8 * C.NSTEPS * C.U * box).all()
    hold(s, t, state(m), ref, box, s.dt, TOL_R, TOL_V, "faces(7) barostat step 40")
    assert m.constraint_stats()[1] == 0
    m.close()


def test_too_large_is_refused_and_the_context_lives_on():
    from ddcmd_amd.martini import MartiniHIP, DdcmiError
    s, t = C.system("too_large")
    with pytest.raises(DdcmiError, match="error -2: constraint group of 19 atoms / 18 pairs exceeds the LDS budget"):
        MartiniHIP(s, constraint_groups=t)
    m = MartiniHIP(s)
    po, pi, pj, dd = t
    _ip, _dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    assert m.lib.ddcmi_set_constraints(m.ctx, 3, po.ctypes.data_as(_ip), pi.ctypes.data_as(_ip), pj.ctypes.data_as(_ip), dd.ctypes.data_as(_dp)) == -2
    assert b"exceeds the LDS budget" in m.lib.ddcmi_last_error(m.ctx)
    small = (po[:2].copy(), pi[:po[1]].copy(), pj[:po[1]].copy(), dd[:po[1]].copy())
    assert m.lib.ddcmi_set_constraints(m.ctx, 1, *[a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp) for a in small]) == 0
    m.eval_forces()
    m.step(1)
    st = state(m)
    ref = C.step(s, small, 1)
    assert np.abs(st["v"] - ref[1]).max() <= TOL_V1 and m.constraint_stats() == (ref[3], 0)
    m.close()


def test_partner_beyond_the_halo_is_refused():
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP, DdcmiError
    s, t = C.system("beyond_halo")
    g = MartiniGroup(s, s.grid, constraint_groups=t)
    for again in range(2):          # an error return, not a fault: the contexts answer the same way a second time ...
        with pytest.raises(DdcmiError, match="-4.*1 constraint groups have an atom on this domain and a partner beyond its halo"):
            g.eval_forces()
    # ... and still hold their beads and their box
    held = np.concatenate([rk.download_particles()["gid"] for rk in g.ranks])
    assert np.array_equal(np.sort(held), np.sort(np.asarray(s.gid))) and np.array_equal(g.ranks[0].box(), C.box_of(s))
    g.close()
    m = MartiniHIP(s, constraint_groups=t)      # one domain: every partner is here
    m.eval_forces(); m.step(1)
    assert m.constraint_stats()[1] == 0
    m.close()


def gathered(s, g):
    st = g.gather()
    assert np.array_equal(st["gid"], np.sort(np.asarray(s.gid)))          # every bead once
    return {k: R_order(s, np.stack(st[k], 1)) for k in ("r", "v", "f")}


def R_order(s, by_gid):
    return C.R.to_setup_order(s, by_gid)


@pytest.mark.parametrize("grid", C.GRIDS, ids=["2x1x1", "1x1x2", "2x2x2"])
def test_decomposed(grid):
    """groups across every internal face, one at the bricks' corner, some swinging through a face: the gathered state against the
    reference and against the one-domain run; every rank converged"""
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP, domain_of
    s, t = C.system("domains", grid)
    g = MartiniGroup(s, grid, constraint_groups=t)
    m = MartiniHIP(s, constraint_groups=t)
    g.eval_forces(); m.eval_forces()
    for _ in range(C.NSTEPS // 10):
        g.step(10); m.step(10)
    st, one = gathered(s, g), state(m)
    ref = C.reference_run(("domains", grid), C.NSTEPS)
    hold(s, t, st, ref, C.box_of(s), s.dt, TOL_R, TOL_V, "%s decomposed step 40" % s.name)
    dr = np.abs(C.min_image(st["r"] - one["r"], C.box_of(s))).max()
    dv = np.abs(st["v"] - one["v"]).max()
    print("against one domain: |dr| %.3e A |dv| %.3e" % (dr / C.ANG, dv))
    assert dr <= TOL_R and dv <= TOL_V
    c = s.groups[s.corner_group]
    assert np.abs(st["v"][c] - ref[1][c]).max() <= TOL_V
    for rk in g.ranks:
        assert rk.constraint_stats()[1] == 0
    after = copy.copy(s)
    after.rx, after.ry, after.rz = (np.ascontiguousarray(st["r"][:, a]) for a in range(3))
    moved = sum(set(domain_of(after, grid)[idx].tolist()) != set(domain_of(s, grid)[idx].tolist()) for idx in s.groups)
    assert moved >= 2, moved
    g.close(); m.close()


def test_barostat_scales_the_halo_of_a_decomposed_run():
    """domains(2, 1, 1) under the barostat: a one-domain solve never reads an image (its partners are owned slots under the minimum
    image), a decomposed one reads its partners' halo copies, which k_scale_pos must move with the box before the FRONT solve"""
    from ddcmd_amd.martini import MartiniGroup
    key = ("domains", (2, 1, 1))
    s0, t = C.system(*key)
    s = C.with_barostat(s0)
    g = MartiniGroup(s, s0.grid, constraint_groups=t)
    g.eval_forces()
    g.step(1)
    ref = C.reference_run(key, 1, True)
    box = g.ranks[0].box()
    assert (np.abs(box / C.box_of(s) - 1) > 5e-4).all() and (np.abs(box - np.asarray(ref[2], float)) <= 8 * C.U * box).all()
    hold(s, t, gathered(s, g), ref, box, s.dt, TOL_R1, TOL_V1, "domains(2, 1, 1) barostat step 1")
    g.step(9); g.step(10); g.step(20)
    ref = C.reference_run(key, C.NSTEPS, True)
    box = g.ranks[0].box()
    hold(s, t, gathered(s, g), ref, box, s.dt, TOL_R, TOL_V, "domains(2, 1, 1) barostat step 40")
    for rk in g.ranks:
        assert rk.constraint_stats()[1] == 0
    g.close()


# -- molecular virial --------------------------------------------------------------------------------------------------------------
def pressure(s, ctx, decomposed):
    """eval_forces, the state, the virial, one step with a tiny beta, barostat_pressure: (pmol V - N kT, r, f, virial diagonal, N kT)"""
    from ddcmd_amd.martini import molecule_lists
    ctx.eval_forces()
    st = gathered(s, ctx) if decomposed else state(ctx)
    vir = ctx.energies()[1][:3].copy()
    box = (ctx.ranks[0] if decomposed else ctx).box()
    ctx.step(1)
    p = (ctx.ranks[0] if decomposed else ctx).barostat_pressure()
    nkt = molecule_lists(s)[0] * s.npt_T
    return np.asarray(p, LD) * LD(np.prod(box)) - LD(nkt), st["r"], st["f"], vir, nkt, box


def hold_pressure(s, lhs, r, f, vir, nkt, box, tag):
    molv, _, _ = C.molecular_virial(s, r, f, box)
    bound = C.pressure_bound(s, r, f, box, vir, nkt)
    err = np.abs(lhs - (np.asarray(vir, LD) - molv))
    print("%s: |(pmol V - N kT) - (vir - molv)| / bound %s; molv / vir %s" % (tag, np.asarray(err / bound, float), np.asarray(molv / vir, float)))
    assert (err <= bound).all(), (tag, np.asarray(err, float), np.asarray(bound, float))
    return bound


MOL_SETS = [("molecules", n) for n in C.MOL_COUNTS] + [("molecules_faces", p) for p in C.PBCS]


@pytest.mark.parametrize("key", MOL_SETS, ids=["-".join(str(x) for x in k) for k in MOL_SETS])
def test_molecular_pressure(key):
    from ddcmd_amd.martini import MartiniHIP
    s = C.system(*key)
    m = MartiniHIP(s)
    lhs, r, f, vir, nkt, box = pressure(s, m, False)
    hold_pressure(s, lhs, r, f, vir, nkt, box, s.name)
    m.close()


@pytest.mark.parametrize("grid", C.GRIDS, ids=["2x1x1", "1x1x2", "2x2x2"])
def test_molecular_pressure_decomposed(grid):
    """molecules owned by 1, 2, 4 and 8 ranks: against the reference, against one domain, and the split term is seen: a reference
    that leaves (P / M) o F out for the split molecules is more than ten bounds away"""
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP
    s = C.system("molecules_split", grid)
    g = MartiniGroup(s, grid)
    lhs, r, f, vir, nkt, box = pressure(s, g, True)
    bound = hold_pressure(s, lhs, r, f, vir, nkt, box, s.name)
    m = MartiniHIP(s)
    one = pressure(s, m, False)
    assert (np.abs(lhs - one[0]) <= 2 * bound + np.abs(np.asarray(vir, LD) - np.asarray(one[3], LD))).all()
    own, _ = C.owners(s, grid)
    split = [k for k, o in enumerate(own) if len(o) > 1]
    assert len(split) == s.nsplit
    wrong, _, _ = C.molecular_virial(s, r, f, box, skip_pf=set(split))
    assert (np.abs(lhs - (np.asarray(vir, LD) - wrong)) > 10 * bound).any()
    g.close(); m.close()


def _run20(s, grid):
    from ddcmd_amd.deck import units_convert
    from ddcmd_amd.martini import MartiniGroup, MartiniHIP
    s = copy.copy(s)
    s.npt_beta = units_convert(3.0e-6, "1/bar")
    c = MartiniGroup(s, grid) if grid else MartiniHIP(s)
    c.eval_forces()
    c.step(20)
    first = c.ranks[0] if grid else c
    out = (first.box().copy(), first.barostat_pressure().copy(), gathered(s, c)["r"] if grid else state(c)["r"])
    c.close()
    return out


@pytest.mark.parametrize("grid", [None, (2, 2, 2)], ids=["one_domain", "2x2x2"])
def test_barostat_runs_repeat_bit_for_bit(grid):
    """two fresh contexts, 20 barostat steps: the box, the pressure and every position identical in every bit"""
    s = C.system("molecules", 600) if grid is None else C.system("molecules_split", grid)
    a, b = _run20(s, grid), _run20(s, grid)
    assert (np.abs(a[0] / C.box_of(s) - 1) > 1e-6).all(), a[0] / C.box_of(s)
    for x, y, what in zip(a, b, ("box", "pressure", "positions")):
        assert np.array_equal(x, y), (what, np.abs(np.asarray(x) - np.asarray(y)).max())

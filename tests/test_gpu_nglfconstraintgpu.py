"""GPU tests (-m gpu) of the NGLFCONSTRAINTGPU family at the library level: MartiniHIP built from a Setup of such a type composes constraint
groups, the groups' override (every bead LANGEVIN on the particles' LCG64 streams with group 0's parameters, or every bead FREE) and the
barostat on the molecular pressure, semi-isotropic and isotropic, and follows the oracle (tests/nglfconstraintgpu_systems.ComposedOracle,
held to Oracle.step_npt bit for bit on the CPU) over 25 steps with a rebuild every 10.

Tolerances are those test_gpu_parity.py applies to the same quantities of NGLFCONSTRAINT runs (test_velocity_constraints_match_oracle,
test_barostat_with_molecular_virial_and_constraints; neither scales with the step count): positions 1e-7 of the box side, velocities 1e-6
of the largest component, the box 1e-10.  The LCG64 states are integers and must be equal."""
import numpy as np
import pytest

import constraint_systems as C
import nglfconstraintgpu_systems as N

pytestmark = pytest.mark.gpu
NSTEPS = 25


@pytest.mark.parametrize("name,isotropic", [("NGLFCONSTRAINTGPULANGEVIN", 0), ("NGLFCONSTRAINTGPULANGEVINLCG64", 1), ("NGLFCONSTRAINTGPU", 1)])
def test_25_steps_follow_the_oracle(name, isotropic):
    from ddcmd_amd.martini import MartiniHIP
    s = N.lipid(name, isotropic)                  # group 0 LANGEVIN, group 1 (every other bead) BERENDSEN: both overridden by the type
    langevin = "LANGEVIN" in name
    m = MartiniHIP(s)                             # constraints, barostat, groups: from the Setup's INTEGRATOR type alone
    assert m.plan["constraints"] and m.plan["isotropic"] == bool(isotropic) and list(m.plan["group_type"]) == ([2, 2] if langevin else [0, 0])
    ref = N.ComposedOracle(N.as_run(s))
    o = ref.o
    m.eval_forces()
    lcg0 = s.lcg64.copy()
    for n in (1, 9, 15):                          # rebuilds at loops 10 and 20 fall inside
        m.step(n)
    ref.step(NSTEPS)
    st = m.download()
    box, L0 = m.box(), s.box
    print("%s isotropic %d: box %s (oracle %s)" % (name, isotropic, box / L0, o.box / L0))
    assert np.abs(box - o.box).max() < 1e-10 * o.box.max()
    assert np.abs(box / L0 - 1).max() > 1e-5
    if isotropic:
        assert np.abs(box / L0 - (box / L0)[0]).max() < 1e-14
    else:
        assert abs(box[0] / L0[0] - box[1] / L0[1]) < 1e-14 and abs(box[2] / L0[2] - box[0] / L0[0]) > 1e-9
    for c, (ro, vo) in enumerate(((o.rx, o.vx), (o.ry, o.vy), (o.rz, o.vz))):
        dr = st["r"][c] - ro
        dr -= box[c] * np.rint(dr / box[c])
        dv = np.abs(st["v"][c] - vo).max()
        print("  axis %d: |r - r_oracle| %.3e of the box side (bound 1e-7), |v - v_oracle| %.3e of max |v| (bound 1e-6)" %
              (c, np.abs(dr).max() / box[c], dv / np.abs(vo).max()))
        assert np.abs(dr).max() < 1e-7 * box[c], c
        assert dv < 1e-6 * np.abs(vo).max(), c
    if langevin:
        lcg = m.get_random_lcg64()
        assert np.array_equal(lcg["state"], o.lcg["state"]) and np.array_equal(lcg["multID"], o.lcg["multID"]) and np.array_equal(lcg["prime"], o.lcg["prime"])
        assert (lcg["state"] != lcg0["state"]).all()
    else:
        assert not getattr(m, "_lcg_set", False)                    # every bead FREE: no stream is handed over, none is drawn from
    most, bad = m.constraint_stats()
    want = max(max(f, b) for f, b in ref.sweeps)
    print("  sweeps %d (oracle %d), unconverged %d" % (most, want, bad))
    assert bad == 0 and most == want
    po, pi, pj, dd = m._cons
    d = np.stack([st["r"][c][pi] - st["r"][c][pj] for c in range(3)], axis=1)
    d -= box * np.rint(d / box)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) / dd - 1.0).max() < 1e-10
    assert m.list_stats()["rebuilds"] >= 3
    m.close()


@pytest.mark.parametrize("ratio", [None, 4], ids=["equal", "1to4"])
def test_a_solve_keeps_every_groups_momentum(ratio):
    """the force-free gas under NGLFCONSTRAINTGPU (its BERENDSEN group runs as FREE: nothing but the two solves of a step changes a
    velocity): every group's momentum after a step is its momentum before, within test_gpu_constraints.hold's bound -- two roundings of the
    size of a bead's momentum per pair update and bead -- for groups of one mass and of masses 1 : 4.  The solver weights a pair's impulse
    by 1 / mass (resMoveConsOld, nglfconstraint.c:198); weighting by the mass, as the reference's GPU kernel does, fails this at 1 : 4."""
    from ddcmd_amd.martini import MartiniHIP
    s, t = N.gas(ratio)
    m = MartiniHIP(s, constraint_groups=t)
    assert list(m.plan["group_type"]) == [0] and m.plan["overridden"] == [0]
    m.eval_forces()
    m.step(1)
    st = m.download()
    v = np.stack(st["v"], 1)
    most, bad = m.constraint_stats()
    ref = C.step(s, t, 1)
    assert bad == 0 and abs(most - ref[3]) <= 1
    assert np.abs(v - ref[1]).max() <= C.FACTOR * C.VEL_MEASURED
    p0, p1 = C.group_momenta(s, C.velocities(s)), C.group_momenta(s, v)
    mass = C.masses(s)
    worst = 0.0
    for g, idx in enumerate(s.groups):
        bound = 4 * C.U * (2 * most + 2) * len(idx) * np.abs(mass[idx, None] * v[idx]).max()
        worst = max(worst, float(np.abs(p1[g] - p0[g]).max() / bound))
        assert (np.abs(p1[g] - p0[g]) <= bound).all(), (g, p1[g] - p0[g], bound)
    assert np.abs(v - C.velocities(s)).max() > 1e-3 * np.abs(v).max()          # the solves did change velocities
    print("gas %s: %d sweeps, largest momentum change %.3f of the bound" % (s.name, most, worst))
    m.close()

"""tests/nglfconstraintgpu_systems.py held to the oracle on the CPU: ComposedOracle -- the reference the GPU tests read sweep counts from --
takes Oracle.step_npt's trajectory bit for bit, Langevin streams included, across a list rebuild."""
import numpy as np
import pytest

import nglfconstraintgpu_systems as N
import pyoracle


@pytest.mark.parametrize("name,isotropic", [("NGLFCONSTRAINTGPULANGEVIN", 1), ("NGLFCONSTRAINTGPU", 0)])
def test_the_composed_step_is_the_oracles(name, isotropic):
    s = N.as_run(N.lipid(name, isotropic))
    assert set(s.group_type) == ({2} if "LANGEVIN" in name else {0}) and s.npt_isotropic == isotropic
    c = N.ComposedOracle(s)
    o = pyoracle.Oracle(s, constraints=True)
    o.forces()
    lcg0 = None if o.lcg is None else o.lcg.copy()
    c.step(11)
    e, vir, rk, tion = o.step_npt(11, s.npt_T, s.npt_P0, s.npt_beta, s.npt_tau, molecular=True)
    assert o.loop.value == c.o.loop.value == s.loop + 11 and o.time.value == c.o.time.value
    for k in ("rx", "ry", "rz", "vx", "vy", "vz", "fx", "fy", "fz", "box", "virial", "pmol"):
        assert np.array_equal(getattr(o, k), getattr(c.o, k)), k
    assert rk == c.o.rk.value and np.array_equal(tion, c.o.tion)
    if "LANGEVIN" in name:
        assert np.array_equal(o.lcg, c.o.lcg) and (o.lcg["state"] != lcg0["state"]).all()
    else:
        assert o.lcg is None
    assert len(c.sweeps) == 11 and all(1 < f < 500 and 1 <= b < 500 for f, b in c.sweeps)
    assert np.abs(o.box / s.box - 1).max() > 1e-6                # the barostat moved the box


def test_the_gas_has_the_masses_it_names():
    import constraint_systems as C
    for ratio in (None, 4):
        s, t = N.gas(ratio)
        m = C.masses(s)
        per_group = [sorted(set(np.round(m[g] / m.min()).astype(int))) for g in s.groups]      # (the lightest free bead: 18 M_p)
        assert all(p == ([1, 4] if ratio else [4]) for p in per_group), per_group[:3]
        assert s.natoms == 20 * 18 + 20 * 4 + 300 and len(t[0]) - 1 == 40

"""The numpy reference of tests/integrator_reference.py held against the oracle's C restatement, on the cases of
tests/test_gpu_integrator_groups.py and at the oracle's forces: the reference is known to be right before a device is asked.
Needs no GPU.  Two restatements written apart from the same formulas agree to rounding: the gates are those of the device tests."""
import numpy as np
import pytest

import pyoracle
import integrator_reference as ir

CASES = [("all-32", n) for n in ir.SIZES] + [(t, n) for t in ("mixed", "holes", "free+equal-berendsen", "free") for n in ir.TABLE_SIZES]
BATCHES = {"single": [1] * 6, "k2": [2, 2, 2], "k5": [5, 3]}


def _forces(o):
    return np.stack([o.fx, o.fy, o.fz]).copy()


def drive_oracle(s, sizes):
    """steps in batches of `sizes`, the group temperatures published between batches only; every step is compared"""
    o = pyoracle.Oracle(s)
    o.forces()
    o.group_temperature()
    ref = ir.NGLFReference(s, lcg=s.lcg64)
    ref.publish()
    what = "%d beads" % s.natoms
    for k in sizes:
        for _ in range(k):
            ref.front(_forces(o))
            _, _, rk, tion = o.step(1)
            ref.back(_forces(o))
            ir.compare(ref, s, np.stack([o.rx, o.ry, o.rz]), np.stack([o.vx, o.vy, o.vz]), rk, tion, None, None, None, what=what)
        o.group_temperature()
        ref.publish()
        T = np.array([o.groups[g].temperature for g in range(s.ngroup)])
        ir.compare(ref, s, np.stack([o.rx, o.ry, o.rz]), np.stack([o.vx, o.vy, o.vz]), None, None, T, o.kinetic_detail(0), o.kinetic_detail(1), what=what)
    assert o.loop.value == ref.loop == s.loop + sum(sizes)
    if s.lcg64 is not None:
        assert np.array_equal(o.lcg["state"], ref.lcg["state"]) and not np.array_equal(ref.lcg["state"], s.lcg64["state"])
    return o, ref


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("interacting", [False, True], ids=["force-free", "interacting"])
@pytest.mark.parametrize("table,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_reference_equals_oracle(table, n, interacting, batch):
    drive_oracle(ir.make_system(n, table, interacting), BATCHES[batch])


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("interacting", [False, True], ids=["force-free", "interacting"])
def test_reference_equals_oracle_on_lcg64_streams(interacting, batch):
    drive_oracle(ir.make_system(257, "mixed", interacting, lcg=True), BATCHES[batch])


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_reference_equals_oracle_from_loop_7(batch):
    """loop % interval out of phase with a fresh start: the interval-3 group scales after steps 2 and 5, not 3 and 6"""
    o, ref = drive_oracle(ir.make_system(65, "mixed", False, loop=7), BATCHES[batch])
    assert ref.loop == 7 + sum(BATCHES[batch])


def test_the_reference_thermostats_act():
    """the cases are not trivially passed: over 6 steps BERENDSEN groups change their temperature, LANGEVIN groups draw noise, the
    tau = 0 group runs through its cycle, FREE beads fly straight"""
    s = ir.make_system(1025, "mixed", False)
    ref = ir.NGLFReference(s)
    T0 = ref.publish()
    v0 = ref.v.copy()
    f = np.zeros((3, s.natoms))
    for _ in range(6):
        ref.front(f)
        ref.back(f)
        ref.publish()
    assert np.array_equal(ref.v[:, s.group == 0], v0[:, s.group == 0])
    assert ref.T[1] > 1.005 * T0[1] and ref.T[2] > 1.005 * T0[2]
    # tau = 0 with the lag of the published temperature: T_{k+1} = T_k Teq / T_{k-1}, a cycle of period 6 through T0, T0, Teq, Teq^2/T0, ...
    assert abs(ref.T[5] - T0[5]) < 1e-12 * T0[5] and abs(T0[5] - s.group_Teq[5]) > 0.1 * T0[5]
    for g in (3, 4):
        assert np.abs(ref.v[:, s.group == g] - v0[:, s.group == g]).min() > 0.0
    # the group with a drift velocity is pulled towards it: mean (v - v0) along vcm is positive
    dv = (ref.v - v0)[:, s.group == 4].mean(axis=1)
    assert np.dot(dv, s.group_vcm[4]) > 0.0


def test_counter_normals_are_unit_normals():
    g = ir.counter_normals(12345, np.arange(200000, dtype=np.uint64) << np.uint64(32), 6)
    assert np.abs(g.mean(axis=1)).max() < 0.01 and np.abs(g.var(axis=1) - 1.0).max() < 0.02
    assert abs(np.mean(g[0] * g[1])) < 0.01 and abs(np.mean(g[0] * g[2])) < 0.01
    assert not np.array_equal(g, ir.counter_normals(12345, np.arange(200000, dtype=np.uint64) << np.uint64(32), 7))

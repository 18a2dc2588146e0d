"""CPU tests (-m "not gpu") that the systems of tests/approach_systems.py ARE adversarial for the shell-limited walk: conditions on the
inputs, held along the oracle's trajectory -- tests/test_gpu_shell_walk.py is worth what these hold."""
import os
import re

import numpy as np
import pytest

import approach_systems as A
from approach_systems import ANG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "ddcmd_amd", "csrc", "hip")
CASES = [("one_type", {}), ("types20", {}), ("charged", {}), ("one_type", dict(update_rate=40, step_A=0.05)), ("one_type", dict(grid=(2, 2, 2)))]
IDS = ["one_type", "types20", "charged", "period40", "grid222"]
# the first steps at which shells 3..7 are walked again, by hand for 12 / 4 A: the smallest n with 2 n step_A >= sh_reach[s]
FIRST_STEPS = {0.1: (4, 7, 11, 14, 17), 0.05: (7, 14, 21, 28, 34)}
_traj = {}


def run(case):
    variant, kw = case
    key = (variant, tuple(sorted(kw.items())))
    if key not in _traj:
        s = A.system(variant, **kw)
        n = int(s.updateRate) + 5
        R, V = A.oracle_trajectory(s, n)
        _traj[key] = (s, R, V, A.schedule(s, n, R))
    return _traj[key]


def test_restated_constants_are_the_code_s():
    """the constants of approach_systems are read out of the sources where the module says they stand (the numbers alone: a reformatted
    line still matches), and the shell edges they give for 12 / 4 A are the ones worked out by hand: r0 = 11 A, steps of
    (256 - 121) / 6.99 A^2 in r^2"""
    src = {f: open(os.path.join(HIP, f)).read() for f in ("ddcmi_rebuild.inl", "ddcmi_listbuild.inl", "ddcmi_step.inl", "ddcmi_nonbond.inl", "ddcmi_internal.h")}
    num = r"([0-9.]+(?:e-?[0-9]+)?)f?"
    found = (int(re.search(r"#\s*define\s+NSHELL\s+(\d+)", src["ddcmi_listbuild.inl"]).group(1)),
             float(re.search(r"sh_step\s*=[^;]*NSHELL\s*-\s*" + num, src["ddcmi_rebuild.inl"]).group(1)),
             float(re.search(r"r0\s*=\s*rcut\s*-\s*" + num + r"\s*\*\s*dR", src["ddcmi_rebuild.inl"]).group(1)),
             float(re.search(r"sh_reach\[sq\]\s*=[^;]*\(\s*1\.0\s*-\s*" + num + r"\s*\)\s*-\s*ctx->rmax", src["ddcmi_step.inl"]).group(1)),
             int(re.search(r"#\s*define\s+LEAN_W\s+(\d+)", src["ddcmi_internal.h"]).group(1)),
             float(re.search(r"#\s*define\s+LEAN_C\s+" + num, src["ddcmi_nonbond.inl"]).group(1)))
    assert found == (A.NSHELL, A.SHELL_FRACTION, A.R0_SKIN_FRACTION, A.REACH_MARGIN, A.LEAN_W, A.LEAN_C), found
    assert re.search(r"sh_reach\[s_\]\s*>\s*twoD\s*\)\s*smax\s*=\s*s_\s*-\s*1", src["ddcmi_nonbond.inl"])
    by_hand = [np.sqrt(121.0 + (sq - 1) * 135.0 / 6.99) * (1.0 - 1e-4) - 12.0 for sq in range(1, 8)]
    reach = A.shell_reach(12.0 * ANG, 4.0 * ANG)[1:] / ANG
    assert np.abs(reach - np.array(by_hand)).max() < 1e-6, reach.tolist()          # (r0^2 is kept as a float: 3e-8 A)
    assert np.abs(reach - np.array(A.SH_REACH_12_4_A)).max() < 2e-9, reach.tolist()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_isolation(case):
    """no bead other than its partner comes within list radius + skin of a probe bead at any step; at most 2000 beads"""
    s, R, V, sch = run(case)
    assert s.natoms <= 2000
    partner = np.full(s.natoms, -1)
    partner[s.pair_i], partner[s.pair_j] = s.pair_j, s.pair_i
    box = A.box_of(s)
    probes = np.flatnonzero(s.probe)
    lim = s.rmax + 2.0 * s.deltaR
    for n in range(len(R)):
        d = A.min_image(R[n][probes, None, :] - R[n][None, :, :], box)
        d2 = (d * d).sum(axis=2)
        d2[np.arange(probes.size), probes] = np.inf
        d2[np.arange(probes.size), partner[probes]] = np.inf
        assert d2.min() > lim * lim, (n, np.sqrt(d2.min()) / ANG)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_shells_are_occupied_and_every_pair_crosses(case):
    """every shell 2..7 holds at least 4 probe pairs at the rebuild; every probe pair with d0 < rcut + 2 step_A updateRate - 0.05 A is
    inside the cut-off at some step of the period, with a non-zero reference force there; no pair is ever within 1e-3 A of the
    cut-off at a step (so that double and longdouble agree on who is inside); pairs straddle the faces they are meant to"""
    s, R, V, sch = run(case)
    ur = int(s.updateRate)
    moving = s.pair_kind != "rest"
    edges = A.shell_edges(s.rmax, s.deltaR)
    shell0 = np.searchsorted(edges[1:], sch[0]["dist"], side="right")
    assert np.bincount(shell0[moving], minlength=8)[2:].min() >= 4
    assert min(np.abs(e["dist"] - s.rmax).min() for e in sch) > 1e-3 * ANG
    crossing = np.flatnonzero(moving & (s.pair_d0 < 12.0 + 2.0 * s.step_A * ur - 0.05))
    assert crossing.size >= 70
    first = {}
    for n in range(1, ur + 1):
        for q in sch[n]["inside"]:
            first.setdefault(q, n)
    assert set(crossing.tolist()) <= set(first)
    for n in sorted(set(first[q] for q in crossing)):
        f = A.reference_forces(s, R[n])
        for q in crossing:
            if first[q] == n:
                assert np.abs(f[s.pair_i[q]]).max() > 0 and np.abs(f[s.pair_j[q]]).max() > 0, (n, q)
    # resting pairs never cross, their beads never feel a force
    assert all(not (e["dist"][~moving] < s.rmax).any() for e in sch)
    # face pairs: the partners are on opposite sides of the box; domain pairs: in different domains
    box = A.box_of(s)
    r0 = R[0]
    for q in np.flatnonzero(s.pair_kind == "face"):
        d = r0[s.pair_i[q]] - r0[s.pair_j[q]]
        assert (np.abs(d) > 0.5 * box).sum() == 1
    assert (s.pair_kind == "face").sum() == 3
    if case[1].get("grid"):
        from ddcmd_amd.martini import domain_of
        owner = domain_of(s, case[1]["grid"])
        dom = np.flatnonzero(s.pair_kind == "domain")
        assert dom.size == 3 and all(owner[s.pair_i[q]] != owner[s.pair_j[q]] for q in dom)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_first_step_and_stop_conditions(case):
    """for every shell s = 3..7 the pair at b_s (1 + 3e-5) is OUTSIDE the cut-off until the last step before the schedule walks shell s
    again (the stop is exercised: a walk that never stops early is not what passes) and INSIDE at that first step (a walk that
    re-admits the shell one step late loses a force); the steps are the ones worked out by hand, 4 7 11 14 17 at 0.1 A per step; the
    schedule does not depend on the code's round-up factors; the pair at b_s (1 - 3e-5) belongs to shell s - 1 for the walk
    (margin 1e-4) and is inside at that step too"""
    s, R, V, sch = run(case)
    ur = int(s.updateRate)
    assert all(e["smax"] == e["smax_hi"] for e in sch)
    assert sch[0]["smax"] == 2 and sch[ur]["smax"] == 2 and sch[ur - 1]["smax"] == 7
    firsts = []
    for sh in range(3, A.NSHELL):
        n1 = min(n for n in range(1, ur) if sch[n]["smax"] >= sh)
        firsts.append(n1)
        plus = [q for q in np.flatnonzero(s.pair_kind == "edge+") if s.pair_shell[q] == sh]
        minus = [q for q in np.flatnonzero(s.pair_kind == "edge-") if s.pair_shell[q] == sh]
        assert len(plus) == 1 and len(minus) == 1
        q = plus[0]
        assert q in sch[n1]["inside"], (sh, n1, sch[n1]["dist"][q] / ANG)
        assert all(q not in sch[n]["inside"] for n in range(n1)), sh
        assert sch[n1 - 1]["smax"] == sh - 1
        assert minus[0] in sch[n1]["inside"]
    assert tuple(firsts) == FIRST_STEPS[s.step_A], firsts
    # a whole family of sweep pairs crosses while its shell is not walked yet only if the bound were loose: none does
    edges = A.shell_edges(s.rmax, s.deltaR)
    shell0 = np.searchsorted(edges[1:], sch[0]["dist"], side="right")
    for n in range(1, ur):
        assert all(shell0[q] <= sch[n]["smax"] for q in sch[n]["inside"]), n


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_speeds_stay_near_vmax(case):
    """the oracle's largest speed over the period stays within a few per cent of vmax, so the bound stays tight: largest ratios
    one_type / types20 1.0195, charged 1.0003 (like charges: the partners slow each other down).  period40 reaches 1.0798, a
    deliberate deviation from "a few per cent": the system is the issue's collider("one_type", update_rate=40, step_A=0.05) as it
    states it -- half the speed and twice the steps inside the cut-off's attraction -- and is bounded at 9 % here; its re-admission
    steps are still the tight ones (7 14 21 28 34, test_first_step_and_stop_conditions), and the GPU test measures tightness
    against the oracle's own sum dt max |v|, not against n step_A"""
    s, R, V, sch = run(case)
    ur = int(s.updateRate)
    speed = np.sqrt((V[:ur + 1] ** 2).sum(axis=2)).max(axis=1) / s.vmax
    print(case, "largest speed / vmax over the period: %.4f" % speed.max())
    assert speed.min() >= 1.0 - 1e-12
    assert speed.max() < (1.09 if s.step_A < 0.1 else 1.03)
    # until the first pair is inside the cut-off nobody feels a force: the bound is EXACTLY n step_A
    assert abs(sch[1]["D"] - s.step_A * ANG) < 1e-12 * ANG


def test_lean_step_count_of_the_call_patterns():
    assert A.lean_steps_after((25,), 20) == [5]
    assert A.lean_steps_after((1,) * 25, 20) == [0] * 25
    assert A.lean_steps_after((3, 4, 4, 3, 3, 8), 20) == [2, 5, 8, 10, 12, 5]
    assert A.lean_steps_after((45,), 40) == [5] and A.lean_steps_after((33, 12), 40) == [32, 5] and A.lean_steps_after((35,), 40) == [32]


def test_projectile():
    s = A.projectile()
    assert s.natoms == 6912
    v = np.sqrt(s.vx ** 2 + s.vy ** 2 + s.vz ** 2)
    k = s.fast_bead
    assert 0.95 * 0.5 * s.deltaR < s.dt * v[k] * s.updateRate < 0.5 * s.deltaR
    assert np.delete(v, k).max() < 0.2 * v[k]


def test_one_sided_movers_and_a_resting_rank():
    """one_sided(): every mover is on rank 0 of 2 x 1 x 1 at every step and stays there, rank 1's own bound walks shell 2 only through the
    whole period (2 D of its beads < sh_reach[3]), yet cross pairs of shells 3 and 4 are inside the cut-off before the rebuild, with
    a reference force on the resting partner; nobody is within list radius + skin of a y or z face (no rank holds images of its own
    beads); probe beads meet nobody but their partners"""
    from ddcmd_amd.martini import domain_of
    import copy
    s = A.one_sided()
    ur = int(s.updateRate)
    R, V = A.oracle_trajectory(s, ur + 5)
    sch = A.schedule(s, ur + 5, R)
    box = A.box_of(s)
    lim = s.rmax + 2.0 * s.deltaR
    owner0 = domain_of(s, s.grid)
    reach = A.shell_reach(s.rmax, s.deltaR)
    D1 = 0.0
    partner = np.full(s.natoms, -1)
    partner[s.pair_i], partner[s.pair_j] = s.pair_j, s.pair_i
    for n in range(len(R)):
        sn = copy.copy(s)
        sn.rx, sn.ry, sn.rz = R[n][:, 0].copy(), R[n][:, 1].copy(), R[n][:, 2].copy()
        assert np.array_equal(domain_of(sn, s.grid), owner0), n
        assert (np.abs(R[n][:, 1:]) < 0.5 * box[1:] - lim).all(), n
        d = A.min_image(R[n][:, None, :] - R[n][None, :, :], box)
        d2 = (d * d).sum(axis=2)
        d2[np.arange(s.natoms), np.arange(s.natoms)] = np.inf
        d2[np.arange(s.natoms), partner] = np.inf
        assert d2.min() > lim * lim, n
        if 0 < n < ur:
            dr = A.min_image(R[n] - R[n - 1], box)[owner0 == 1]
            D1 += np.sqrt((dr * dr).sum(axis=1)).max()
            assert A.smax_of(reach, D1 * (1.0 + A.ROUND_UP)) == 2, n
    speed0 = np.sqrt((V[0] ** 2).sum(axis=1))
    assert (speed0[owner0 == 1] == 0).all() and (speed0[s.probe & (owner0 == 0)] > 0.999 * s.vmax).all()
    cross = np.flatnonzero(s.pair_kind == "cross")
    assert all(owner0[s.pair_i[q]] == 0 and owner0[s.pair_j[q]] == 1 for q in cross)
    late = [q for q in cross if s.pair_shell[q] >= 3]
    assert len(late) == 10 and sorted(set(s.pair_shell[late].tolist())) == [3, 4]
    assert min(np.abs(e["dist"] - s.rmax).min() for e in sch) > 1e-3 * ANG
    f = A.reference_forces(s, R[ur - 1])
    for q in late:
        assert q in sch[ur - 1]["inside"] and q not in sch[3]["inside"] and np.abs(f[s.pair_j[q]]).max() > 0, q

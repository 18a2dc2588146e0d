"""GPU tests (-m gpu) of the list build's exclusion logic on the adversarial molecular systems of tests/molecule_systems.py:
large molecules, several groups per molecule (atom codes up to 0xffff), sparse 32-bit molecule ids that collide in the build's
compressed forms, more excluded partners per bead than the rows the build starts with.  Every case is built so that a wrong
decision changes the pair sets: lists are compared as exact sets over ALL beads with the oracle's, forces / energies / virial
with the oracle and with the brute-force longdouble reference of the same module.  Tolerances are those of
tests/test_gpu_parity.py.  docs/molecule_exclusion_variants.md records six one-line mutations of the kernels and which of these
tests each turns red."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle
from conftest import rel_force_err
from molecule_systems import make_molecule_setup, counts, system, reference, oracle_list, VARIANTS
from molecule_worker import run_single, run_group

pytestmark = pytest.mark.gpu
TOL = 1e-6          # energies along a trajectory (tests/test_gpu_parity.py)
TIGHT = 1e-10       # step-0 forces, energies, virial
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, 1, 2), (2, 2, 1), (2, 2, 2)]


def device_list(m, which):
    start, j = m.get_list(which)
    i = np.repeat(np.arange(m.n), np.diff(start))
    return set(zip(i.tolist(), j.tolist()))


def check_step0(s, variant, f, e, vir, tag):
    """forces, lj, ele, virial against the oracle and against the brute-force reference; then the beads of types B-E alone,
    normalised by the largest force among them, so that water (and the control type A) cannot mask them"""
    _, o, _, eo, viro = system(variant)
    rf, rlj, rele, rvir, _, _ = reference(variant)
    refs = (("oracle", (o.fx, o.fy, o.fz), eo["lj"], eo["ele"], viro),
            ("brute force", tuple(np.asarray(c, np.float64) for c in rf), float(rlj), float(rele), np.asarray(rvir, np.float64)))
    mol = np.flatnonzero(np.isin(s.mol_kind, list("BCDE")))
    for name, g, glj, gele, gvir in refs:
        err = rel_force_err(f, g)
        err_mol = rel_force_err([np.asarray(c)[mol] for c in f], [np.asarray(c)[mol] for c in g])
        print("%s %s vs %s: forces %.2e types B-E %.2e lj %.2e ele %.2e virial %.2e" % (
            variant, tag, name, err, err_mol, abs(e["lj"] - glj) / abs(glj), abs(e["ele"] - gele) / abs(gele), np.abs(vir - gvir).max() / np.abs(gvir).max()))
        assert err < TIGHT, (tag, name, err)
        assert err_mol < TIGHT, (tag, name, err_mol)
        assert abs(e["lj"] - glj) < TIGHT * abs(glj), (tag, name)
        assert abs(e["ele"] - gele) < TIGHT * abs(gele), (tag, name)
        assert np.abs(vir - gvir).max() < TIGHT * np.abs(gvir).max(), (tag, name)


@pytest.mark.parametrize("variant", VARIANTS)
def test_lists_forces_and_energies_at_step_0(variant, monkeypatch, capfd):
    """kept and excluded lists equal the oracle's as sets of pairs; the counts; forces, energies and virial; the rows of the
    excluded list were grown once, to the largest count + 4 (the build's report under DDCMI_DEBUG_SCHED)"""
    from ddcmd_amd.martini import MartiniHIP
    s, o, npairs, eo, viro = system(variant)
    monkeypatch.setenv("DDCMI_DEBUG_SCHED", "1")
    m = MartiniHIP(s)
    e, vir = m.eval_forces()
    monkeypatch.delenv("DDCMI_DEBUG_SCHED")
    report = [l for l in capfd.readouterr().err.splitlines() if l.startswith("ddcmi build:")]
    assert device_list(m, 0) == oracle_list(o, 0)
    assert device_list(m, 1) == oracle_list(o, 1)
    st = m.list_stats()
    assert st["entries"] == 2 * npairs[0] and st["excluded"] == 2 * npairs[1]
    check_step0(s, variant, m.download()["f"], e, vir, "one domain")
    assert len(report) == 1, report
    words = report[0].split()
    assert int(words[words.index("maxexcl") + 1]) == counts(variant)["max_excluded"] + 4, report
    m.close()


def build_attempts(err):
    """launches of the list build a context made, from its DDCMI_DEBUG_PHASES report at ddcmi_destroy (`ddcmi phase 11 build+transpose
    launched ... x <count>`: one count per attempt, a build that is started over after growing a buffer counts again) and the
    builds that were completed (phase 13)"""
    out = {}
    for line in err.splitlines():
        w = line.split()
        if line.startswith("ddcmi phase") and int(w[2]) in (11, 13):
            out[int(w[2])] = int(w[-1])
    return out[11], out[13]


@pytest.mark.parametrize("variant", VARIANTS)
def test_45_steps_across_two_rebuilds(variant, monkeypatch, capfd):
    """the oracle steps the same system: energies, kinetic energy and virial after every step; after the second rebuild the
    lists are the oracle's again.  The rows of the excluded list are grown once and stay grown: a context that only evaluates
    step 0 launches the build more than once (16 rows are too few for the hubs), and the 45 steps with their two rebuilds add
    exactly two launches to that -- no rebuild was started over"""
    from ddcmd_amd.martini import MartiniHIP
    s = make_molecule_setup(variant)
    monkeypatch.setenv("DDCMI_DEBUG_PHASES", "1")
    m0 = MartiniHIP(s)
    m0.eval_forces()
    capfd.readouterr()
    m0.close()
    first = build_attempts(capfd.readouterr().err)
    o = pyoracle.Oracle(s)
    o.forces()
    m = MartiniHIP(s)
    m.eval_forces()
    monkeypatch.delenv("DDCMI_DEBUG_PHASES")      # (a context reads it at its first build)
    for step in range(45):
        eo, vo, rko, _ = o.step(1)
        m.step(1)
        e, vir, rk, _ = m.energies()
        for k in ("lj", "ele", "total"):
            assert abs(e[k] - eo[k]) < TOL * abs(eo[k]), (step, k)
        assert abs(rk - rko) < TOL * rko, step
        assert np.abs(vir - vo).max() < TOL * np.abs(vo).max(), step
    st = m.list_stats()
    assert st["rebuilds"] == 3
    assert device_list(m, 0) == oracle_list(o, 0)
    assert device_list(m, 1) == oracle_list(o, 1)
    assert st["excluded"] == 2 * o.L.orc_nbr_npairs(o.nbr, 1) and st["entries"] == 2 * o.L.orc_nbr_npairs(o.nbr, 0)
    d = m.download()
    assert rel_force_err(d["f"], (o.fx, o.fy, o.fz)) < TOL
    capfd.readouterr()
    m.close()
    after = build_attempts(capfd.readouterr().err)
    print(variant, "build launches (attempts, completed): step 0", first, "after 45 steps", after)
    assert first[1] == 1 and first[0] >= 2
    assert after[1] == 3 and after[0] == first[0] + 2


def child(variant, mode, out, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "molecule_worker.py"), variant, mode, out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0 and "molecule_worker ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return dict(np.load(out))


@pytest.mark.parametrize("variant", VARIANTS)
def test_split_step_and_two_level_pair_table_equal_the_default(variant, monkeypatch, tmp_path):
    """the excluded walk exists in every instantiation of k_nonbond<true, ...>: the two-level pair table (DDCMI_FORCE_LEVEL_TABLE=1)
    and the split step (DDCMI_NO_FUSED_STEP=1, read once per process: a child process) give the default's step 0 and its
    state after 45 steps bit for bit"""
    for k in ("DDCMI_FORCE_LEVEL_TABLE", "DDCMI_NO_FUSED_STEP"):
        assert not os.environ.get(k), "%s is set in this environment: there is no default run to compare with" % k
    s = make_molecule_setup(variant)
    base = run_single(s)
    assert base["stats"][2] == 3
    monkeypatch.setenv("DDCMI_FORCE_LEVEL_TABLE", "1")
    lvl = run_single(s)
    monkeypatch.delenv("DDCMI_FORCE_LEVEL_TABLE")
    split = child(variant, "single", str(tmp_path / "split.npz"), {"DDCMI_NO_FUSED_STEP": "1"})
    for name, other in (("level table", lvl), ("split step", split)):
        for k in sorted(base):
            assert np.array_equal(np.asarray(base[k]), np.asarray(other[k])), (name, k)


def check_group(s, variant, res, o45, tag):
    """a decomposed run's step 0 (summed energies / virial, gathered forces) and its state after 45 steps against the oracle"""
    by_gid = np.argsort(np.asarray(s.gid, np.uint64), kind="stable")
    assert np.array_equal(res["gid"], np.asarray(s.gid, np.uint64)[by_gid])
    inv = np.empty_like(by_gid)
    inv[by_gid] = np.arange(by_gid.size)
    e0 = dict(zip(("lj", "ele", "total"), res["e0"].tolist()))
    check_step0(s, variant, [res["f0"][c][inv] for c in range(3)], e0, res["vir0"], tag)
    eo, vo, rko, (fo, ro, vel) = o45
    for c, k in enumerate(("lj", "ele", "total")):
        assert abs(res["e"][c] - eo[k]) < TOL * abs(eo[k]), (tag, k)
    assert abs(float(res["rk"]) - rko) < TOL * rko and np.abs(res["vir"] - vo).max() < TOL * np.abs(vo).max(), tag
    assert rel_force_err([res["f"][c][inv] for c in range(3)], fo) < TOL, tag
    box = np.array([s.h[0], s.h[4], s.h[8]])
    for c in range(3):
        dr = res["r"][c][inv] - ro[c]
        dr -= box[c] * np.rint(dr / box[c])
        assert np.abs(dr).max() < 1e-8, (tag, c)
        assert np.abs(res["v"][c][inv] - vel[c]).max() < 1e-8 * np.abs(vel[c]).max(), (tag, c)


_o45 = {}


def oracle_after_45_steps(variant):
    if variant not in _o45:
        s = make_molecule_setup(variant)
        o = pyoracle.Oracle(s)
        o.forces()
        eo, vo, rko, _ = o.step(45)
        _o45[variant] = (eo, vo, rko, ((o.fx.copy(), o.fy.copy(), o.fz.copy()), (o.rx.copy(), o.ry.copy(), o.rz.copy()), (o.vx.copy(), o.vy.copy(), o.vz.copy())))
    return _o45[variant]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_decomposed_before_and_after_45_steps(variant, grid):
    """molecules of every type straddle the domain faces: bonded partners coded 255 and more and ids of 2^24 and more are HALO
    beads (the gid read for a halo slot, the tag word carried by the exchange), and they migrate"""
    from ddcmd_amd.martini import domain_of
    import copy
    s = make_molecule_setup(variant)
    o45 = oracle_after_45_steps(variant)
    # conditions on the inputs: types B, C and D have a copy cut by a domain face, and beads change owners within 45 steps
    owner = domain_of(s, grid)
    for kind in "BCD":
        assert any(np.unique(owner[s.copy_of == k]).size > 1 for k in np.unique(s.copy_of[s.mol_kind == kind])), (kind, grid)
    s45 = copy.copy(s)
    s45.rx, s45.ry, s45.rz = o45[3][1]
    assert (domain_of(s45, grid) != owner).sum() > 0
    check_group(s, variant, run_group(s, grid), o45, "%dx%dx%d" % grid)


@pytest.mark.parametrize("mode", ["single", "group222"])
def test_exactly_sized_buffers_with_canaries(mode, tmp_path):
    """DDCMI_DEBUG_GUARD=1 (read once per process: a child process): every device buffer exactly as large as asked for, a
    canary behind it checked when the buffer is grown or released -- the grown rows of the excluded list among them.  The run
    ends without a complaint and computes what the oracle computes"""
    variant = "wide"
    s = make_molecule_setup(variant)
    res = child(variant, mode, str(tmp_path / "guard.npz"), {"DDCMI_DEBUG_GUARD": "1"})
    o45 = oracle_after_45_steps(variant)
    if mode == "group222":
        check_group(s, variant, res, o45, "guard 2x2x2")
        return
    _, o, npairs, eo, viro = system(variant)
    e0 = dict(zip(("lj", "ele", "total"), res["e0"].tolist()))
    check_step0(s, variant, list(res["f0"]), e0, res["vir0"], "guard one domain")
    assert res["stats0"][0] == 2 * npairs[0] and res["stats0"][1] == 2 * npairs[1] and res["stats"][2] == 3
    e45, v45, rk45, (f45, _, _) = o45
    for c, k in enumerate(("lj", "ele", "total")):
        assert abs(res["e"][c] - e45[k]) < TOL * abs(e45[k]), k
    assert abs(float(res["rk"]) - rk45) < TOL * rk45 and rel_force_err(list(res["f"]), f45) < TOL

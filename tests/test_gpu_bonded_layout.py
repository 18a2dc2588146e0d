"""GPU tests (-m gpu) of the bonded kernels' lane layout -- build_rows() and k_bonded_gather<HEAVY, TABL> of
ddcmd_amd/csrc/hip/bonded.hip -- on the adversarial molecule topologies of tests/bonded_systems.py: molecules longer than a wave and
a workgroup, runs that end exactly at a workgroup's last lane and one lane behind it, atoms that are in one launch's list only,
interleaved molecules, a hub, tables on either side of 384 pieces, terms that differ in one parameter.  A lane that reads another bead's
record gives a wrong force, not a crash: every case is compared bead by bead with the longdouble reference of the same module
(no oracle, no device code in it), and the layout census (ddcmi_debug_bonded_layout) shows that the system drives each path.
docs/bonded_layout_variants.md records one-line mutations of the kernels and which of these tests each turns red."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bonded_systems as bs
from bonded_worker import with_terms, census, run_single, run_group, E_KEYS
from conftest import rel_force_err

pytestmark = pytest.mark.gpu
TOL = 1e-6          # along a trajectory (tests/test_gpu_parity.py: test_lipid_deck_20_steps)
TIGHT = 1e-10       # step-0 forces, energies, virial
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("bond", "angle", "tors", "impr")
GRIDS = [(2, 1, 1), (1, 2, 2), (2, 2, 2)]
TABL = {"lds": (1, 1), "light_spills": (0, 1), "heavy_spills": (1, 0), "edge": (1, 1), "edge385": (0, 1), "shuffled": (0, 1), "reversed": (0, 0)}

_ref = {}


def ref0(variant):
    """the reference at step 0, made once per variant and process: (f [3][N] float64, e dict, virial)"""
    if variant not in _ref:
        s, terms, _ = bs.make_bonded_setup(variant)
        f, e, vir = bs.reference(s, terms)
        e = {k: float(v) for k, v in e.items()}
        e["total"] = sum(e[k] for k in KINDS)
        _ref[variant] = (tuple(np.ascontiguousarray(f[:, c], dtype=np.float64) for c in range(3)), e, vir.astype(np.float64))
    return _ref[variant]


def check_against(f, e, vir, ref, tag, terms_atoms=None):
    fr, er, vr = ref
    err = rel_force_err(f, fr)
    print("%s: forces %.2e" % (tag, err), " ".join("%s %.2e" % (k, abs(e[k] - er[k]) / abs(er[k])) for k in KINDS + ("total",)),
          "virial %.2e" % (np.abs(vir - vr).max() / np.abs(vr).max()))
    assert err < TIGHT, (tag, err, int(np.argmax(np.abs(np.asarray(f) - np.asarray(fr)).max(axis=0))))
    for k in KINDS + ("total",):
        assert abs(e[k] - er[k]) < TIGHT * abs(er[k]), (tag, k, e[k], er[k])
    assert np.abs(vir - vr).max() < TIGHT * np.abs(vr).max(), tag


@pytest.mark.parametrize("variant", bs.VARIANTS)
def test_step_0_against_the_reference_and_the_census(variant):
    """(a) forces per bead, energies by kind and the virial against reference(); lj and ele exactly 0; the device's census equals the
    layout restated in Python, has filler lanes and waves of all three classes, and the launches took the instantiations the tables'
    sizes ask for: 384 pieces in LDS, 385 not"""
    from ddcmd_amd.martini import MartiniHIP
    s, terms, _ = bs.make_bonded_setup(variant)
    m = with_terms(terms, lambda: MartiniHIP(s, test_api=True))
    assert census(m)[:, 10].tolist() == [-1, -1]
    e, vir = m.eval_forces()
    f = m.download()["f"]
    cen = census(m)
    m.close()
    assert e["lj"] == 0.0 and e["ele"] == 0.0
    check_against(f, e, vir, ref0(variant), variant)
    lay = bs.layout(terms)
    print(variant, cen.tolist())
    for q in (0, 1):
        assert cen[q, :10].tolist() == [lay[q]["census"][k] for k in bs.CENSUS[:10]], (q, cen[q].tolist(), lay[q]["census"])
    assert cen[0, 1] + cen[1, 1] >= 1 and all(cen[0, k] + cen[1, k] >= 1 for k in (7, 8, 9))
    assert (cen[0, 10], cen[1, 10]) == TABL[variant]
    assert (cen[0, 3] <= 384, cen[1, 3] <= 384) == tuple(bool(x) for x in TABL[variant])
    if variant.startswith("edge"):
        assert cen[0, 3] == (384 if variant == "edge" else 385)


@pytest.mark.parametrize("variant", ["lds", "heavy_spills"])
def test_45_steps_across_two_rebuilds(variant):
    """(b) NGLF with a rebuild every 16 steps -- the cell sort renumbers the slots twice under unchanged lanes -- against velocity Verlet
    in numpy driven by reference(): energies by kind, kinetic energy and virial after every step, positions and velocities at the end;
    then the final forces against reference() at the device's own final positions, which tells a layout error after the re-sort
    from integration drift"""
    from ddcmd_amd.martini import MartiniHIP
    s, terms, _ = bs.make_bonded_setup(variant)
    hist, (r, v, _) = bs.verlet(s, terms, 45)
    m = with_terms(terms, lambda: MartiniHIP(s, test_api=True))
    m.eval_forces()
    for step in range(45):
        m.step(1)
        e, vir, rk, _ = m.energies()
        h = hist[step]
        tot = sum(abs(h[k]) for k in KINDS)
        for k in KINDS:
            assert abs(e[k] - h[k]) < TOL * max(abs(h[k]), tot * 1e-3), (step, k)
        assert abs(rk - h["rk"]) < TOL * h["rk"], step
        assert np.abs(vir - h["vir"]).max() < TOL * np.abs(h["vir"]).max(), step
    assert m.list_stats()["rebuilds"] == 3
    d = m.download()
    m.close()
    box = np.array([s.h[0], s.h[4], s.h[8]])
    for c in range(3):
        dr = d["r"][c] - r[:, c]
        dr -= box[c] * np.rint(dr / box[c])
        assert np.abs(dr).max() < TOL * box[c], c
        assert np.abs(d["v"][c] - v[:, c]).max() < TOL * np.abs(v).max(), c
    fr = bs.reference(s, terms, np.stack(d["r"], axis=1))[0].astype(np.float64)
    err = rel_force_err(d["f"], tuple(fr[:, c] for c in range(3)))
    print(variant, "forces after 45 steps against the reference at the device's positions: %.2e" % err)
    assert err < TIGHT


def child(variant, nonbonded, mode, out, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bonded_worker.py"), variant, "1" if nonbonded else "0", mode, out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "bonded_worker ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return dict(np.load(out)), p.stderr


@pytest.mark.parametrize("variant", ["lds", "light_spills"])
def test_instantiations_bit_for_bit(variant, monkeypatch, tmp_path):
    """(c) with the pair kernel on (every epsilon zero: it adds nothing) the step is fused and lean, the bonded forces go to the record
    array -- the light launch stores, the heavy one adds, so G's heavy-only atoms must start from zero there -- : step 0 against the
    reference, and the state after 45 steps bit for bit with the tables read from memory (DDCMI_NO_BONDED_LDS_TABLES=1, a switch of the
    context), with a reduction per step (DDCMI_NO_LEAN_STEP=1) and with the split step (DDCMI_NO_FUSED_STEP=1: a child process)"""
    for k in ("DDCMI_NO_BONDED_LDS_TABLES", "DDCMI_NO_LEAN_STEP", "DDCMI_NO_FUSED_STEP"):
        assert not os.environ.get(k), "%s is set in this environment: there is no default run to compare with" % k
    s, terms, _ = bs.make_bonded_setup(variant, nonbonded=True)
    base = run_single(s, terms)
    assert base["rebuilds"] == 3 and tuple(base["census"][:, 10]) == TABL[variant]
    e0 = dict(zip(E_KEYS, base["e0"].tolist()))
    assert e0["lj"] == 0.0 and e0["ele"] == 0.0
    check_against(list(base["f0"]), e0, base["vir0"], ref0(variant), variant + " pair kernel on")
    others = {}
    monkeypatch.setenv("DDCMI_NO_BONDED_LDS_TABLES", "1")
    others["tables from memory"] = run_single(s, terms)
    monkeypatch.delenv("DDCMI_NO_BONDED_LDS_TABLES")
    assert tuple(others["tables from memory"]["census"][:, 10]) == (0, 0)
    again = run_single(s, terms)          # (the switch is the context's: the next context has its tables in LDS again)
    assert tuple(again["census"][:, 10]) == TABL[variant]
    monkeypatch.setenv("DDCMI_NO_LEAN_STEP", "1")
    others["reduction per step"] = run_single(s, terms)
    monkeypatch.delenv("DDCMI_NO_LEAN_STEP")
    others["split step"], _ = child(variant, True, "single", str(tmp_path / "split.npz"), {"DDCMI_NO_FUSED_STEP": "1"})
    for name, other in others.items():
        for k in sorted(base):
            if k != "census":
                assert np.array_equal(np.asarray(base[k]), np.asarray(other[k])), (name, k)


@pytest.mark.parametrize("variant", ["shuffled", "reversed"])
def test_other_hand_over_bead_by_bead(variant):
    """(d) the same system in a random caller order and in reversed order with shuffled term lists against the ordered hand-over, bead by
    bead through the permutation; the sums of the energies"""
    from ddcmd_amd.martini import MartiniHIP
    out = {}
    for v in ("lds", variant):
        s, terms, info = bs.make_bonded_setup(v)
        m = with_terms(terms, lambda: MartiniHIP(s))
        e, vir = m.eval_forces()
        out[v] = (m.download()["f"], e, vir, info["perm"])
        m.close()
    (f0, e0, v0, _), (f1, e1, v1, perm) = out["lds"], out[variant]
    err = rel_force_err(f1, tuple(np.asarray(c)[perm] for c in f0))
    print(variant, "against the ordered hand-over: %.2e" % err)
    assert err < TIGHT
    for k in KINDS + ("total",):
        assert abs(e1[k] - e0[k]) < TIGHT * abs(e0[k]), k
    assert np.abs(v1 - v0).max() < TIGHT * np.abs(v0).max()


def test_atoms_named_by_gid_on_one_domain():
    """(e) ddcmi_set_bonded_gid: atoms numbered by the rank of their gid among the term gids"""
    from ddcmd_amd.martini import MartiniHIP
    for variant in ("lds", "shuffled"):
        s, terms, _ = bs.make_bonded_setup(variant)
        m = with_terms(terms, lambda: MartiniHIP(s, bonded_by_gid=True))
        e, vir = m.eval_forces()
        check_against(m.download()["f"], e, vir, ref0(variant), variant + " by gid")
        m.close()


_one = {}


def one_domain_45(variant):
    if variant not in _one:
        s, terms, _ = bs.make_bonded_setup(variant)
        _one[variant] = run_single(s, terms)
    return _one[variant]


def check_group(s, terms, res, variant, tag):
    by_gid = np.argsort(np.asarray(s.gid, np.uint64), kind="stable")
    assert np.array_equal(res["gid"], np.asarray(s.gid, np.uint64)[by_gid])
    inv = np.empty_like(by_gid)
    inv[by_gid] = np.arange(by_gid.size)
    e0 = dict(zip(E_KEYS, res["e0"].tolist()))
    check_against([res["f0"][c][inv] for c in range(3)], e0, res["vir0"], ref0(variant), tag + " step 0")
    r45 = np.stack([res["r"][c][inv] for c in range(3)], axis=1)
    fr = bs.reference(s, terms, r45)[0].astype(np.float64)
    err = rel_force_err([res["f"][c][inv] for c in range(3)], tuple(fr[:, c] for c in range(3)))
    print(tag, "forces after 45 steps against the reference at the gathered positions: %.2e" % err)
    assert err < TIGHT, tag
    one = one_domain_45(variant)
    for q, k in enumerate(E_KEYS):
        if k in KINDS + ("total",):          # every term is booked once, by the owner of its first atom
            assert abs(res["e"][q] - one["e"][q]) < TIGHT * abs(one["e"][q]), (tag, k)
    return r45


@pytest.mark.parametrize("grid", GRIDS)
def test_decomposed_before_and_after_45_steps(grid):
    """(e) in-process domains: the L300 and G copies are cut by the faces, partners are halo beads, beads migrate within the 45 steps"""
    from ddcmd_amd.martini import domain_of
    import copy
    variant = "lds"
    s, terms, info = bs.make_bonded_setup(variant)
    owner = domain_of(s, grid)
    for kind in ("L300", "G"):
        assert np.unique(owner[info["kind"] == kind]).size > 1, (kind, grid)
    r45 = check_group(s, terms, run_group(s, terms, grid), variant, "%dx%dx%d" % grid)
    s45 = copy.copy(s)
    s45.rx, s45.ry, s45.rz = r45[:, 0], r45[:, 1], r45[:, 2]
    moved = domain_of(s45, grid) != owner
    assert moved.sum() > 0 and moved[info["mol"] >= 0].sum() > 0, grid


def test_partners_out_of_the_receive_buffer(monkeypatch):
    """(e) through the RCCL loopback with the pair kernel on the halo is staged from the exchange's receive buffer and the bonded kernels
    take received partners out of it (bead() with hrecv3): bit for bit the run with DDCMI_NO_DIRECT_HALO=1, and the reference's forces"""
    import ctypes
    from ddcmd_amd.martini import MartiniRank, _declare_domains
    variant = "lds"
    s, terms, _ = bs.make_bonded_setup(variant, nonbonded=True)

    def rank():
        monkeypatch.setenv("DDCMI_RCCL_LOOPBACK", "1")
        monkeypatch.setenv("DDCMI_HALO_OVERLAP", "0")
        m = with_terms(terms, lambda: MartiniRank(s, np.arange(s.natoms)))
        _declare_domains(m.lib)
        buf = ctypes.create_string_buffer(128)
        assert m.lib.ddcmi_comm_unique_id(buf) == 0
        m.comm_init(0, 1, buf.raw, (1, 1, 1))
        m.upload_local()
        return m

    monkeypatch.delenv("DDCMI_NO_DIRECT_HALO", raising=False)
    a = rank()
    monkeypatch.setenv("DDCMI_NO_DIRECT_HALO", "1")
    b = rank()
    monkeypatch.delenv("DDCMI_NO_DIRECT_HALO", raising=False)
    a.eval_forces(); b.eval_forces()
    for n in (1, 19, 25):
        a.step(n); b.step(n)
        pa, pb = a.download_particles(), b.download_particles()
        assert np.array_equal(pa["gid"], pb["gid"])
        for k in ("r", "v", "f"):
            for c in range(3):
                assert np.array_equal(pa[k][c], pb[k][c]), (n, k, c)
    ea, eb = a.energies()[0], b.energies()[0]
    for k in KINDS:
        assert abs(ea[k] - eb[k]) <= 1e-12 * abs(eb[k]), k
    a.close(); b.close()
    order = np.argsort(pa["gid"], kind="stable")          # the setup's gids ascend with the bead number
    r = np.stack([pa["r"][c][order] for c in range(3)], axis=1)
    fr = bs.reference(s, terms, r)[0].astype(np.float64)
    assert rel_force_err([pa["f"][c][order] for c in range(3)], tuple(fr[:, c] for c in range(3))) < TIGHT


@pytest.mark.parametrize("mode", ["single", "group222"])
def test_exactly_sized_buffers_with_canaries(mode, tmp_path):
    """(f) DDCMI_DEBUG_GUARD=1 (read at load: a child process) on the variant with as many patterns as atoms: every device buffer exactly
    as large as asked for with a canary behind it -- the rows' read-ahead padding is really there.  The run ends without a complaint
    and computes what the reference computes"""
    variant = "light_spills"
    s, terms, _ = bs.make_bonded_setup(variant)
    res, err = child(variant, False, mode, str(tmp_path / "guard.npz"), {"DDCMI_DEBUG_GUARD": "1"})
    assert "write beyond a device buffer" not in err, err[-2000:]
    if mode == "group222":
        check_group(s, terms, res, variant, "guard 2x2x2")
        return
    e0 = dict(zip(E_KEYS, res["e0"].tolist()))
    check_against(list(res["f0"]), e0, res["vir0"], ref0(variant), "guard one domain")
    fr = bs.reference(s, terms, res["r"].T)[0].astype(np.float64)
    assert rel_force_err(list(res["f"]), tuple(fr[:, c] for c in range(3))) < TIGHT and res["rebuilds"] == 3

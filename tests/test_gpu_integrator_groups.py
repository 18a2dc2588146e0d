"""The velocity updates on the device -- k_kick_drift, k_kick_ke, k_kick_ke_drift, the pair kernel's fused epilogue, the lean step
and the in-process group's phases -- against the numpy reference of tests/integrator_reference.py (itself held against the oracle
by tests/test_integrator_reference_host.py), with the groups' kinds MIXED, group ids up to 31, empty groups, three species of
different mass, and bead counts either side of the kernels' block edges: 64 (wave), 256 (k_kick_drift), 1024 (KE_PER * DDCMI_BLOCK of
k_kick_ke / k_kick_ke_drift) and 131 072 (the stride of k_group_ke / k_class_kinetic).

Gates (those of tests/test_integrator_closed_forms.py): v within 1e-12 max|v|, r within 1e-10 bohr modulo the box, rk, tion, the
group temperatures and kinetic_detail within 1e-12 of the system's sums.  An update is about ten float64 roundings, the normals add
a few ulp of libm, a run has at most 8 steps: below 1e-14.

Worst deviation seen over the whole matrix on an MI355X, as a fraction of the gate (v / r / rk / tion / T / detail by group / by
species): see WORST, printed when the module's tests are over (pytest -s)."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest

import integrator_paths_worker as paths
import integrator_reference as ir
from ranks import run_ranks
from ddcmd_amd import martini
from ddcmd_amd.martini import MartiniHIP, MartiniGroup

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [("all-32", n) for n in ir.SIZES] + [(t, n) for t in ("mixed", "holes", "free+equal-berendsen") for n in ir.TABLE_SIZES]
CASE_IDS = ["%s-%d" % c for c in CASES]
BATCHES = {"single": [1] * 6, "k2": [2, 2, 2], "k5": [5, 3]}
VARIANTS = dict(argnames="interacting", argvalues=[False, True], ids=["force-free", "interacting"])
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst deviation / gate over the matrix: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _forces(m):
    return np.stack(m.download(martini.FORCE)["f"])


def _state(m):
    d = m.download(martini.POS | martini.VEL)
    return np.stack(d["r"]), np.stack(d["v"])


def _start(s, m=None):
    m = m or MartiniHIP(s)
    m.eval_forces()
    m.group_temperatures()
    ref = ir.NGLFReference(s, lcg=s.lcg64)
    ref.publish()
    return m, ref


def _boundary(m, ref, s, what):
    """a publication on both sides, then everything a print step reads"""
    T = m.group_temperatures()
    ref.publish()
    r, v = _state(m)
    _, _, rk, tion = m.energies()
    ir.compare(ref, s, r, v, rk, tion, T, m.kinetic_detail(0), m.kinetic_detail(1), worst=WORST, what=what)


def _lcg_end(m, ref, s):
    if s.lcg64 is not None:
        got = m.get_random_lcg64()
        assert np.array_equal(got["state"], ref.lcg["state"]) and not np.array_equal(got["state"], s.lcg64["state"])
        assert np.array_equal(got["prime"], ref.lcg["prime"]) and np.array_equal(got["multID"], ref.lcg["multID"])


def drive_free_flight(s, sizes, m=None):
    """force-free: the reference needs nothing from the device.  step(k), a publication between batches only"""
    m, ref = _start(s, m)
    zero = np.zeros((3, s.natoms))
    try:
        for b, k in enumerate(sizes):
            for _ in range(k):
                ref.front(zero)
                ref.back(zero)
            m.step(k)
            _boundary(m, ref, s, "%d beads, batch %d of %d steps" % (s.natoms, b, k))
        assert m.clock()[0] == ref.loop
        _lcg_end(m, ref, s)
    finally:
        m.close()


def drive_interacting(s, sizes, m=None):
    """interacting, single steps with a publication between batches only: after every step the forces come down and feed the
    reference's next half kicks; every step is compared.  Returns what a batched run of the same boundaries must repeat bit for bit."""
    m, ref = _start(s, m)
    out = []
    try:
        f = _forces(m)
        for b, k in enumerate(sizes):
            for q in range(k):
                ref.front(f)
                m.step(1)
                f = _forces(m)
                ref.back(f)
                r, v = _state(m)
                _, _, rk, tion = m.energies()
                ir.compare(ref, s, r, v, rk, tion, None, None, None, worst=WORST, what="%d beads, batch %d step %d" % (s.natoms, b, q))
            _boundary(m, ref, s, "%d beads, batch %d" % (s.natoms, b))
            out.append(_bits(m))
        _lcg_end(m, ref, s)
    finally:
        m.close()
    return out


def _bits(m):
    d = m.download()
    e, vir, rk, tion = m.energies()
    return [np.stack(d["r"]), np.stack(d["v"]), np.stack(d["f"]), np.array([e["total"], rk]), vir, tion, np.array(m.clock())]


def drive_batches_bitwise(s, sizes, want):
    """batched and single steps agree bit for bit (and with them fused and split, lean and plain steps)"""
    m, _ = _start(s)
    try:
        for b, k in enumerate(sizes):
            m.step(k)
            m.group_temperatures()
            for name, a, w in zip(("r", "v", "f", "e rk", "virial", "tion", "clock"), _bits(m), want[b]):
                assert np.array_equal(a, w), "batch %d of %d steps: %s differs from the single steps by %.3g" % (b, k, name, np.abs(a - w).max())
    finally:
        m.close()


def run_case(s, batch, interacting):
    sizes = BATCHES[batch]
    if not interacting:
        return drive_free_flight(s, sizes)
    want = drive_interacting(s, sizes)
    if batch != "single":
        drive_batches_bitwise(s, sizes, want)


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize(**VARIANTS)
@pytest.mark.parametrize("table,n", CASES, ids=CASE_IDS)
def test_mixed_groups_follow_the_reference(table, n, interacting, batch):
    run_case(ir.make_system(n, table, interacting), batch, interacting)


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize(**VARIANTS)
@pytest.mark.parametrize("n", [65, 257])
def test_lcg64_streams_follow_the_reference(n, interacting, batch):
    """the Langevin groups draw from the beads' own LCG64 streams: the same velocities, and the final states bit for bit"""
    run_case(ir.make_system(n, "mixed", interacting, lcg=True), batch, interacting)


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize(**VARIANTS)
def test_a_run_that_starts_at_loop_7(interacting, batch):
    """set_clock(loop = 7): loop % interval is out of phase with a fresh start, and the noise counters start at 14"""
    run_case(ir.make_system(65, "mixed", interacting, loop=7), batch, interacting)


@pytest.mark.parametrize("no_lean", [False, True], ids=["lean", "DDCMI_NO_LEAN_STEP"])
@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize(**VARIANTS)
@pytest.mark.parametrize("n", ir.TABLE_SIZES)
def test_free_groups_with_and_without_the_lean_step(n, interacting, batch, no_lean, monkeypatch):
    """all groups FREE: batches run lean steps unless DDCMI_NO_LEAN_STEP is set when the context is created"""
    if no_lean:
        monkeypatch.setenv("DDCMI_NO_LEAN_STEP", "1")
    else:
        monkeypatch.delenv("DDCMI_NO_LEAN_STEP", raising=False)
    run_case(ir.make_system(n, "free", interacting), batch, interacting)


@pytest.fixture(scope="module")
def split_runs(tmp_path_factory):
    """run (c) of every case, in ONE child process: DDCMI_NO_FUSED_STEP is read once per process"""
    out = str(tmp_path_factory.mktemp("paths") / "split.npz")
    env = dict(os.environ, DDCMI_NO_FUSED_STEP="1")
    env.pop("DDCMI_NO_LEAN_STEP", None)
    res = run_ranks([[sys.executable, os.path.join(HERE, "integrator_paths_worker.py"), out]], [env], timeout=300, check=True)
    assert "integrator_paths_worker ok" in res[0].stdout
    return dict(np.load(out))


@pytest.mark.parametrize("table,n,lcg", paths.CASES, ids=paths.IDS)
def test_the_step_paths_agree_bit_for_bit(table, n, lcg, split_runs, monkeypatch, request):
    """Six interacting steps by every path the StepPlan can take, held against each other byte for byte: (a) six calls of one step
    (k_kick_ke, then k_kick_drift), (b) one call of six (k_kick_ke_drift, or the pair kernel's fused epilogue where fuse_ok holds),
    (c) the same under DDCMI_NO_FUSED_STEP (k_kick_ke_drift for every table; a child process), (d) all groups FREE only: the same
    under DDCMI_NO_LEAN_STEP (the fused epilogue, its sums reduced after every step).  Compared: r, v, the group temperatures and the
    LCG64 states behind step 6, and rk and tion of step 6 -- a batched call shows its sums at its end only.  The temperatures are read
    once, behind step 6, in run (a) too: a read between the steps would hand Berendsen other averages than the batched runs see."""
    s = ir.make_system(n, table, True, lcg=lcg)
    monkeypatch.delenv("DDCMI_NO_LEAN_STEP", raising=False)
    a = paths.six_steps(s, BATCHES["single"])
    case = request.node.callspec.id
    runs = {"one call of 6 steps": paths.six_steps(s, [6]),
            "DDCMI_NO_FUSED_STEP": {k[len(case) + 1:]: v for k, v in split_runs.items() if k.startswith(case + " ")}}
    if table == "free":
        monkeypatch.setenv("DDCMI_NO_LEAN_STEP", "1")      # (read when the context is created)
        runs["DDCMI_NO_LEAN_STEP"] = paths.six_steps(s, [6])
    assert a["sums"].shape == (6, 7) and ("lcg" in a) == lcg
    for what, b in runs.items():
        assert sorted(b) == sorted(a), (what, sorted(b))
        assert b["sums"].shape == (1, 7)
        assert np.array_equal(b["sums"][0], a["sums"][5]), "%s: rk, tion of step 6 differ from the single steps' by %.3g" % (what, np.abs(b["sums"][0] - a["sums"][5]).max())
        for name in ("r", "v", "T", "lcg")[:4 if lcg else 3]:
            assert np.array_equal(b[name], a[name]), "%s: %s differs from the single steps'" % (what, name)
    assert not np.array_equal(a["v"], np.stack([s.vx, s.vy, s.vz]))      # (the steps did something)
    if lcg:
        assert not np.array_equal(a["lcg"], s.lcg64["state"])


def test_kinetic_sums_past_the_stride_of_their_kernels():
    """131 073 beads: the smallest count that sends k_group_ke and k_class_kinetic (GKE_BLOCKS * DDCMI_BLOCK = 131 072 beads per
    sweep) into the second iteration of their stride loops -- for one bead, the last"""
    s = ir.make_system(131073, "all-32", False)
    m = MartiniHIP(s)
    try:
        ref = ir.NGLFReference(s)
        ref.publish()
        T = m.group_temperatures()
        rk, tion = m.kinetic()
        tot = ir.class_sums(np.zeros(s.natoms, int), 1, ref.m, ref.v)[0]
        ref.rk, ref.tion = float(tot[0]), tot[1:7].astype(np.float64)
        r, v = _state(m)
        dev = ir.compare(ref, s, r, v, rk, tion, T, m.kinetic_detail(0), m.kinetic_detail(1), worst=WORST, what="131073 beads")
        assert dev["v"] == 0.0
        assert int(round(m.kinetic_detail(1)[:, 8].sum())) == 131073 and int(round(m.kinetic_detail(0)[:, 8].sum())) == 131073
    finally:
        m.close()


def test_in_process_group_with_an_empty_domain():
    """2 x 1 x 1 domains of an in-process group, every bead in the lower half of the box along x: the second domain holds none"""
    s = ir.make_system(257, "mixed", False)
    L = s.h[0]
    s.rx = 0.5 * (s.rx - L * np.rint(s.rx / L) + 0.5 * L) - 0.5 * L
    g = MartiniGroup(s, (2, 1, 1))
    try:
        g.eval_forces()
        assert [int(r.lib.ddcmi_nlocal(r.ctx)) for r in g.ranks] == [257, 0]
        g.group_temperatures()
        ref = ir.NGLFReference(s)
        ref.publish()
        zero = np.zeros((3, s.natoms))
        order = np.argsort(np.asarray(s.gid, dtype=np.uint64), kind="stable")
        for step in range(6):
            ref.front(zero)
            ref.back(zero)
            g.step(1)
            T = g.group_temperatures()
            ref.publish()
            d = g.gather()
            assert np.array_equal(d["gid"], np.asarray(s.gid, dtype=np.uint64)[order])
            r, v = np.zeros((3, s.natoms)), np.zeros((3, s.natoms))
            r[:, order], v[:, order] = np.stack(d["r"]), np.stack(d["v"])
            _, _, rk, tion = g.energies()
            ir.compare(ref, s, r, v, rk, tion, T, None, None, worst=WORST, what="group step %d" % step)
    finally:
        g.close()


# ---- the setters under an uploaded state -----------------------------------------------------------------------------------
_IP, _DP = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)


def _set_groups(m, kinds, Teq, tau, interval):
    k, T, t, iv = np.array(kinds, np.int32), np.array(Teq, np.float64), np.array(tau, np.float64), np.array(interval, np.int32)
    rc = m.lib.ddcmi_set_groups(m.ctx, len(kinds), k.ctypes.data_as(_IP), T.ctypes.data_as(_DP), t.ctypes.data_as(_DP), iv.ctypes.data_as(_IP))
    return rc, m.lib.ddcmi_last_error(m.ctx).decode()


@pytest.mark.parametrize("kinds", [[ir.LANGEVIN, 7], [ir.BERENDSEN, ir.BERENDSEN, 7]], ids=["same-count", "growing-count"])
def test_a_refused_set_groups_changes_nothing(kinds):
    """an unknown kind behind valid groups: DDCMI_EUNSUPPORTED with a message, and the run goes on bit for bit like its twin that
    never saw the call (the call used to keep the groups in front of the one it refused -- and with a larger count the next step wrote
    past the Berendsen scalars on the host)"""
    s = ir.make_system(257, "two-berendsen", True)
    a, b = MartiniHIP(s), MartiniHIP(s)
    try:
        for m in (a, b):
            m.eval_forces()
            m.group_temperatures()
            m.step(3)
            m.group_temperatures()
        ng = len(kinds)
        rc, msg = _set_groups(a, kinds, [s.group_Teq[1]] * ng, [s.group_tau[1]] * ng, [1] * ng)
        assert rc == -4 and "group %d" % (ng - 1) in msg and len(msg) > 20, (rc, msg)
        for step in range(5):
            for m in (a, b):
                m.step(1)
            Ta, Tb = a.group_temperatures(), b.group_temperatures()
            assert np.array_equal(Ta, Tb)
            for name, x, y in zip(("r", "v", "f", "e rk", "virial", "tion", "clock"), _bits(a), _bits(b)):
                assert np.array_equal(x, y), "step %d after the refused call: %s differs" % (step, name)
        assert np.abs(Ta / s.group_Teq - 1.0).max() > 1e-3      # (the thermostats were still at work)
    finally:
        a.close()
        b.close()


def test_set_species_under_an_uploaded_state():
    """a table shorter than the beads' species ids is refused (the kick would read past it); one of the same length with new masses takes
    effect, and the kick then follows the reference with the new masses"""
    s = ir.make_system(65, "mixed", True)
    m = MartiniHIP(s)
    f64, i32 = lambda a: np.ascontiguousarray(a, dtype=np.float64), lambda a: np.ascontiguousarray(a, dtype=np.int32)

    def set_species(nsp, mass):
        ma, ch, lj, mt = f64(mass), f64(s.charge[:nsp]), i32(s.ljtype[:nsp]), i32(s.moltype[:nsp])
        rc = m.lib.ddcmi_set_species(m.ctx, nsp, ma.ctypes.data_as(_DP), ch.ctypes.data_as(_DP), lj.ctypes.data_as(_IP), mt.ctypes.data_as(_IP))
        return rc, m.lib.ddcmi_last_error(m.ctx).decode()

    try:
        m.eval_forces()
        rc, msg = set_species(2, s.mass[:2])
        assert rc == -2 and "2 species" in msg and "species 2" in msg, (rc, msg)
        s2 = copy.copy(s)
        s2.mass = s.mass * np.array([0.5, 3.0, 1.25])
        rc, msg = set_species(3, s2.mass)
        assert rc == 0, msg
    except BaseException:
        m.close()
        raise
    drive_interacting(s2, BATCHES["single"], m=m)

"""GPU tests (-m gpu) of the shell-limited walk of the pair kernel on the head-on colliders of tests/approach_systems.py: between
rebuilds k_nonbond ends every row at the last distance shell a pair could have left, by a displacement bound D that reaches it as a
word the reduction launches add to, a ring of per-step words the lean steps file, and -- decomposed -- a measured halo displacement or
a full walk.  A bound wrong in the unsafe direction loses a pair's force without a fault.  Here every moving bead has the same
speed, pairs approach head-on from the shells' inner edges, and the first step at which a shell must be walked again is a step at
which a pair of that shell is inside the cut-off (tests/test_approach_systems_host.py proves it of the inputs): the context is
compared bit for bit with one that walks every entry (DDCMI_NO_SHELL_SKIP=1), its forces with an all-pairs longdouble reference, and
the bound itself (ddcmi_debug_disp) with the real displacements (sound) and with sum dt max |v| of the oracle (tight).
docs/shell_walk_variants.md records eight mutations of the decision and which of these tests each turns red."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle
import approach_systems as A
from approach_worker import run_one_call
from ranks import rank_env, run_ranks

pytestmark = pytest.mark.gpu
TOL = 1e-6          # energies along a trajectory (tests/test_gpu_parity.py)
FORCE_TOL = 1e-10   # max |f - f_ref| / max |f_ref| (docs/molecule_exclusion_variants.md)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = {"single_steps": None, "one_call": None, "mixed": (3, 4, 4, 3, 3, 8)}


def pattern_of(name, nsteps):
    return {"single_steps": (1,) * nsteps, "one_call": (nsteps,)}.get(name) or PATTERNS[name]


def need_lean():
    if any(os.environ.get(k) for k in ("DDCMI_NO_LEAN_STEP", "DDCMI_NO_SELF_IMAGES", "DDCMI_NO_FUSED_STEP")):
        pytest.skip("the lean step is switched off in this environment")


def two_contexts(s, monkeypatch, make):
    """a: the default; b: created under DDCMI_NO_SHELL_SKIP=1 (walks every entry)"""
    monkeypatch.delenv("DDCMI_NO_SHELL_SKIP", raising=False)
    a = make(True)
    monkeypatch.setenv("DDCMI_NO_SHELL_SKIP", "1")
    b = make(False)
    monkeypatch.delenv("DDCMI_NO_SHELL_SKIP", raising=False)
    return a, b


def single(s):
    from ddcmd_amd.martini import MartiniHIP
    return lambda test_api: MartiniHIP(s, test_api=test_api)


def debug_disp(m):
    """(the reduction launches' word, the ring's words, words in use) -- include/ddcmi_test.h"""
    m.lib.ddcmi_debug_disp.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
    D, ring, nr = ctypes.c_double(0), (ctypes.c_float * 64)(), ctypes.c_int(0)
    m._chk(m.lib.ddcmi_debug_disp(m.ctx, ctypes.byref(D), ring, ctypes.byref(nr)))
    return D.value, [float(ring[q]) for q in range(A.LEAN_W)], nr.value


def bound_of(word, ring, nring, ring_dt):
    """the bound as tools/disp_bound_r06.py forms it: the word + dt sqrt of the decaying maximum over the ring"""
    e, bound = 0.0, word
    for q in range(nring):
        e = max(ring[q], e * A.LEAN_C)
        bound += ring_dt * np.sqrt(e)
    return bound


def state(m):
    d = m.download()
    return {k: np.stack(d[k], 1) for k in ("r", "v", "f")}


def assert_same_bits(a, b, da, db, tag):
    for k in ("r", "v", "f"):
        assert np.array_equal(da[k], db[k]), (tag, k, int((da[k] != db[k]).any(axis=1).sum()), "beads differ")
    (ea, va, rka, ta), (eb, vb, rkb, tb) = a.energies(), b.energies()
    assert ea == eb and np.array_equal(va, vb) and rka == rkb and np.array_equal(ta, tb), tag


def assert_reference_forces(s, r, f, tag):
    """forces against the longdouble all-pairs reference at the SAME positions, and the same set of beads with a force at all"""
    ref = np.asarray(A.reference_forces(s, r), np.float64)
    scale = np.abs(ref).max()
    err = np.abs(f - ref).max() / scale
    print("%s: max |f - f_ref| / max |f_ref| = %.2e, %d beads with a force" % (tag, err, int((ref != 0).any(axis=1).sum())))
    assert scale > 0 and err <= FORCE_TOL, (tag, err)
    lost = np.flatnonzero((ref != 0).any(axis=1) != (f != 0).any(axis=1))
    assert lost.size == 0, (tag, "beads whose force is zero on one side only", lost.tolist())


def run_pattern(s, pattern, monkeypatch, dts=None, bound=False, forces=True, tag=""):
    """a and b through the calls of a pattern; after every call the checks of test_head_on_pairs and (bound) test_bound_is_sound_and_tight.
    The real displacement is measured between DEVICE positions: a's download at this call's end against the download at the last
    rebuild -- a's, or, where the rebuild falls inside a call of a's, the full walk's, which takes that call in two (the two contexts are
    equal bit for bit wherever both are downloaded, and a state does not depend on how the steps before it were cut into calls:
    test_lean_steps_equal_steps_with_a_reduction_launch_each)"""
    a, b = two_contexts(s, monkeypatch, single(s))
    nsteps = sum(pattern)
    dts_step = [s.dt] * nsteps if dts is None else [dt for k, dt in zip(pattern, dts) for _ in range(k)]
    R, V = A.oracle_trajectory(s, nsteps, dts_step)
    sch = A.schedule(s, nsteps, R)
    a.eval_forces(); b.eval_forces()
    r_rebuild, ur = state(a)["r"], int(s.updateRate)
    lean = A.lean_steps_after(pattern, int(s.updateRate)) if dts is None else None
    out, n = [], 0
    box = A.box_of(s)
    for c, k in enumerate(pattern):
        dt = None if dts is None else dts[c]
        a.step(k, dt)
        last = ((n + k) // ur) * ur
        if n < last < n + k:          # a rebuild inside this call: the full walk takes the call in two, and its positions at the rebuild are the device's
            b.step(last - n, dt)
            r_rebuild = state(b)["r"]
            b.step(n + k - last, dt)
        else:
            b.step(k, dt)
        n += k
        da, db = state(a), state(b)
        if last == n:
            r_rebuild = da["r"]
        t = "%s call %d (step %d)" % (tag, c, n)
        assert_same_bits(a, b, da, db, t)
        if forces:
            assert_reference_forces(s, da["r"], da["f"], t)
        if bound:
            word, ring, nring = debug_disp(a)
            D = bound_of(word, ring, nring, s.dt)
            dr = A.min_image(da["r"] - r_rebuild, box)
            real = np.sqrt((dr * dr).sum(axis=1)).max()
            S = sch[n]["D"]
            print("%s: bound %.9f A = word %.6f + %d ring words, real %.9f A, sum dt max|v| %.9f A" % (t, D / A.ANG, word / A.ANG, nring, real / A.ANG, S / A.ANG))
            assert D >= real * (1.0 - 1e-12), (t, D, real)
            assert D <= S * (1.0 + A.ROUND_UP), (t, D, S)
            if lean is not None:
                assert nring == lean[c], (t, nring, lean[c])
            out.append((n, word, nring))
    # the end state against the oracle, at the tolerances of tests/test_gpu_parity.py for a run across a rebuild
    dr = A.min_image(da["r"] - R[-1], box)
    assert np.abs(dr).max() < 1e-8, tag
    assert np.abs(da["v"] - V[-1]).max() < 1e-8 * np.abs(V[-1]).max(), tag
    assert a.list_stats()["rebuilds"] == 1 + nsteps // int(s.updateRate)
    a.close(); b.close()
    return out


@pytest.mark.parametrize("variant,calls", [(v, c) for v in ("one_type", "types20") for c in PATTERNS] + [("charged", "mixed")])
def test_head_on_pairs(variant, calls, monkeypatch):
    """after every call of the pattern (every step split / every step but the last lean / lean-ending and split-ending steps on the
    re-admission steps 4 7 11 14 17): r, v, f and energies of the default context equal the full walk's bit for bit; forces against the
    longdouble reference at the downloaded positions within 1e-10 of the largest, the same beads with a non-zero force; at the end r and
    v against the oracle.  one_type: the shift bit rides in the list entry; types20: bare entries, tags in the staged z; charged:
    k_nonbond<HAS_Q>"""
    need_lean()
    s = A.system(variant)
    run_pattern(s, pattern_of(calls, int(s.updateRate) + 5), monkeypatch, tag="%s %s" % (variant, calls))


@pytest.mark.parametrize("calls", list(PATTERNS))
def test_bound_is_sound_and_tight(calls, monkeypatch):
    """the bound itself, read through ddcmi_debug_disp after every call: >= the largest real displacement since the rebuild (no
    tolerance beyond 1e-12 relative), <= S (1 + 1e-4), S = sum dt max |v| of the oracle -- the 1e-4 covers |v|^2 kept as a float rounded
    up and the factors (1 + 1e-7), (1 + 2e-6)(1 + 1e-6) the code multiplies its terms by, 3.2e-6 in all, and the oracle's |v| against
    the device's (1e-9); the ring holds as many words as the pattern has lean steps since the rebuild"""
    need_lean()
    s = A.system("one_type")
    run_pattern(s, pattern_of(calls, int(s.updateRate) + 5), monkeypatch, bound=True, forces=False, tag="bound %s" % calls)


@pytest.mark.parametrize("pattern", [(45,), (33, 12), (35, 10)])
def test_period_longer_than_the_ring(pattern, monkeypatch):
    """a rebuild period of 40 steps: the ring of 32 words fills, the steps behind it add to the reduction launches' word while the
    ring still carries the first 32 -- all of test_head_on_pairs and test_bound_is_sound_and_tight, and after 35 steps in one call
    32 words in use and a word of three steps' drift (the call's first, steps 34 and 35)"""
    need_lean()
    s = A.system("one_type", update_rate=40, step_A=0.05)
    out = run_pattern(s, pattern, monkeypatch, bound=True, tag="period 40 %s" % (pattern,))
    if pattern[0] == 35:
        n, word, nring = out[0]
        assert nring == A.LEAN_W and 2.9 * s.dt * s.vmax < word < 3.2 * s.dt * s.vmax, (word / (s.dt * s.vmax), nring)
    if pattern[0] == 33:
        assert out[0][2] == A.LEAN_W and 0.99 * s.dt * s.vmax < out[0][1] < 1.01 * s.dt * s.vmax


def test_dt_changes_inside_a_period(monkeypatch):
    """step(6), step(6, dt / 2), step(6): the steps at the other dt leave the lean path (the ring's words keep the first dt) and add to the
    reduction launches' word; shell 4 is re-admitted inside the second call, at step 8, with its edge pair inside the cut-off.  Bit for bit
    the full walk, forces against the longdouble reference, the bound sound and tight; the oracle takes a dt per step, so it is part of this"""
    need_lean()
    s = A.system("one_type")
    out = run_pattern(s, (6, 6, 6), monkeypatch, dts=(s.dt, 0.5 * s.dt, s.dt), bound=True, tag="dt change")
    assert [o[2] for o in out] == [5, 5, 10], out
    step = s.dt * s.vmax
    assert 0.99 * step < out[0][1] < 1.01 * step and 3.99 * step < out[1][1] < 4.03 * step, [o[1] / step for o in out]


def test_projectile_and_velocity_jumps(monkeypatch):
    """thermal water at 1 K with ONE fast bead (dt |v| updateRate just under skin / 2): the bound is that bead's, everybody around it
    walks short rows at first.  Default context, full walk and oracle over updateRate + 5 steps in the mixed call pattern; the bound
    sound after every call.
    The velocity jumps the issue describes are left out: no upload keeps the walk -- ddcmi_upload_state clears list_valid and
    ddcmi_upload_positions (the only upload of velocities between rebuilds, positions required) clears shell_skip until the next
    rebuild, so after either the rows are walked to the end and the ring is not read."""
    need_lean()
    s = A.projectile()
    a, b = two_contexts(s, monkeypatch, single(s))
    o = pyoracle.Oracle(s)
    o.forces()
    a.eval_forces(); b.eval_forces()
    r0, n, box = state(a)["r"], 0, A.box_of(s)
    for c, k in enumerate(PATTERNS["mixed"]):
        a.step(k); b.step(k)
        eo, vo, rko, _ = o.step(k)
        n += k
        da, db = state(a), state(b)
        assert_same_bits(a, b, da, db, "projectile call %d" % c)
        ea, _, rka, _ = a.energies()
        assert abs(ea["total"] - eo["total"]) < TOL * abs(eo["total"]) and abs(rka - rko) < TOL * rko, c
        if n < int(s.updateRate):
            word, ring, nring = debug_disp(a)
            dr = A.min_image(da["r"] - r0, box)
            real = np.sqrt((dr * dr).sum(axis=1)).max()
            D = bound_of(word, ring, nring, s.dt)
            print("projectile step %d: bound %.6f A, real %.6f A" % (n, D / A.ANG, real / A.ANG))
            assert D >= real * (1.0 - 1e-12), (n, D, real)
            assert nring == A.lean_steps_after(PATTERNS["mixed"], int(s.updateRate))[c]
    dr = A.min_image(da["r"] - np.stack([o.rx, o.ry, o.rz], 1), box)
    assert np.abs(dr).max() < 1e-8
    a.close(); b.close()


def test_split_step_reads_the_ring_per_wave(monkeypatch, tmp_path):
    """DDCMI_NO_FUSED_STEP=1 (read once per process: a child process, under a time limit): every step split, every drift in the reduction
    launches' word.  This process runs the same call lean: its last step and every force evaluation behind lean steps take k_nonbond<!FUSE>,
    which sums the ring once per wave.  r, v, f and energies after updateRate + 5 steps in one call agree bit for bit"""
    need_lean()
    s = A.system("one_type")
    base = run_one_call(s)
    env = dict(os.environ)
    env["DDCMI_NO_FUSED_STEP"] = "1"
    out = str(tmp_path / "split.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "approach_worker.py"), "one_type", out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "approach_worker ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    split = dict(np.load(out))
    assert int(base["rebuilds"]) == 2
    for k in sorted(base):
        assert np.array_equal(np.asarray(base[k]), np.asarray(split[k])), k
    assert_reference_forces(s, base["r"].T, base["f"].T, "one call, fused")


def by_gid(p):
    order = np.argsort(p["gid"], kind="stable")
    return {k: np.stack([p[k][c][order] for c in range(3)], 1) for k in ("r", "v", "f")}


def run_decomposed(s, a, b, get, tag):
    a.eval_forces(); b.eval_forces()
    for c, k in enumerate(PATTERNS["mixed"]):
        a.step(k); b.step(k)
        da, db = get(a), get(b)
        for q in ("r", "v", "f"):
            assert np.array_equal(da[q], db[q]), (tag, c, q, int((da[q] != db[q]).any(axis=1).sum()), "beads differ")
        (ea, va, rka, _), (eb, vb, rkb, _) = a.energies(), b.energies()
        assert ea == eb and np.array_equal(va, vb) and rka == rkb, (tag, c)
        assert_reference_forces(s, da["r"], da["f"], "%s call %d" % (tag, c))
    a.close(); b.close()


@pytest.mark.parametrize("grid", [(2, 2, 1), (2, 2, 2)])
def test_pairs_across_domain_faces(grid, monkeypatch):
    """an in-process group of domains, the collider built for the grid: probe pairs straddle every periodic face and every internal
    domain face, so one partner is a received bead whose displacement the halo update measures (hdisp).  Bit for bit the group that
    walks every entry over updateRate + 5 steps, gathered forces against the longdouble reference"""
    from ddcmd_amd.martini import MartiniGroup
    s = A.system("one_type", grid=grid)
    a, b = two_contexts(s, monkeypatch, lambda test_api: MartiniGroup(s, grid))
    run_decomposed(s, a, b, lambda g: by_gid(g.gather()), "group %dx%dx%d" % grid)


def test_pairs_across_the_faces_of_a_loopback_rank(monkeypatch):
    """a single rank behind the RCCL loopback transport: every image is a received bead staged from the receive buffer and the tiles
    that stage one walk their rows to the end (halo_full_walk).  This test cannot tell whether they do: the received beads are the
    rank's OWN beads' images, 2 D bounds them too, and the shortened walk gives the same bits -- what it holds is the wire and the
    all-owned tiles of such a rank, with pairs across the periodic faces.  test_movers_on_one_rank_only is the test of that line"""
    from test_gpu_rccl_loopback import _loopback_rank
    s = A.system("one_type")
    a, b = two_contexts(s, monkeypatch, lambda test_api: _loopback_rank(s, monkeypatch))
    run_decomposed(s, a, b, lambda m: by_gid(m.download_particles()), "loopback")


def rank_launch(d, pattern, extra_env):
    """commands and environments of the two ranks of one_sided() as fresh processes over the host transport"""
    envs = []
    for rank in range(2):
        env = rank_env(rank, 2, d)
        for k in ("DDCMI_NO_SHELL_SKIP", "DDCMI_HALO_OVERLAP", "DDCMI_NO_DIRECT_HALO"):
            env.pop(k, None)
        env.update(extra_env)
        envs.append(env)
    return [[sys.executable, os.path.join(ROOT, "tests", "approach_worker.py"), "rank", d, ",".join(str(k) for k in pattern)]] * 2, envs


def collect_ranks(d, res, ncalls):
    """the merged states by gid, one per download; any rank that failed ends the test"""
    for r in res:
        assert r.returncode == 0 and "approach_worker ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    recs = [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(2)]
    assert all(str(rec["transport"][0]) == "host" for rec in recs)
    states = []
    for c in range(ncalls + 1):
        gid = np.concatenate([rec["gid%d" % c] for rec in recs])
        order = np.argsort(gid, kind="stable")
        st = {k: np.concatenate([rec["%s%d" % (k, c)] for rec in recs])[order] for k in ("r", "v", "f")}
        st["gid"] = gid[order]
        st["nloc"] = [len(rec["gid%d" % c]) for rec in recs]
        states.append(st)
    return states


@pytest.mark.parametrize("calls", ["single_steps", "mixed"])
def test_movers_on_one_rank_only(calls, tmp_path):
    """two real ranks (2 x 1 x 1, host transport, the halo staged from the receive buffer): every mover of one_sided() lives on rank 0, so
    rank 1's own displacement bound stays at zero while the partners it receives come inside the cut-off from shells 3 and 4 -- its
    side of those pairs exists only because the tiles that stage received beads walk their rows to the end.  Against the same two
    ranks under DDCMI_NO_SHELL_SKIP=1 bit for bit, and against the longdouble reference, after every call.  single_steps: no launch
    reads the ring (the guard in front of the staging decides); mixed: lean launches (the guard behind it)"""
    s = A.one_sided()
    pattern = pattern_of(calls, int(s.updateRate) + 5)
    da, db = str(tmp_path / "a"), str(tmp_path / "b")
    os.mkdir(da); os.mkdir(db)
    (ca, ea), (cb, eb) = rank_launch(da, pattern, {}), rank_launch(db, pattern, {"DDCMI_NO_SHELL_SKIP": "1"})
    res = run_ranks(ca + cb, ea + eb, cwd=ROOT, timeout=120)      # both pairs side by side
    sa, sb = collect_ranks(da, res[:2], len(pattern)), collect_ranks(db, res[2:], len(pattern))
    assert sa[0]["nloc"] == [18, 18] and np.array_equal(sa[0]["gid"], np.asarray(s.gid))
    n = 0
    for c, (x, y) in enumerate(zip(sa, sb)):
        n += pattern[c - 1] if c else 0
        tag = "two ranks %s step %d" % (calls, n)
        for k in ("gid", "r", "v", "f"):
            assert np.array_equal(x[k], y[k]), (tag, k, int((x[k] != y[k]).reshape(len(x[k]), -1).any(axis=1).sum()), "beads differ")
        if n > 2:          # (nobody is inside the cut-off before step 3: the reference is zero everywhere)
            assert_reference_forces(s, x["r"], x["f"], tag)

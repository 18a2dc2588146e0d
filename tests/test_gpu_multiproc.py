"""GPU tests (-m gpu): the decomposed path between REAL processes on the one GPU a test box has.

RCCL refuses two ranks of a communicator on one device ("Duplicate GPU detected"), so two processes cannot share
a GPU over the RCCL transport; test_gpu_rccl_loopback.py covers the RCCL wire with one rank, test_gpu_domains.py
the multi-domain logic inside one process.  Here every rank is a fresh child process with its own HIP context,
its own address space and its own rank of the rendezvous, and the SAME libddcmi code path as the RCCL runs --
mg_phase1..4, the count all-gather, plan_recv_counts, the peer-major halo layout, migration, per-step halo
messages, the energy / group-temperature all-reduce -- with the messages carried by the host transport
(ddcmi_comm_init_host: pinned staging + the rendezvous' TCP streams).  The parent process checks the merged
result against the oracle.  The last test starts bench.py exactly as the driver does for N = 2."""
import json
import os
import subprocess
import sys
import tempfile
import numpy as np
import pytest

import pyoracle
import ddcmd_amd
from conftest import rel_force_err
from ddcmd_amd.deck import units_convert
from ranks import ROOT, rank_env, run_ranks

pytestmark = pytest.mark.gpu
KINDS = ("lj", "ele", "bond", "angle", "tors", "impr", "total")


def _worker_ranks(workload, grid, d, nsteps, block, extra_env=None, timeout=600, check=False):
    world = grid[0] * grid[1] * grid[2]
    cmd = [sys.executable, os.path.join(ROOT, "tests", "mp_worker.py"), workload, "%dx%dx%d" % grid, d, str(nsteps), str(block)]
    return run_ranks([cmd] * world, [rank_env(r, world, d, extra_env) for r in range(world)], timeout=timeout, check=check)


def _run_ranks(workload, grid, nsteps, block):
    with tempfile.TemporaryDirectory() as d:
        _worker_ranks(workload, grid, d, nsteps, block, check=True)
        return [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(grid[0] * grid[1] * grid[2])]


def test_a_failing_rank_ends_the_rebuild_on_every_rank():
    """a hard error of one rank inside the rebuild (here: a bead that is not a number, found by the last rank's
    list build) used to leave the other ranks inside the next exchange until the transport's 300 s timeout.  Every rank
    must return an error from the same rebuild, at once, and say whose error it is."""
    import time
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        res = _worker_ranks("water_fault", (2, 1, 1), d, 0, 1, timeout=120)
        assert time.time() - t0 < 100, "the ranks waited for each other"
        assert [r.returncode for r in res] == [3, 3], [(r.returncode, r.stderr[-800:]) for r in res]
        errs = [r.stderr for r in res]
        # the rank that holds the bead (migration may have handed it to the neighbour first) says what is wrong, its peer is told
        # whose error it is -- or both learn of a bead "further than one domain" away in the same count round
        own = [("non-finite" in e) for e in errs]
        told = [("failed during the list rebuild" in e) for e in errs]
        both = [("further than one domain" in e) for e in errs]
        # (since the flag rides in the halo count round, both ranks normally say "beads of rank r have non-finite coordinates")
        assert all(both) or all(own) or (any(own) and any(told) and all(a or b for a, b in zip(own, told))), errs
        if all(own):
            import re
            assert len({re.search(r"beads of rank (\d)", e).group(1) for e in errs}) == 1      # and they name the same rank


def _preflight_ranks(grid, extra_env, timeout=120):
    with tempfile.TemporaryDirectory() as d:
        res = _worker_ranks("water_preflight", grid, d, 0, 1, extra_env, timeout)
    return [r.returncode for r in res], [r.stderr for r in res]


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_preflight_between_real_processes(grid):
    """ddcmi_comm_preflight over the host transport between real processes -- one grouped exchange with every peer the
    brick plan names (2x2x2: seven distinct peers, 26 directions), the 24-double all-reduce, the count all-gather, all verified"""
    rcs, errs = _preflight_ranks(grid, {})
    assert rcs == [0] * len(rcs), errs
    world = len(rcs)
    for e in errs:
        assert "PREFLIGHT-OK" in e and "'stages_verified': 3" in e, e
        if world == 2:          # only the directions with dx != 0 leave the rank: 18 of 26, all to the one neighbour
            assert "'directions': 18" in e and ("'peers': [1]" in e or "'peers': [0]" in e), e
        else:
            import re
            assert "'directions': 26" in e and len(re.search(r"'peers': \[([^\]]*)\]", e).group(1).split(",")) == 7, e


def test_preflight_names_the_peer_and_direction_of_a_wrong_message():
    """fault injection: rank 1 spoils the message it sends along its direction code 14 = (+1, 0, 0); its +x neighbour (rank 0 on the
    periodic 2x1x1 grid) must say from whom and along which direction the data is wrong, and EVERY rank must leave non-zero"""
    rcs, errs = _preflight_ranks((2, 1, 1), {"DDCMI_DEBUG_HOOKS": "1", "DDCMI_DEBUG_PREFLIGHT_CORRUPT": "14", "DDCMI_DEBUG_PREFLIGHT_CORRUPT_RANK": "1"})
    assert rcs == [4, 4], (rcs, errs)
    assert "the message from rank 1" in errs[0] and "my direction (-1,+0,+0)" in errs[0] and "wrong at element 7" in errs[0], errs[0]
    assert "another rank's check of the communicator failed" in errs[1], errs[1]


def test_preflight_names_the_rank_that_was_given_other_parameters():
    """the all-gather of the preflight carries a hash of what every rank must have been given alike (box, cut-offs, neighbour settings, tables, species,
    molecule tables, term counts, groups, grid): rank 2 of four runs with a skin 1 % wider -- every rank leaves non-zero, and says who differs from it"""
    rcs, errs = _preflight_ranks((2, 2, 1), {"DDCMI_TEST_DETUNE_RANK": "2"})
    assert rcs == [4, 4, 4, 4], (rcs, errs)
    for r, e in enumerate(errs):
        if r == 2:
            assert "rank 0 was given other parameters than this rank" in e, e
        else:
            assert "rank 2 was given other parameters than this rank" in e and "same deck" in e, e


def test_preflight_ends_with_a_deadline_when_a_rank_stays_away():
    """fault injection: rank 1 never joins the exchange; rank 0 must give up at the transport's deadline (3 s here) naming rank 1, not hang"""
    import time
    t0 = time.time()
    rcs, errs = _preflight_ranks((2, 1, 1), {"DDCMI_DEBUG_HOOKS": "1", "DDCMI_DEBUG_PREFLIGHT_ABSENT": "1", "DDCMI_TEST_RDZV_TIMEOUT": "3",
                                              "DDCMI_TEST_PREFLIGHT_TIMEOUT": "3"})
    assert time.time() - t0 < 60
    assert rcs == [4, 4], (rcs, errs)
    assert "timed out after 3 s waiting for rank 1 (nothing received" in errs[0] and "grouped exchange with the brick's peers failed" in errs[0], errs[0]
    assert "stayed away" in errs[1], errs[1]


def _merge(recs, key_gid, key):
    gid = np.concatenate([r[key_gid] for r in recs])
    order = np.argsort(gid, kind="stable")
    return gid[order], np.concatenate([r[key] for r in recs], axis=1)[:, order]


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 2), (2, 2, 2)])
def test_water_between_processes(grid):
    """forces at step 0 and the state after 45 steps (two rebuilds with migration between the processes).  2x2x2: eight ranks, seven
    peers each, a halo of received beads only -- the bench's 8-GPU decomposition, and the configuration in which k_nonbond stages
    the neighbours' beads straight from the exchange's receive buffer (no halo update launch; round 5)"""
    s = ddcmd_amd.make_water_setup(12)          # 6912 beads, box 97.5 A: bricks of 48.7 A
    o = pyoracle.Oracle(s)
    e0, v0 = o.forces()
    f_ref0 = (o.fx.copy(), o.fy.copy(), o.fz.copy())
    recs = _run_ranks("water", grid, 45, 15)
    gid, f0 = _merge(recs, "gid0", "f0")
    assert np.array_equal(gid, np.sort(s.gid))
    assert rel_force_err(f0, f_ref0) < 1e-10
    assert abs(sum(r["e0"][0] for r in recs) - e0["lj"]) < 1e-10 * abs(e0["lj"])
    assert np.abs(sum(r["vir0"] for r in recs) - v0).max() < 1e-10 * np.abs(v0).max()
    for b in range(3):
        eo, vo, rko, _ = o.step(15)
        for r in recs:                          # every rank holds the same all-reduced numbers
            assert abs(r["traj"][b][0] - eo["total"]) < 1e-6 * abs(eo["total"])
            assert abs(r["traj"][b][1] - rko) < 1e-6 * rko
            assert np.abs(r["traj"][b][2:8] - vo).max() < 1e-6 * np.abs(vo).max()
            assert np.array_equal(r["traj"][b], recs[0]["traj"][b])
    gid, f = _merge(recs, "gid", "f")
    assert np.array_equal(gid, np.sort(s.gid)), "beads lost or duplicated in migration"
    assert [int(r["nloc"][1]) for r in recs] != [int(r["nloc"][0]) for r in recs], "no bead changed owner"
    assert all(int(r["rebuilds"][0]) >= 3 for r in recs)
    assert rel_force_err(f, (o.fx, o.fy, o.fz)) < 1e-6
    _, pos = _merge(recs, "gid", "r")
    L = s.h[0]
    for c, ref in enumerate((o.rx, o.ry, o.rz)):
        dr = pos[c] - ref
        dr -= L * np.rint(dr / L)
        assert np.abs(dr).max() < 1e-8
    _, vel = _merge(recs, "gid", "v")
    for c, ref in enumerate((o.vx, o.vy, o.vz)):
        assert np.abs(vel[c] - ref).max() < 1e-8 * np.abs(ref).max()


def test_lipid_deck_between_processes():
    """bonded terms by gid across a process boundary + the Berendsen group temperature, all-reduced over the transport"""
    from ddcmd_amd.deck import load_deck
    deck = os.path.join(ROOT, "tests", "golden", "lipid_deck")
    s = load_deck(os.path.join(deck, "object_nvt.data"), restart_file=os.path.join(deck, "relaxed", "restart"))
    o = pyoracle.Oracle(s)
    e0, v0 = o.forces()
    f_ref0 = (o.fx.copy(), o.fy.copy(), o.fz.copy())
    o.group_temperature()
    T0 = o.groups[0].temperature
    recs = _run_ranks("lipid", (1, 1, 2), 20, 10)
    gid, f0 = _merge(recs, "gid0", "f0")
    assert np.array_equal(gid, np.sort(s.gid))
    assert rel_force_err(f0, f_ref0) < 1e-9
    for k, name in enumerate(KINDS):
        assert abs(sum(r["e0"][k] for r in recs) - e0[name]) < 1e-9 * max(abs(e0[name]), 1e-12), name
    for r in recs:
        assert abs(r["Tg"][0][0] - T0) < 1e-10 * T0
    for b in range(2):
        eo, vo, rko, _ = o.step(10)
        o.group_temperature()
        for r in recs:
            assert abs(r["traj"][b][0] - eo["total"]) < 1e-6 * abs(eo["total"])
            assert abs(r["traj"][b][1] - rko) < 1e-6 * rko
            assert abs(r["Tg"][b + 1][0] - o.groups[0].temperature) < 1e-6 * T0
    gid, f = _merge(recs, "gid", "f")
    assert np.array_equal(gid, np.sort(s.gid))
    assert rel_force_err(f, (o.fx, o.fy, o.fz)) < 1e-6


def test_bench_world2_as_the_driver_launches_it():
    """python -m torch.distributed.run ... bench.py --gpus 2: two ranks, one device, host transport; the process maps
    only /opt/rocm's runtime, no bead is lost (bench.py asserts it) and the JSON line carries the contract's fields"""
    port = 29900 + os.getpid() % 90
    env = dict(os.environ)
    env.update({"DDCMI_BENCH_SINGLE_DEVICE": "1", "DDCMI_TRANSPORT": "host"})
    env.pop("DDCMI_RDZV_FILE", None); env.pop("DDCMI_RDZV_PORT", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "60", "--warmup", "20", "--lattice", "14"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 prints ONE JSON line"
    out = json.loads(lines[0])
    # "steps" says what was TIMED (exactly --steps, in windows of 20), "steps_requested" echoes --steps
    assert out["n_gpus"] == 2 and out["steps"] == 60 and out["steps_requested"] == 60 and out["steps_timed"] == 60 and out["value"] > 0 and out["scaling"] == "strong"
    pf = out["comm"]["preflight_rank0"]
    assert pf["stages_verified"] == 3 and pf["directions"] == 18 and pf["peers"] == [1] and out["comm"]["ranks_met"] == 2
    assert out["comm"]["peers_rank0"][0]["peer"] == 1 and out["comm"]["peers_rank0"][0]["send_bytes_per_step"] > 0
    assert out["config"]["beads_total"] == 4 * 14 ** 3 and 0 < out["config"]["beads_rank0"] < out["config"]["beads_total"]
    # 60 timed steps in windows of 20 (one rebuild each); the median window is the figure
    assert out["steps_timed"] == 60 and len(out["window_ms"]) == 3 and out["config"]["rebuilds_in_timed_region"] == 3
    assert abs(out["ms_per_step"] - sorted(out["window_ms"])[1] / 20.0) < 1e-9 * out["ms_per_step"] + 1e-4
    c = out["comm"]
    assert c["ranks_met"] == 2 and sum(c["beads_per_rank"]) == 4 * 14 ** 3 and len(c["halo_beads_sent_per_step"]) == 2
    assert c["transport"] == "host" and c["rccl_version"] and c["halo_bytes_per_step_all_ranks"] == 24 * sum(c["halo_beads_sent_per_step"]) > 0
    assert "cpu_baseline" not in out and "also" not in out               # rank 0 at N = 1 only
    for l in out["runtime_libs"]:
        assert os.path.realpath(l).startswith(os.path.realpath("/opt/rocm") + os.sep), l
    # the same box on one rank gives the same energies (the decomposition changes no physics)
    p1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "60", "--warmup", "20", "--lattice", "14", "--no-cpu"],
                        cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p1.returncode == 0, p1.stderr[-3000:]
    one = json.loads([l for l in p1.stdout.splitlines() if l.startswith("{")][0])
    assert abs(out["check"]["epot"] - one["check"]["epot"]) < 1e-7 * abs(one["check"]["epot"])
    assert abs(out["check"]["ekin"] - one["check"]["ekin"]) < 1e-7 * abs(one["check"]["ekin"])


def test_bench_gpus2_with_no_launcher_runs_two_ranks():
    """`python3 bench.py --gpus 2 ...` exactly as the driver starts N = 1 (no launcher, no WORLD_SIZE): the command
    starts its two ranks itself; n_gpus and the ranks that met say 2"""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "DDCMI_RDZV_FILE", "DDCMI_RDZV_PORT"):
        env.pop(k, None)
    env.update({"DDCMI_BENCH_SINGLE_DEVICE": "1", "DDCMI_TRANSPORT": "host"})      # (one GPU on the test box: both ranks on device 0, host-staged messages)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--lattice", "14", "--steps", "20", "--warmup", "5"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["comm"]["ranks_met"] == 2 and sum(out["comm"]["beads_per_rank"]) == 4 * 14 ** 3
    assert "2x1x1" in out["config"]["parallelism"] and out["value"] > 0


def test_bench_times_the_steps_asked_and_dumps_what_it_computed(tmp_path):
    """bench.py --steps K times exactly K steps (windows of 20, the last one shorter) and a plain run carries no side measurement;
    --dump-outputs writes what the timed path computed as float64 .npy files: the whole box at this size, energies as the line says,
    and two runs of the same arguments write the same bits (same inputs, and a run repeats bit for bit)"""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DDCMI_TRANSPORT", "DDCMI_RCCL_LOOPBACK"):
        env.pop(k, None)
    n = 4 * 14 ** 3
    dumps = []
    for run in range(2):
        d = str(tmp_path / ("out%d" % run))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--lattice", "14", "--steps", "50", "--warmup", "5", "--dump-outputs", d],
                           cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == out["steps_timed"] == out["steps_requested"] == 50 and len(out["window_ms"]) == 3
        per = sorted(w / k for w, k in zip(out["window_ms"], (20, 20, 10)))
        assert abs(out["ms_per_step"] - per[1]) < 1e-3 * per[1] + 1e-4      # (window_ms is rounded to 0.1 us)
        assert "also" not in out and "cpu_baseline" not in out
        a = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
        assert set(a) == {"positions", "velocities", "forces", "bead_index", "energy_terms", "virial", "kinetic"}
        assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
        assert a["positions"].shape == a["velocities"].shape == a["forces"].shape == (n, 3) and np.array_equal(a["bead_index"], np.arange(n))
        assert a["energy_terms"][6] == out["check"]["epot"] and a["kinetic"][0] == out["check"]["ekin"] and a["kinetic"].shape == (7,)
        assert np.abs(a["forces"]).max() > 0 and sum(v.nbytes for v in a.values()) <= 64 << 20
        dumps.append(a)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_nglfconstraint_between_processes():
    """constraints + barostat with the ranks in separate processes: velocity halo and the barostat's all-reduce (incl. the
    split molecules' partial sums) travel over the transport; both processes arrive at the oracle's box and pressure"""
    from test_oracle import CONSTRAINT_X
    from ddcmd_amd.deck import load_deck
    deck = os.path.join(ROOT, "tests", "golden", "lipid_deck")
    s = load_deck(os.path.join(deck, "object_nvt.data"), restart_file=os.path.join(deck, "relaxed", "restart"), extra_objects=CONSTRAINT_X)
    T, P0 = units_convert(310.0, "K"), units_convert(1.0, "bar")
    beta, tau = units_convert(3.0e-4, "1/bar") * 20.0, units_convert(1.0, "ps")
    o = pyoracle.Oracle(s, constraints=True)
    o.forces()
    o.group_temperature()
    os.environ["DDCMI_TEST_CONSTRAINT_X"] = CONSTRAINT_X
    try:
        recs = _run_ranks("lipid_npt", (2, 1, 1), 15, 5)
    finally:
        os.environ.pop("DDCMI_TEST_CONSTRAINT_X", None)
    for b in range(3):
        eo, vo, rko, _ = o.step_npt(5, T, P0, beta, tau, molecular=True)
        o.group_temperature()
        for r in recs:
            assert abs(r["traj"][b][0] - eo["total"]) < 1e-6 * abs(eo["total"])
            assert abs(r["traj"][b][1] - rko) < 1e-6 * rko
            assert np.abs(r["baro"][b][:3] - o.pmol).max() < 1e-8 * np.abs(o.pmol).max()
            assert np.abs(r["baro"][b][3:] - o.box).max() < 1e-10 * o.box.max()
    gid, _ = _merge(recs, "gid", "f")
    assert np.array_equal(gid, np.sort(s.gid))


def test_bench_world8_on_one_device():
    """the driver's N = 8 launch (2x2x2 bricks, 7 peers per rank) with all eight ranks on the one GPU of the test box over the
    host transport: rendezvous of eight processes, migration and halo messages between every pair of neighbours, the
    all-reduces; bench.py itself asserts that no bead is lost"""
    port = 29800 + os.getpid() % 90
    env = dict(os.environ)
    env.update({"DDCMI_BENCH_SINGLE_DEVICE": "1", "DDCMI_TRANSPORT": "host"})
    env.pop("DDCMI_RDZV_FILE", None); env.pop("DDCMI_RDZV_PORT", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "60", "--warmup", "20", "--lattice", "16"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["config"]["beads_total"] == 4 * 16 ** 3 and out["config"]["rebuilds_in_timed_region"] == 3
    assert "2x2x2" in out["config"]["parallelism"]
    # what the first contact with a real 8-GPU node should show at a glance: who met, who owns what, what travels per step, which RCCL
    c = out["comm"]
    assert c["ranks_met"] == 8 and len(c["beads_per_rank"]) == 8 and sum(c["beads_per_rank"]) == 4 * 16 ** 3
    assert c["peers_per_rank"] == [7] * 8 and all(b > 0 for b in c["halo_beads_sent_per_step"])
    assert c["halo_bytes_per_step_all_ranks"] == 24 * sum(c["halo_beads_sent_per_step"]) and c["rccl_version"].count(".") == 2
    p1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "60", "--warmup", "20", "--lattice", "16", "--no-cpu"],
                        cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p1.returncode == 0, p1.stderr[-3000:]
    one = json.loads([l for l in p1.stdout.splitlines() if l.startswith("{")][0])
    assert abs(out["check"]["epot"] - one["check"]["epot"]) < 1e-7 * abs(one["check"]["epot"])
    assert abs(out["check"]["ekin"] - one["check"]["ekin"]) < 1e-7 * abs(one["check"]["ekin"])


def test_decomposed_runs_repeat_bit_for_bit():
    """Migrants and halo beads arrive in the order atomics and messages deliver them; the in-cell order of a decomposed run
    is by gid, so that order does not reach the lists: two runs of the same launch agree in every bit, and so do two real
    processes over the host transport and two domains emulated inside one process (45 steps, three rebuilds, migration)"""
    from ddcmd_amd.martini import MartiniGroup
    a = _run_ranks("water", (2, 1, 1), 45, 15)
    b = _run_ranks("water", (2, 1, 1), 45, 15)
    for key in ("r", "v", "f"):
        ga, xa = _merge(a, "gid", key)
        gb, xb = _merge(b, "gid", key)
        assert np.array_equal(ga, gb) and np.array_equal(xa, xb), key
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["traj"], rb["traj"])
    s = ddcmd_amd.make_water_setup(12)
    g = MartiniGroup(s, (2, 1, 1))
    g.eval_forces()
    for _ in range(3):
        g.step(15)
    out = g.gather()
    g.close()
    ga, xa = _merge(a, "gid", "r")
    assert np.array_equal(out["gid"], ga)
    for c in range(3):
        assert np.array_equal(out["r"][c], xa[c]), "positions differ between the host transport and the in-process group"
    _, va = _merge(a, "gid", "v")
    for c in range(3):
        assert np.array_equal(out["v"][c], va[c])


def test_bench_rows_child_runs_eight_workloads_in_one_process():
    """bench.py --rows-only (what the N=1 headline run starts as a child process): eight workloads -- 1 M water, the 2 M bilayer four ways, three
    loopback bricks -- one after another in ONE process, every row without an error.  Round 6: rounds 3-5 registered the context object itself
    with hipHostRegister; contexts created and destroyed in one process at recycled heap addresses ended 5 of 12 such processes with a GPU
    memory fault, in a different workload every time (tools/rowsloop.sh).  One run here is a net, not a proof."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DDCMI_TRANSPORT", "DDCMI_RCCL_LOOPBACK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows-only"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert len(rows["also"]) == 8 and len(rows["pmc"]) == 8
    for r in rows["also"]:
        assert "error" not in r, r
        assert r["value"] > 0 and r["steps_timed"] >= 100 and r["roofline"]["frac"] > 0.1
    bricks = [r for r in rows["also"] if r["comm"]]
    assert len(bricks) == 3 and all(b["comm"]["preflight_rank0"]["stages_verified"] == 3 and b["comm"]["transport"] == "rccl-loopback" for b in bricks)


@pytest.mark.parametrize("workload,grid", [("water_drift", (2, 1, 1)), ("lipid_drift", (1, 1, 2)), ("water_drift", (2, 2, 2))])
def test_ranks_swing_between_empty_and_full_over_the_host_transport(workload, grid):
    """the migration soak between REAL processes: the count rounds with a rank that holds nothing, arrays that grow in the middle of a migration (keep[], round
    6), the bonded sums of a rank that has just been emptied (round 6).  Twelve rebuild periods, the all-reduced total energy and kinetic energy after every
    period against the same system on one domain in this process (the two runs part like any two trajectories: 1e-9 here), and the final bead set whole"""
    from ddcmd_amd.martini import MartiniHIP
    from drift_setup import drifting_setup
    s = drifting_setup(workload, grid)
    period = int(s.updateRate)
    nper = 12
    recs = _run_ranks(workload, grid, nper * period, period)
    one = MartiniHIP(s)
    one.eval_forces()
    thermo = any(int(t) == 1 for t in np.asarray(s.group_type).ravel())
    if thermo:
        one.group_temperatures()      # (the worker publishes the group temperature at the same points: tests/mp_worker.py)
    ref = []
    for _ in range(nper):
        one.step(period)
        e, vir, rk, _ = one.energies()
        ref.append([e["total"], rk] + list(vir))
        if thermo:
            one.group_temperatures()
    one.close()
    ref = np.array(ref)
    for r in recs:
        assert r["traj"].shape == ref.shape
        assert np.abs(r["traj"][:, :2] / ref[:, :2] - 1.0).max() < 1e-9, np.abs(r["traj"][:, :2] / ref[:, :2] - 1.0).max(axis=1)
        assert np.abs(r["traj"][:, 2:] - ref[:, 2:]).max() < 1e-8 * np.abs(ref[:, 2:]).max()
    gid = np.sort(np.concatenate([r["gid"] for r in recs]))
    assert np.array_equal(gid, np.sort(np.asarray(s.gid)))
    n_first, n_last = [int(r["nloc"][0]) for r in recs], [int(r["nloc"][1]) for r in recs]
    assert sum(n_first) == s.natoms == sum(n_last) and n_first != n_last, (n_first, n_last)

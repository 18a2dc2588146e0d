"""The cases of tests/test_gpu_step_plan.py: which path a configuration's force evaluations take (ddcmi_debug_step_plan,
include/ddcmi_test.h), step by step.

A case is {"env": switches set before the context is made, "make": () -> model, "run": [steps per call], "dt": [dt per call or None],
"want": one plan per force evaluation}.  Every case evaluates forces once (which builds the list) and then steps; the list is rebuilt
when the loop count reaches a multiple of UPDATE = 4.  A plan is (halo, fused, lean, reduction), see ddcmd_amd.martini.MartiniHIP.step_plan.

The expected plans are written out from the conditions of the code as it was before the plan existed (launch_forces' ladder, lean_capable,
self_images, fuse_ok, step_post), not from plan_forces:
  * the last step of every call cannot fuse: no step follows it that would own the FRONT kick and drift;
  * the evaluation directly behind a rebuild -- ddcmi_eval_forces' first, a step whose loop count is a multiple of UPDATE -- finds the
    images and the halo fresh and refreshes nothing.  Where the pair kernel finds the images at their owners the mode says so on every
    evaluation: it names where the kernel reads, and nothing is ever refreshed;
  * a fused step that is not lean refreshes the images (or packs the next messages) in its reduction launch, so the step behind it
    refreshes nothing either;
  * self_images asks lean_capable: DDCMI_NO_LEAN_STEP takes the images at their owners away too, and without them no step is lean, so
    DDCMI_NO_SELF_IMAGES and DDCMI_NO_LEAN_STEP give the same plans."""
import os
import numpy as np

UPDATE = 4
NONE, OWNERS, UPDATE_LAUNCH, DIRECT, OVERLAP, IMAGES = range(6)      # halo
R_NONE, R_PLAIN, R_IMAGES, R_PACK = range(4)                         # reduction
SWITCHES = ("DDCMI_NO_LEAN_STEP", "DDCMI_NO_SELF_IMAGES", "DDCMI_NO_FUSED_STEP", "DDCMI_FORCE_LEVEL_TABLE", "DDCMI_NO_DIRECT_HALO",
            "DDCMI_HALO_OVERLAP", "DDCMI_RCCL_LOOPBACK")
LIPID = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lipid_deck")


def water(**kw):
    from ddcmd_amd.synth import make_water_setup
    return make_water_setup(12, update_rate=kw.pop("update_rate", UPDATE), **kw)      # 6912 beads


def lipid(exclude=0, extra=None):
    from ddcmd_amd.deck import load_deck
    s = load_deck(os.path.join(LIPID, "object_nvt.data"), restart_file=os.path.join(LIPID, "relaxed", "restart"), extra_objects=extra)
    s.updateRate = UPDATE
    s.excludePotentialTerm = exclude
    return s


def groups(s, kinds, interval=1, tau_ps=(1.0, 2.0)):
    from ddcmd_amd.deck import units_convert
    s.ngroup = len(kinds)
    s.group_name = ["g%d" % g for g in range(s.ngroup)]
    s.group = (np.arange(s.natoms) % s.ngroup).astype(np.int32)
    s.group_type = np.array(kinds, np.int32)
    s.group_Teq = np.array([units_convert(300.0 + 50.0 * g, "K") for g in range(s.ngroup)])
    s.group_tau = np.array([units_convert(tau_ps[g], "ps") for g in range(s.ngroup)])
    s.group_interval = np.full(s.ngroup, interval, np.int32)
    return s


def restrained(s):
    """every 97th bead held at its own place in all three directions"""
    from restraint_systems import KB_UNIT
    bead = np.arange(0, s.natoms, 97)
    L = np.array([s.h[0], s.h[4], s.h[8]])
    s.nrest, s.rest_origin = len(bead), 0
    s.rest_gid = np.asarray(s.gid, np.uint64)[bead].copy()
    s.rest_fc = np.ones((len(bead), 3), np.int32)
    s.rest_r0 = np.ascontiguousarray(np.stack([s.rx[bead], s.ry[bead], s.rz[bead]], 1) / L + 0.5)
    s.rest_kb = np.full(len(bead), 200.0 * KB_UNIT)
    return s


def barostat(s):
    from ddcmd_amd.deck import units_convert
    s.npt_T, s.npt_P0 = units_convert(310.0, "K"), units_convert(1.0, "bar")
    s.npt_beta, s.npt_tau = units_convert(3.0e-4, "1/bar"), units_convert(1.0, "ps")
    return s


def single(s, **kw):
    from ddcmd_amd.martini import MartiniHIP
    return MartiniHIP(s, test_api=True, **kw)


def constrained_lipid():
    from test_oracle import CONSTRAINT_X
    return single(lipid(extra=CONSTRAINT_X), constraints=True)


def loopback(s):
    """one brick whose periodic neighbours are reached through RCCL (DDCMI_RCCL_LOOPBACK=1 in the case's env)"""
    import ctypes
    from ddcmd_amd.martini import MartiniRank, _declare_domains
    m = MartiniRank(s, np.arange(s.natoms), test_api=True)
    _declare_domains(m.lib)
    buf = ctypes.create_string_buffer(128)
    assert m.lib.ddcmi_comm_unique_id(buf) == 0
    m.comm_init(0, 1, buf.raw, (1, 1, 1))
    m.upload_local()
    return m


def group2(s):
    from ddcmd_amd.martini import MartiniGroup
    return MartiniGroup(s, (2, 1, 1))


def steps(first, steady, rebuilt=None, last=None, n=7):
    """the plans of ddcmi_eval_forces + one call of n steps (loop counts 1 ... n): `first` for the evaluation, `steady` for a step,
    `rebuilt` (default: steady) for a step behind a rebuild, `last` for the call's last step"""
    out = [first]
    for loop in range(1, n + 1):
        out.append((last or steady) if loop == n else (rebuilt or steady) if loop % UPDATE == 0 else steady)
    return out


LEAN = (OWNERS, 1, 1, R_NONE)
OWNERS_SPLIT = (OWNERS, 0, 0, R_NONE)
SPLIT, SPLIT_FRESH = (IMAGES, 0, 0, R_NONE), (NONE, 0, 0, R_NONE)
FUSED_IMG = (NONE, 1, 0, R_IMAGES)      # (the reduction launch in front refreshed the images)
# fused, not lean, a single domain: the first step refreshes the images itself (ddcmi_eval_forces' launch has no job on the side), every later one finds them fresh
NOT_LEAN = [SPLIT_FRESH, (IMAGES, 1, 0, R_IMAGES)] + [FUSED_IMG] * 5 + [SPLIT_FRESH]
SPLIT_ALL = steps(SPLIT_FRESH, SPLIT, SPLIT_FRESH, SPLIT)
RUN7 = {"run": [7], "dt": [None]}

CASES = {
    "water_free": dict(RUN7, env={}, make=lambda: single(water()), want=steps(OWNERS_SPLIT, LEAN, last=OWNERS_SPLIT)),
    "water_one_berendsen": dict(RUN7, env={}, make=lambda: single(water(thermostat="berendsen")), want=steps(OWNERS_SPLIT, LEAN, last=OWNERS_SPLIT)),
    # both groups scale when the loop count is a multiple of 3, by different factors (different tau): those steps take the split kernels
    "water_two_berendsen": dict(RUN7, env={}, make=lambda: single(groups(water(), [1, 1], interval=3)),
                                want=[OWNERS_SPLIT, LEAN, LEAN, OWNERS_SPLIT, LEAN, LEAN, OWNERS_SPLIT, OWNERS_SPLIT]),
    "water_langevin": dict(RUN7, env={}, make=lambda: single(groups(water(), [0, 2])), want=SPLIT_ALL),
    # (no rebuild is asked for within seven steps at 50 K: the displacement check runs on the host before every step)
    "water_update_rate_0": dict(RUN7, env={}, make=lambda: single(water(update_rate=0)), want=NOT_LEAN),
    "water_restraints": dict(RUN7, env={}, make=lambda: single(restrained(water())), want=NOT_LEAN),
    "water_barostat": dict(RUN7, env={}, make=lambda: single(barostat(water())), want=SPLIT_ALL),
    "lipid": dict(RUN7, env={}, make=lambda: single(lipid()), want=steps(OWNERS_SPLIT, LEAN, last=OWNERS_SPLIT)),
    "lipid_constraints": dict(RUN7, env={}, make=constrained_lipid, want=SPLIT_ALL),
    "lipid_bit_128": dict(RUN7, env={}, make=lambda: single(lipid(exclude=128)), want=SPLIT_ALL),
    "no_lean_step": dict(RUN7, env={"DDCMI_NO_LEAN_STEP": "1"}, make=lambda: single(water()), want=NOT_LEAN),
    "no_self_images": dict(RUN7, env={"DDCMI_NO_SELF_IMAGES": "1"}, make=lambda: single(water()), want=NOT_LEAN),
    "force_level_table": dict(RUN7, env={"DDCMI_FORCE_LEVEL_TABLE": "1"}, make=lambda: single(water()), want=steps(OWNERS_SPLIT, LEAN, last=OWNERS_SPLIT)),
    # a fresh process: fuse_ok reads the switch once per process
    "no_fused_step": dict(RUN7, env={"DDCMI_NO_FUSED_STEP": "1"}, make=lambda: single(water()), want=steps(OWNERS_SPLIT, OWNERS_SPLIT), fresh_process=True),
    "loopback": dict(RUN7, env={"DDCMI_RCCL_LOOPBACK": "1"}, make=lambda: loopback(water()),
                     want=steps((NONE, 0, 0, R_NONE), (DIRECT, 1, 1, R_NONE), (NONE, 1, 1, R_NONE), (DIRECT, 0, 0, R_NONE))),
    "loopback_no_direct": dict(RUN7, env={"DDCMI_RCCL_LOOPBACK": "1", "DDCMI_NO_DIRECT_HALO": "1"}, make=lambda: loopback(water()),
                               want=steps((NONE, 0, 0, R_NONE), (UPDATE_LAUNCH, 1, 0, R_PACK), (NONE, 1, 0, R_PACK), (UPDATE_LAUNCH, 0, 0, R_NONE))),
    "loopback_overlap": dict(RUN7, env={"DDCMI_RCCL_LOOPBACK": "1", "DDCMI_HALO_OVERLAP": "1"}, make=lambda: loopback(water()),
                             want=steps((NONE, 0, 0, R_NONE), (OVERLAP, 1, 0, R_PLAIN), (NONE, 1, 0, R_PLAIN), (OVERLAP, 0, 0, R_NONE))),
    # the ring of the displacement bound holds LEAN_W = 32 words: the 32nd lean step since the rebuild is the last one, its flush follows
    # it, and the steps up to the next rebuild run fused with the plain reduction launch (only the last 16 plans are kept)
    "lean_ring_full": dict(env={}, make=lambda: single(water(update_rate=40)), run=[36], dt=[None],
                           want=[None] * 21 + [LEAN] * 12 + [(OWNERS, 1, 0, R_PLAIN)] * 3 + [OWNERS_SPLIT]),
    # another dt ends the lean run: the ring's words are speeds times the dt of the steps that filed them
    "dt_change": dict(env={}, make=lambda: single(water(update_rate=40)), run=[3, 3], dt=[None, 0.5],
                      want=[OWNERS_SPLIT, LEAN, LEAN, OWNERS_SPLIT, (OWNERS, 1, 0, R_PLAIN), (OWNERS, 1, 0, R_PLAIN), OWNERS_SPLIT]),
    # two domains in one process: the driver exchanges, the update launch places the received beads; never fused
    "group_2x1x1": dict(RUN7, env={}, make=lambda: group2(water()), want=SPLIT_ALL),
}


def run_case(name, plans=True):
    """runs the case in this process (the caller has set its env) and returns [(halo, fused, lean, reduction, level, fixed, hdisp,
    direct)] per evaluation, None where the plan has left the ring; plans=False: only runs it"""
    c = CASES[name]
    m = c["make"]()
    m.eval_forces()
    for n, dt in zip(c["run"], c["dt"]):
        m.step(n, dt=None if dt is None else dt * m.s.dt)
    ranks = getattr(m, "ranks", [m])
    out = []
    if plans:
        nev = 1 + sum(c["run"])
        for r in ranks:
            got = [r.step_plan(nev - 1 - k) if nev - 1 - k < 16 else None for k in range(nev)]
            out.append([None if p is None else (p["halo"], p["fused"], p["lean"], p["reduction"], p["level_table"], p["fixed_layout"], p["halo_disp"],
                                                p["direct"]) for p in got])
    if hasattr(m, "close"):
        m.close()
    else:
        for r in ranks:
            r.close()
    return out

"""Systems and runs of the FORCE_AVERAGE tests (helper module, no tests in here): the force-free gas of tests/restraint_systems.py at
chosen bead counts with a few restrained beads (so that forces are not zero), tracked lists of every kind the interface admits, the
host's running sums from downloads, and the twin run of the "nothing changes" check."""
import numpy as np

import restraint_systems as R
from ddcmd_amd.synth import Setup

WHATS = ("force", "velocity", "position")
KEY = {"force": "f", "velocity": "v", "position": "r"}
SHIFT = np.uint64(32)
SCHEDULE = (0, 5, 10, 3, 12, 8, 7)      # steps in front of each of the 7 accumulations: 45 in all, across rebuilds every 10 or 20


def gas(n, update_rate=10, seed=20261021, restrained=8):
    """n beads (up to 2000) on the jittered lattice of the gas, speeds up to 0.12 A per step, gids (k + 5) << 32 in an order unrelated to
    the slots, min(n, restrained) beads on harmonic restraints"""
    rng = np.random.RandomState(seed + n)
    s = Setup()
    R._forcefield(s, update_rate)
    L = np.array(R.BOX_A)
    dims = np.array([10, 10, 20])
    k = rng.permutation(int(dims.prod()))[:n]
    ijk = np.stack([k % 10, (k // 10) % 10, k // 100], 1)
    r = -0.5 * L + (ijk + 0.5) * L / dims + rng.uniform(-0.3, 0.3, (n, 3)) * L / dims
    v = rng.uniform(-0.12, 0.12, (n, 3)) * R.ANG / s.dt
    R._finish(s, r, v, rng)
    s.gid = ((rng.permutation(n) + 5).astype(np.uint64) << SHIFT)
    nr = min(n, restrained)
    bead = rng.permutation(n)[:nr]
    R._set_restraints(s, bead, np.ones((nr, 3), int), r[bead] - rng.uniform(1.0, 3.0, (nr, 3)), rng.uniform(50.0, 500.0, nr))
    s.name = "track_gas%d" % n
    return s


def tracked_list(s, nl, seed=3):
    """nl gids: the smallest and the largest gid of the system first where there is room, then a shuffled mix of present gids, gids inside
    the range that no bead carries ((k << 32) + 1), gids just outside the range on both sides (below 2^32 among them), and duplicates of
    entries already listed; returned with the mask of the entries some bead carries"""
    rng = np.random.RandomState(seed + nl + len(s.gid))
    gid = np.asarray(s.gid, np.uint64)
    lo, hi = gid.min(), gid.max()
    with np.errstate(over="ignore"):      # (gid 0 - 1 wraps to the largest gid: legal, and above the range)
        absent = np.concatenate([gid[rng.permutation(len(gid))[:max(1, nl // 8)]] + np.uint64(1),
                                 np.array([lo - np.uint64(1), hi + np.uint64(1), np.uint64(7), lo - (np.uint64(1) << SHIFT), hi + (np.uint64(1) << SHIFT)], np.uint64)])
    pool = np.concatenate([gid[rng.permutation(len(gid))], absent])
    out = [lo, hi][:nl]
    while len(out) < nl:
        take = pool[rng.permutation(len(pool))[:nl - len(out)]]
        out.extend(take.tolist())
        if len(out) < nl:      # more ids than the pool holds: duplicates and further absent gids
            out.extend((take[:max(1, (nl - len(out)) // 2)]).tolist())
            extra = (np.arange(nl - len(out), dtype=np.uint64) << SHIFT) + np.uint64(3)
            out.extend(extra.tolist())
    out = np.array(out[:nl], np.uint64)
    if nl >= 4:
        out[nl // 2] = out[0]      # a duplicate of a present gid, and one of whatever stands last
        out[nl // 3] = out[-1]
        out = out[::-1].copy() if nl % 2 else out[rng.permutation(nl)]      # reverse or shuffled order
    return out, np.isin(out, gid)


def index_of(s, gids):
    """setup index of every listed gid, -1 where no bead carries it"""
    gid = np.asarray(s.gid, np.uint64)
    order = np.argsort(gid)
    pos = np.minimum(np.searchsorted(gid[order], gids), len(gid) - 1)
    return np.where(gid[order][pos] == gids, order[pos], -1)


def values(d, what, idx, dtype=np.float64):
    """[n, 3] of a download's arrays at the setup indices idx; zero rows for -1"""
    a = np.stack([np.asarray(c) for c in d[KEY[what]]], 1).astype(dtype)
    return np.where((idx >= 0)[:, None], a[np.maximum(idx, 0)], dtype(0))


def twin_run(s, track, gids=None):
    """eval, then five calls of the step with an accumulation in front of each (track), a read with reset in the middle, 20 further
    steps: the energies behind every call, the download at the end, the step plans that occurred"""
    from ddcmd_amd.martini import MartiniHIP
    m = MartiniHIP(s, test_api=True)
    try:
        m.eval_forces()
        if track:
            m.track_set(gids)
        en, plans, reads = [], set(), []
        for it, k in enumerate((3, 7, 10, 5, 20)):
            if track:
                m.track_accumulate("force" if it < 3 else "position")
            m.step(k)
            p = m.step_plan(1) if k > 1 else m.step_plan()      # (the last step of a call is never fused: the one before it)
            plans.add((p["fused"], p["lean"]))
            e, vir, rk, tion = m.energies()
            en.append(np.concatenate([[e[q] for q in sorted(e)], vir, [rk], tion]))
            if track and it == 2:
                reads.append(m.track_read(reset=True))
        if track:
            reads.append(m.track_read())
        m.step(20)
        e, vir, rk, tion = m.energies()
        en.append(np.concatenate([[e[q] for q in sorted(e)], vir, [rk], tion]))
        d = m.download()
        return {"en": np.array(en), "r": np.stack(d["r"]), "v": np.stack(d["v"]), "f": np.stack(d["f"]), "plans": np.array(sorted(plans)),
                "hits": np.array([h for _, h in reads])}
    finally:
        m.close()

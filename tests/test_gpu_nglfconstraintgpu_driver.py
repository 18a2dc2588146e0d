"""GPU tests (-m gpu) of the NGLFCONSTRAINTGPU family through the ddcmi_md driver, on the relaxed lipid deck with the constraint lists of
tests/nglfconstraintgpu_systems.CONSTRAINT_X (what test_gpu_driver.py hands the driver through -x), the barostat on, 20 steps with a
rebuild at 10 and 20, a checkpoint at 20."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import nglfconstraintgpu_systems as N
import pyoracle
from ddcmd_amd.deck import load_deck, units_convert
from ranks import EXE, ROOT, driver_ranks

pytestmark = pytest.mark.gpu
DECK = os.path.join(N.LIPID, "object_nvt.data")
RESTART = os.path.join(N.LIPID, "relaxed", "restart")
RUN = ("simulate SIMULATE { deltaloop = 20; maxloop = 20; printrate = 10; checkpointrate = 20; } system SYSTEM { nConstraints = 1000; } "
       "printinfo PRINTINFO { printMolecularPressure = 1; } ")
SNAP = "snapshot.%012d" % 20


def extra(name, group, isotropic=0):
    return N.CONSTRAINT_X + group + N.integrator(name, isotropic) + RUN


def run(tmp_path, tag, x, world=1):
    """the driver in a directory of its own: (data, restart, atoms file as bytes; stdout; stderr of rank 0).  The atoms file's header carries
    the wall-clock second it was written in (create_time, collection_write.c): that one value is blanked, every other byte is compared"""
    d = tmp_path / tag
    d.mkdir()
    args = ["-o", DECK, "-r", RESTART, "-d", "data", "-x", x]
    if world == 1:
        out = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300, cwd=str(d))
        assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
        so, se = out.stdout, out.stderr
    else:
        res = driver_ranks(world, args, str(d))
        for rc, o, er in res:
            assert rc == 0, o[-1000:] + er[-2000:]
        so, se = res[0][1], res[0][2]
    files = [re.sub(rb"create_time=[-0-9:]{19};", b"create_time=;", open(str(d / f), "rb").read())
             for f in ("data", os.path.join(SNAP, "restart"), os.path.join(SNAP, "atoms#000000"))]
    assert files[2].count(b"create_time=;") == 1
    return files, so, se, d


def rows(data):
    return np.array([[float(v) for v in l.split()] for l in data.decode().splitlines() if l.strip() and not l.startswith("#")])


def test_nglfconstraintgpu_is_nglfconstraint_with_free_groups(tmp_path):
    """(a) FREE groups, isotropic = 0: data file and checkpoint of NGLFCONSTRAINTGPU are NGLFCONSTRAINT's, byte for byte; (b) the same deck
    with a LANGEVIN group: the type runs it as FREE -- the same bytes again -- and says so once on stderr"""
    a, _, se_a, _ = run(tmp_path, "nglfconstraint", extra("NGLFCONSTRAINT", N.FREE_GROUP))
    b, _, se_b, _ = run(tmp_path, "gpu_free", extra("NGLFCONSTRAINTGPU", N.FREE_GROUP))
    assert a == b and rows(a[0]).shape[0] == 3
    assert "runs as" not in se_a and "runs as" not in se_b
    assert abs(rows(a[0])[-1, 8] / rows(a[0])[0, 8] - 1) > 1e-6          # the barostat moved the box
    c, _, se_c, _ = run(tmp_path, "gpu_langevin", extra("NGLFCONSTRAINTGPU", N.LANGEVIN_GROUP))
    assert c == b
    assert se_c.count("ddcmi_md: INTEGRATOR type NGLFCONSTRAINTGPU: GROUP group (LANGEVIN) runs as FREE\n") == 1 and se_c.count("runs as") == 1


def test_the_two_langevin_names_are_one_path_and_follow_the_oracle(tmp_path):
    """(c) NGLFCONSTRAINTGPULANGEVIN and ...LCG64: the same bytes; the checkpoint's LCG64 fields are the oracle's advanced states, the data
    file's energy, temperature, molecular pressure and box columns the oracle's within the bounds of test_gpu_driver.py's NGLFGPULANGEVIN
    and NGLFCONSTRAINT tests (1e-6 relative; the box 1e-7 A)"""
    x = extra("NGLFCONSTRAINTGPULANGEVIN", N.LANGEVIN_GROUP, isotropic=1)
    a, _, se, d = run(tmp_path, "langevin", x)
    b, _, _, _ = run(tmp_path, "lcg64", extra("NGLFCONSTRAINTGPULANGEVINLCG64", N.LANGEVIN_GROUP, isotropic=1))
    assert a == b and "runs as" not in se
    s = load_deck(DECK, restart_file=RESTART, extra_objects=x)
    assert s.integrator_type == "NGLFCONSTRAINTGPULANGEVIN" and s.npt_isotropic == 1 and s.nresicons == 5
    o = pyoracle.Oracle(N.as_run(s), constraints=True)
    assert o.lcg is not None
    e, vir = o.forces()
    rk, tion = o.kinetic()
    r = rows(a[0])
    n = s.natoms
    cE, cT, cP, cL = (units_convert(1, None, u) for u in ("kJ/mol", "K", "bar", "Angstrom"))
    mol = (np.asarray(s.gid) >> np.uint64(32)).astype(np.int64)
    mass = np.asarray(s.mass)[np.asarray(s.species)]
    first = np.zeros(mol.max() + 1, np.int64)
    first[mol[::-1]] = np.arange(n - 1, -1, -1)
    assert r.shape[0] == 3
    for k, row in enumerate(r):
        info = o.energy_info(e["total"], rk, vir, tion)
        # molecularPressure.c:22-67, as test_ddcmi_md_molecular_pressure forms it
        L = o.box
        pos, f = np.stack([o.rx, o.ry, o.rz], 1), np.stack([o.fx, o.fy, o.fz], 1)
        dd = pos - pos[first[mol]]
        dd -= L * np.rint(dd / L)
        M = np.bincount(mol, weights=mass)
        R = np.stack([np.bincount(mol, weights=mass * dd[:, c]) for c in range(3)], 1) / M[:, None]
        dd -= R[mol]
        T = 2.0 * rk / (3.0 * n - s.nConstraints)
        pmol = np.mean((np.array(vir[:3]) - np.sum(dd * f, axis=0) + len(M) * T) / float(np.prod(L)))
        assert int(row[0]) == 10 * k
        assert abs(row[3] - cE * rk / n) < 1e-6 * abs(row[3]) + 1e-9, k
        assert abs(row[4] - cE * e["total"] / n) < 1e-6 * abs(row[4]) + 1e-9, k
        assert abs(row[5] - cT * info["temperature"]) < 1e-6 * row[5], k
        assert abs(row[6] - cP * pmol) < 1e-6 * abs(cP * pmol) + 1e-6, (k, row[6], cP * pmol)
        assert np.abs(row[8:11] - cL * L).max() < 1e-7, k
        assert abs(row[8] / r[0, 8] - row[10] / r[0, 10]) < 1e-9          # isotropic: one scale factor
        if k < 2:
            e, vir, rk, tion = o.step_npt(10, s.npt_T, s.npt_P0, s.npt_beta, s.npt_tau, molecular=True)
    assert abs(r[-1, 8] / r[0, 8] - 1) > 1e-6
    s1 = load_deck(DECK, restart_file=str(d / SNAP / "restart"), extra_objects=x)
    assert s1.loop == 20 and s1.lcg_from_file == 1
    assert np.array_equal(s1.lcg64["state"], o.lcg["state"]) and np.array_equal(s1.lcg64["prime"], o.lcg["prime"]) and np.array_equal(s1.lcg64["multID"], o.lcg["multID"])
    assert (s1.lcg64["state"] != s.lcg64["state"]).all()
    assert np.abs(s1.vx - o.vx).max() < 1e-6 * np.abs(o.vx).max()


def test_group_zero_must_be_langevin_in_the_driver(tmp_path):
    out = subprocess.run([EXE, "-o", DECK, "-r", RESTART, "-d", str(tmp_path / "d"), "-x", extra("NGLFCONSTRAINTGPULANGEVIN", N.FREE_GROUP)],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert out.returncode != 0 and "NGLFCONSTRAINTGPULANGEVIN needs the first GROUP to be of type LANGEVIN" in out.stderr
    out = subprocess.run([EXE, "-o", DECK, "-r", RESTART, "-d", str(tmp_path / "d"), "-x", "nglf INTEGRATOR { type = NGLFRATTLE; }"],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert out.returncode != 0 and "NGLFRATTLE is not on this path (NGLF, NVTGLF, NGLFGPU, NGLFHIP, NGLFGPULANGEVIN, NGLFCONSTRAINT, NGLFCONSTRAINTGPU, NGLFCONSTRAINTGPULANGEVIN, NGLFCONSTRAINTGPULANGEVINLCG64 are)" in out.stderr


def test_lcg64_name_on_two_ranks(tmp_path):
    """(d) ...LCG64 on two ranks (host transport, one device) against one rank, held to what test_ddcmi_md_nglfconstraint_on_two_ranks holds
    its pair to: the box columns 1e-9, every column 1e-7 of the largest; the streams migrate with their beads"""
    x = extra("NGLFCONSTRAINTGPULANGEVINLCG64", N.LANGEVIN_GROUP)
    one, _, _, d1 = run(tmp_path, "one", x)
    two, so, _, d2 = run(tmp_path, "two", x, world=2)
    assert "2 ranks on a" in so
    a, b = rows(one[0]), rows(two[0])
    assert a.shape == b.shape and a.shape[0] == 3
    assert np.abs(a[:, 8:] - b[:, 8:]).max() < 1e-9 * a[:, 8:].max()
    assert np.abs(a - b).max() <= 1e-7 * np.abs(a).max()
    s1 = load_deck(DECK, restart_file=str(d1 / SNAP / "restart"), extra_objects=x)
    s2 = load_deck(DECK, restart_file=str(d2 / SNAP / "restart"), extra_objects=x)
    i1, i2 = np.argsort(s1.gid), np.argsort(s2.gid)
    assert np.array_equal(s1.gid[i1], s2.gid[i2]) and (s1.lcg64[i1] == s2.lcg64[i2]).all()


def test_the_references_deck_line_runs(tmp_path):
    """(e) the reference's shipped waterbox deck with its line 69 -- INTEGRATOR type=NGLFCONSTRAINTGPULANGEVIN, isotropic -- selected through
    -x: 20 steps, exit 0"""
    cwd = str(tmp_path / "waterbox")
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "ref_waterbox"), cwd)
    line = [l for l in open(os.path.join(cwd, "object.data")).read().splitlines() if "NGLFCONSTRAINTGPULANGEVIN;" in l]
    assert len(line) == 1 and line[0].startswith("//")
    x = line[0][2:] + " simulate SIMULATE { deltaloop = 20; printrate = 10; }"
    out = subprocess.run([EXE, "-o", "object.data", "-d", "data", "-x", x], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
    r = rows(open(os.path.join(cwd, "data"), "rb").read())
    assert r.shape[0] == 3 and int(r[-1, 0]) == 20 and np.isfinite(r).all() and r[-1, 5] > 100.0      # the lattice start heats up, as under the shipped line
    assert abs(r[-1, 8] / r[0, 8] - r[-1, 10] / r[0, 10]) < 1e-9 and "runs as" not in out.stderr

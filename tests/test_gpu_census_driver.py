"""GPU tests (-m gpu) of the ANALYSIS types vcmWrite and zdensity in the ddcmi_md driver: vcm.data in the run directory (one header
at init, one line per output), snapshot.<loop>/zden.dat, both held against the restatements of vcmWrite.c / zdensity.c applied to the
restart state the driver writes at the same loop; one rank against two; a mixed list against its members alone."""
import glob
import os

import numpy as np
import pytest

from ddcmd_amd.analysis import VcmWrite, ZDensity, parse_vcm_output
from ddcmd_amd.deck import load_deck, units_convert
from ranks import GOLDEN, copy_deck, run_driver, tree_files

pytestmark = pytest.mark.gpu
NZ = 16
VCM = "vcm ANALYSIS { type = vcmWrite; outputrate = 10; }\n"
ZDEN = "zden ANALYSIS { type = zdensity; outputrate = 10; nz = %d; }\n" % NZ
SIM = "simulate SIMULATE { %sdeltaloop = 20; maxloop = 20; printrate = 5; snapshotrate = 10; checkpointrate = 100000; }\n"


def _restated_vcm(s):
    """vcmWrite_output's loop over a loaded state, float64 in bead order: (mv[ncl, 3], m[ncl])"""
    ng, ns = max(1, s.ngroup), s.nspecies
    mv, m = np.zeros((1 + ng + ns, 3)), np.zeros(1 + ng + ns)
    v = np.stack([s.vx, s.vy, s.vz], axis=1)
    for i in range(s.natoms):
        mass = s.mass[s.species[i]]
        for c in (0, 1 + s.group[i], 1 + ng + s.species[i]):
            mv[c] += mass * v[i]
            m[c] += mass
    return mv, m


def test_driver_writes_vcm_data_and_zden_files(tmp_path):
    d = copy_deck(tmp_path, "water_deck", "with")
    (out,) = run_driver(d, SIM % "analysis = vcm zden; " + VCM + ZDEN)
    d0 = copy_deck(tmp_path, "water_deck", "without")
    run_driver(d0, SIM % "")
    assert open(str(d / "data"), "rb").read() == open(str(d0 / "data"), "rb").read()      # the analyses change nothing of the run
    assert not [l for l in out.stderr.splitlines() if "not supported" in l]
    txt = open(str(d / "vcm.data")).read()
    lines = txt.splitlines()
    assert len(lines) == 3 and txt.endswith("\n")
    s0 = load_deck(str(d / "object.data"))
    an = VcmWrite(s0.group_name, s0.species_name)
    assert lines[0] + "\n" == an.header() and len(s0.group_name) == 2 and len(s0.species_name) == 2
    loop, time, vcm = parse_vcm_output(txt)
    assert list(loop) == [10, 20] and vcm.shape == (2, 5, 3)
    zan = ZDensity(NZ)
    for k, lp in enumerate((10, 20)):
        snap = "snapshot.%012d" % lp
        s = load_deck(str(d / "object.data"), restart_file=str(d / snap / "restart"))
        assert s.loop == lp and s.natoms == s0.natoms
        assert abs(time[k] - units_convert(s.time, None, "fs")) <= 2e-6      # (both files print the time with six decimals)
        # the restart prints 14 digits of every velocity: the restated centre-of-mass velocities carry a relative error far below
        # the seven digits of %16.6e; a value on a rounding edge may still differ by one unit of the last printed digit
        want_line = an.line(lp, s.time, *_restated_vcm(s))
        _, _, want = parse_vcm_output(want_line)
        print(lp, np.abs(vcm[k] / want[0] - 1).max())
        assert np.allclose(vcm[k], want[0], rtol=1.01e-6, atol=0)
        assert lines[1 + k][:12] == "%12d" % lp and len(lines[1 + k]) == len(want_line) - 1
        # zden.dat: nz lines, fractional bin centres, the beads all counted, the bins those of the restart's positions
        ztxt = open(str(d / snap / "zden.dat")).read()
        rows = np.array([[float(x) for x in ln.split()] for ln in ztxt.splitlines()])
        assert rows.shape == (NZ, 3) and rows[:, 2].sum() == s.natoms
        assert np.allclose(rows[:, 0], (np.arange(NZ) + 0.5) / NZ, atol=1e-6)
        L = s.h[8]
        t = s.rz * (NZ / L) - (L * -0.5) * (NZ / L)
        ig = np.trunc(t).astype(np.int64)
        counts = np.bincount(np.where((ig < 0) | (ig >= NZ), NZ - 1, ig), minlength=NZ)
        # (14 printed digits of z: a bead within 1e-12 of an edge could change bin between the device's z and the file's; none does here)
        assert np.abs(t - np.rint(t)).min() > 1e-9
        assert ztxt == zan.output_text(counts.astype(np.float64), (s.h[0], s.h[4], s.h[8]))


def test_driver_two_ranks_write_the_same_files(tmp_path):
    d1 = copy_deck(tmp_path, "water_deck", "one")
    run_driver(d1, SIM % "analysis = vcm zden; " + VCM + ZDEN)
    d2 = copy_deck(tmp_path, "water_deck", "two")
    outs = run_driver(d2, SIM % "analysis = vcm zden; " + VCM + ZDEN, world=2)
    assert not [l for o in outs for l in o[1].splitlines() if "not supported" in l]
    for loop in (10, 20):
        a = open(str(d1 / ("snapshot.%012d" % loop) / "zden.dat"), "rb").read()
        b = open(str(d2 / ("snapshot.%012d" % loop) / "zden.dat"), "rb").read()
        assert len(a) > 0 and a == b      # integer counts: any split over ranks gives the same sums
    assert open(str(d1 / "vcm.data"), "rb").read() == open(str(d2 / "vcm.data"), "rb").read()


def test_driver_mixed_list_gives_every_file_each_analysis_gives_alone(tmp_path):
    sim = "simulate SIMULATE { %sdeltaloop = 40; maxloop = 40; printrate = 5; snapshotrate = 100000; checkpointrate = 100000; }\n"
    vaf = "vaf ANALYSIS { type = VELOCITYAUTOCORRELATION; eval_rate = 5; length = 4; outputrate = 20; }\n"
    rdf = "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 20; delta_r = 0.1 Angstrom; length = 100; }\n"
    objs = {"vaf": vaf, "vcm": VCM, "rdf": rdf, "zden": ZDEN}
    mixed = copy_deck(tmp_path, "water_deck", "mixed")
    (out,) = run_driver(mixed, sim % "analysis = vaf vcm rdf zden; " + "".join(objs.values()))
    assert not [l for l in out.stderr.splitlines() if "not supported" in l]
    golden = set(tree_files(os.path.join(GOLDEN, "water_deck")))
    seen = set()
    for name, obj in objs.items():
        d = copy_deck(tmp_path, "water_deck", name)
        run_driver(d, sim % ("analysis = %s; " % name) + obj)
        written = sorted(set(tree_files(d)) - golden - {"data"})
        assert written, name
        for f in written:
            assert open(str(d / f), "rb").read() == open(str(mixed / f), "rb").read(), f
        assert open(str(d / "data"), "rb").read() == open(str(mixed / "data"), "rb").read()
        seen |= set(written)
    assert seen == set(tree_files(mixed)) - golden - {"data"}      # and the mixed run writes nothing else
    assert "vcm.data" in seen and "snapshot.%012d/zden.dat" % 40 in seen and "snapshot.%012d/vaf.dat" % 20 in seen

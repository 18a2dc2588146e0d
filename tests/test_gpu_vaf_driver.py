"""GPU tests (-m gpu) of ANALYSIS VELOCITYAUTOCORRELATION in the ddcmi_md driver: the startup evaluation sets the first origin, a
sample at every eval, accumulate / re-origin / sample 0 on reaching length, snapshot.<loop>/vaf.dat as velocityAutocorrelation_output
writes it (gate, header, the one-group / one-species rule, units, member counts) -- held against analysis.VelocityAutocorrelation fed
by a Python run of the same deck."""
import glob
import os

import numpy as np
import pytest

from ddcmd_amd.analysis import VelocityAutocorrelation, parse_vaf_output
from ddcmd_amd.deck import load_deck, units_convert
from ranks import GOLDEN, copy_deck, run_driver, tree_files

pytestmark = pytest.mark.gpu
VAF = "vaf ANALYSIS { type = VELOCITYAUTOCORRELATION; eval_rate = 5; length = 4; outputrate = %d; }\n"
SIM = "simulate SIMULATE { %sdeltaloop = 80; maxloop = 80; printrate = 5; snapshotrate = 100000; checkpointrate = 100000; }\n"


def _python_files(deck, loops):
    """the same run through the Python layer, in the driver's batches of five steps: {loop: text}"""
    from ddcmd_amd.martini import MartiniHIP
    s = load_deck(deck)
    m = MartiniHIP(s, constraints=s.integrator_type.upper().startswith("NGLFCONSTRAINT") and s.nresicons > 0)
    m.eval_forces()
    m.group_temperatures()
    an = VelocityAutocorrelation(s.ngroup, s.nspecies, length=4, eval_rate=5, outputrate=40)
    gc, sc = np.bincount(s.group, minlength=max(1, s.ngroup)), np.bincount(s.species, minlength=s.nspecies)
    an.eval(m.vaf_sample, m.vaf_origin)
    out = {}
    for loop in range(5, max(loops) + 1, 5):
        m.step(5)
        m.energies()
        m.group_temperatures()
        an.eval(m.vaf_sample, m.vaf_origin)
        if loop % 40 == 0:
            out[loop] = an.output_text(s.dt, s.natoms, gc, sc, s.group_name, s.species_name)
    m.close()
    return s, out


@pytest.mark.parametrize("which", ["water_deck", "lipid_deck"])
def test_driver_writes_vaf_files(tmp_path, which):
    d = copy_deck(tmp_path, which, "with")
    run_driver(d, SIM % "analysis = vaf; " + VAF % 40)
    d0 = copy_deck(tmp_path, which, "without")
    run_driver(d0, SIM % "")
    assert open(str(d / "data"), "rb").read() == open(str(d0 / "data"), "rb").read()      # the analysis changes nothing of the run
    s, want = _python_files(str(d / "object.data"), (40, 80))
    nblock = 1 + (s.ngroup if s.ngroup > 1 else 0) + (s.nspecies if s.nspecies > 1 else 0)
    dt_fs = units_convert(s.dt, None, "fs")
    for loop in (40, 80):
        (path,) = glob.glob(str(d / ("snapshot.*%d" % loop) / "vaf.dat"))
        txt = open(path).read()
        labels, t, vaf, msd = parse_vaf_output(txt)
        assert len(labels) == nblock and vaf.shape == (nblock, 5)
        assert txt.splitlines()[0].startswith("%-33s" % "#time (fs)  System vaf MSD") and txt.splitlines()[0].endswith(" (vaf in Ang^2/fs^2; msd in Ang^2)")
        if which == "water_deck":      # two groups, two species: a block each
            assert labels == ["System"] + ["Group %s" % n for n in s.group_name] + ["Species %s" % n for n in s.species_name] and len(labels) == 5
        else:                          # one group: no group columns, the species follow the system
            assert s.ngroup == 1 and labels[1] == "Species %s" % s.species_name[0] and len(labels) == 1 + s.nspecies
        assert np.allclose(t, np.arange(5) * dt_fs * 5, rtol=0, atol=1e-6)
        assert np.all(msd[:, 0] == 0.0) and np.all(msd[0, 1:] > 0) and np.all(vaf[0, 0] > 0)
        assert want[loop] is not None
        lw, tw, vw, mw = parse_vaf_output(want[loop])
        assert lw == labels
        print(which, loop, np.abs(vaf - vw).max() / np.abs(vw).max(), np.abs(msd - mw).max() / np.abs(mw).max())
        assert np.allclose(vaf, vw, rtol=2e-6, atol=2e-6 * np.abs(vw).max()) and np.allclose(msd, mw, rtol=2e-6, atol=0)


def test_gate_shut_writes_no_file(tmp_path):
    d = copy_deck(tmp_path, "water_deck", "gate")
    run_driver(d, SIM % "analysis = vaf; " + VAF % 30)      # nsample * 4 * 5 is 20 at loop 30, 60 at loop 60: never the outputrate
    assert glob.glob(str(d / "snapshot.*" / "vaf.dat")) == []


def test_driver_two_ranks_write_the_same_file(tmp_path):
    d1 = copy_deck(tmp_path, "water_deck", "one")
    run_driver(d1, SIM % "analysis = vaf; " + VAF % 40)
    d2 = copy_deck(tmp_path, "water_deck", "two")
    run_driver(d2, SIM % "analysis = vaf; " + VAF % 40, world=2)
    for loop in (40, 80):
        (a,) = glob.glob(str(d1 / ("snapshot.*%d" % loop) / "vaf.dat"))
        (b,) = glob.glob(str(d2 / ("snapshot.*%d" % loop) / "vaf.dat"))
        ta, tb = open(a).read(), open(b).read()
        la, t1, v1, m1 = parse_vaf_output(ta)
        lb, t2, v2, m2 = parse_vaf_output(tb)
        assert la == lb and np.array_equal(t1, t2)
        # the ranks' sums are added in rank order: the digits %e prints agree unless a value sits on a rounding edge of its last digit
        assert np.allclose(v1, v2, rtol=2e-6, atol=2e-6 * np.abs(v1).max()) and np.allclose(m1, m2, rtol=2e-6, atol=0)


def test_driver_mixed_list_matches_single_analysis_runs(tmp_path):
    """a list of three types -- VELOCITYAUTOCORRELATION, an unsupported one, PAIRCORRELATION -- against the runs of its two supported
    members alone: the run itself, the g(r) files and the vaf files are the same bytes, the unsupported one is named once and writes
    nothing.  Bytes, not a tolerance: the pair counts are integers, the vaf kernels reduce without atomics, and the analyses of one
    list share no state, so the order in which the driver walks them shows in no file."""
    sim = "simulate SIMULATE { %sdeltaloop = 100; maxloop = 100; printrate = 5; snapshotrate = 100000; checkpointrate = 100000; }\n"
    rdf = "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 50; delta_r = 0.1 Angstrom; length = 100; }\n"
    other = "writeCharmm ANALYSIS { type = subsetWrite; outputrate = 10; }\n"
    da, db, dc = (copy_deck(tmp_path, "water_deck", n) for n in ("mixed", "rdf", "vaf"))
    (out,) = run_driver(da, sim % "analysis = vaf writeCharmm rdf; " + VAF % 40 + other + rdf)
    run_driver(db, sim % "analysis = rdf; " + rdf)
    run_driver(dc, sim % "analysis = vaf; " + VAF % 40)
    data = [open(str(d / "data"), "rb").read() for d in (da, db, dc)]
    assert len(data[0]) > 0 and data[0] == data[1] == data[2]
    for single, name, loops in ((db, "paircorrelation.dat", (50, 100)), (dc, "vaf.dat", (40, 80))):
        for loop in loops:
            (a,) = glob.glob(str(da / ("snapshot.*%d" % loop) / name))
            (b,) = glob.glob(str(single / ("snapshot.*%d" % loop) / name))
            ta, tb = open(a, "rb").read(), open(b, "rb").read()
            assert len(ta) > 0 and ta == tb, (name, loop)
    written = sorted(set(tree_files(da)) - set(tree_files(os.path.join(GOLDEN, "water_deck"))))
    assert written == ["data", "snapshot.%012d/vaf.dat" % 40, "snapshot.%012d/paircorrelation.dat" % 50, "snapshot.%012d/vaf.dat" % 80,
                       "snapshot.%012d/paircorrelation.dat" % 100]      # no other analysis file
    lines = [l for l in out.stderr.splitlines() if "writeCharmm" in l]
    assert len(lines) == 1 and "subsetWrite" in lines[0] and "not supported" in lines[0]

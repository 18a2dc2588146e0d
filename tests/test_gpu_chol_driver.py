"""GPU tests (-m gpu) of the ANALYSIS type cholAnalysis in the ddcmi_md driver: cholAnalysis.data in the run directory (one line per
output) and snapshot.<loop>/cholAnalysis.distn, on one rank and on two ranks over the host transport on one device -- where molecules
are split over the ranks and completed on rank 0 -- both equal to analysis.CholAnalysis fed from Python with the evaluations of the
restart states the driver writes at the loops of the evaluations."""
import os

import numpy as np
import pytest

from chol_deck import CHOL, SIM, chol_deck
from ddcmd_amd.analysis import CholAnalysis
from ddcmd_amd.deck import load_deck
from ranks import run_driver

pytestmark = pytest.mark.gpu
EXTRA = SIM % "analysis = chol; " + CHOL
FILES = ("cholAnalysis.data", os.path.join("snapshot.%012d" % 20, "cholAnalysis.distn"))


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    d = chol_deck(tmp_path_factory.mktemp("chol1"), "one")
    return d, run_driver(d, EXTRA)


def test_one_rank_writes_what_python_computes(one_rank):
    from ddcmd_amd import martini
    from ddcmd_amd.martini import MartiniHIP
    d, outs = one_rank
    assert not [l for l in outs[0][1].splitlines() if "not supported" in l]
    assert not [l for l in outs[0][0].splitlines() if "cnt1" in l]      # stdout belongs to the data lines
    s0 = load_deck(str(d / "object.data"), extra_objects=EXTRA)
    (a,) = s0.analysis
    an = CholAnalysis(a["rmin"], a["rmax"], a["delta"], a["filename"], a["data_filename"], a["eval_rate"], a["outputrate"])
    assert an.nbins == a["nbins"] == 48 and an.delta == a["delta"]
    nearest = 1.0
    for lp in (10, 20):      # the startup sample (loop 0 is due) is discarded
        s = load_deck(str(d / "object.data"), restart_file=str(d / ("snapshot.%012d" % lp) / "restart"))
        assert s.loop == lp
        m = MartiniHIP(s)
        m.eval_forces()
        counts, stats, n = m.chol_offsets(a["gid7"], a["rmin"], an.delta, an.nbins)
        assert n == 120
        an.add(counts, stats)
        # (the restart prints 14 digits of every coordinate: an offset within 1e-9 of a bin edge could change bin between the
        # device's position and the file's; none is that close here)
        order = np.argsort(s.gid)
        idx = order[np.searchsorted(s.gid[order], a["gid7"])]
        r = np.stack([s.rx, s.ry, s.rz], 1)[idx]
        for r7 in r:
            d1, d5, _, _ = martini.chol_molecule(m.lib, r7, s.box, s.pbc, a["rmin"], an.delta, an.nbins)
            for v in (d1, d5):
                q = (v - a["rmin"]) / an.delta
                nearest = min(nearest, abs(q - round(q)))
        m.close()
    assert nearest > 1e-9
    data = open(str(d / FILES[0])).read()
    assert data.count("\n") == 1
    want = an.data_line(20, s.time)
    got, exp = data.split(), want.split()
    assert got[0] == exp[0] == "20" and abs(float(got[1]) - float(exp[1])) <= 2e-6
    assert np.all(np.abs(np.array(got[2:], float) - np.array(exp[2:], float)) <= 1.01e-6)      # the digits printed
    assert open(str(d / FILES[1])).read() == an.distn_text()
    assert sorted(os.listdir(str(d / ("snapshot.%012d" % 20)))).count("cholAnalysis.distn.tmp") == 0
    assert not os.path.exists(str(d / ("snapshot.%012d" % 10) / "cholAnalysis.distn"))      # loop 10 evaluates and writes nothing


def test_two_ranks_write_the_same_files(one_rank, tmp_path):
    d1, _ = one_rank
    d2 = chol_deck(tmp_path, "two")
    outs = run_driver(d2, EXTRA, world=2)
    assert not [l for o in outs for l in o[1].splitlines() if "not supported" in l]
    assert open(str(d1 / FILES[1]), "rb").read() == open(str(d2 / FILES[1]), "rb").read()      # counts and their quotients only
    a, b = open(str(d1 / FILES[0])).read().split(), open(str(d2 / FILES[0])).read().split()
    assert len(a) == len(b) == 8 and a[:2] == b[:2]
    assert [a[k] for k in (2, 3, 5, 6)] == [b[k] for k in (2, 3, 5, 6)]      # minimum of minima, maximum of maxima: exact
    assert all(abs(float(a[k]) - float(b[k])) <= 1.01e-6 for k in (4, 7))      # the sums are added in another order: the last printed digit may differ


def test_a_deck_without_chol_writes_the_files_with_0_over_0(tmp_path):
    import shutil
    from chol_deck import LIPID
    d = tmp_path / "none"
    shutil.copytree(LIPID, str(d))
    run_driver(d, EXTRA)
    line = open(str(d / FILES[0])).read().split()
    assert line[0] == "20" and line[4] == "-nan" and line[7] == "-nan"
    rows = open(str(d / FILES[1])).read().splitlines()
    assert len(rows) == 48 and all(r.split()[1:] == ["-nan", "-nan"] for r in rows)

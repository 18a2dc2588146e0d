"""CPU tests of analysis.KineticEnergyDistn: the text of kineticEnergyDistn.c:94-97,128-153 (<name>_kDist.data and the line of
kinetic.data) from hand-made numbers, the accumulation and clearing of :157-203, and the parsers of both files."""
import re

import numpy as np
import pytest

from ddcmd_amd.analysis import KineticEnergyDistn, parse_kdist_output, parse_kinetic_output
from ddcmd_amd.deck import units_convert

EV = units_convert(1.0, "eV", None)      # 1 eV in internal units
EC = units_convert(1.0, None, "eV")


def _groups():
    return [{"name": "wDist", "species": "W", "emin": 0.0, "emax": 0.2 * EV, "nbins": 4},
            {"name": "naDist", "species": "NA", "emin": 0.01 * EV, "emax": 0.05 * EV, "nbins": 2}]


def test_header_and_species_map():
    kd = KineticEnergyDistn(_groups())
    assert kd.header() == "# loop  time(fs)   \n"
    assert list(kd.species_dist(["NA", "X", "W"])) == [1, -1, 0]
    assert list(kd.species_dist(["X", "W"])) == [-1, 0]      # a BIN of a species the system lacks maps nothing
    assert kd.filename(0) == "wDist_kDist.data" and kd.filename(1) == "naDist_kDist.data"
    with pytest.raises(ValueError):
        KineticEnergyDistn(_groups() + [{"name": "again", "species": "W", "emin": 0.0, "emax": 1.0, "nbins": 1}]).species_dist(["W"])
    for bad in ({"nbins": 0}, {"emax": 0.0}, {"emax": -1.0}):
        with pytest.raises(ValueError):
            KineticEnergyDistn([dict(_groups()[0], **bad)])


def test_dist_file_text_from_hand_made_counts():
    kd = KineticEnergyDistn(_groups())
    kd.add([3, 0, 1, 2, 5, 7], [[8, 1, 1], [12, 0, 0]], [[0.3 * EV, 0.001 * EV, 0.25 * EV], [0.36 * EV, 0.011 * EV, 0.049 * EV]])
    txt = kd.dist_text(0)
    lines = txt.splitlines()
    assert lines[0] == "# Energy (eV)      pdf (1/eV)            cnt" and len(lines[0]) == 14 + 1 + 14 + 1 + 14 and txt.endswith("\n")
    delta = (0.2 * EV - 0.0) / 4
    want = ["%e %e %e" % (((j + 0.5) * delta + 0.0) * EC, c / (8.0 * delta) / EC, c) for j, c in enumerate((3.0, 0.0, 1.0, 2.0))]
    assert lines[1:] == want
    e, pdf, cnt = parse_kdist_output(txt)
    assert np.allclose(e, [0.025, 0.075, 0.125, 0.175], rtol=1e-6) and list(cnt) == [3, 0, 1, 2]
    assert np.allclose(pdf, np.array([3, 0, 1, 2]) / (8 * 0.05), rtol=1e-6)      # the pdf of the beads inside and outside: 6/8 of it lies in the bins
    assert abs((pdf * 0.05).sum() - 6 / 8) < 1e-6
    e1, _, cnt1 = parse_kdist_output(kd.dist_text(1))
    assert np.allclose(e1, [0.02, 0.04], rtol=1e-6) and list(cnt1) == [5, 7]


def test_kinetic_line_two_groups_repeat_loop_and_time():
    kd = KineticEnergyDistn(_groups())
    kd.add([3, 0, 1, 2, 5, 7], [[8, 1, 1], [12, 0, 0]], [[0.3 * EV, 0.001 * EV, 0.25 * EV], [0.36 * EV, 0.011 * EV, 0.049 * EV]])
    t = 1234.5      # written as it is: internal units
    line = kd.line(40, t)
    head = "%12d" % 40 + " %16.6f " % t
    want = head + "%12.6f %12.8f %12.8f %4.0f %4.0f %8.0f " % (0.3 * EV / 8 * EC, 0.001 * EV * EC, 0.25 * EV * EC, 1, 1, 8)
    want += head + "%12.6f %12.8f %12.8f %4.0f %4.0f %8.0f " % (0.36 * EV / 12 * EC, 0.011 * EV * EC, 0.049 * EV * EC, 0, 0, 12)
    assert line == want + "\n"
    assert line.count("          40      1234.500000 ") == 2
    assert len(line) == 2 * (12 + 18 + 13 + 13 + 13 + 5 + 5 + 9) + 1
    (loop, time, val), (loop2, _, _) = parse_kinetic_output(kd.header() + line + kd.line(50, 2 * t))
    assert list(loop) == [40, 40] and list(time) == [1234.5, 1234.5] and list(loop2) == [50, 50]
    assert np.allclose(val, [[0.0375, 0.001, 0.25, 1, 1, 8], [0.03, 0.011, 0.049, 0, 0, 12]], rtol=0, atol=5.1e-7)


def test_evaluations_accumulate_until_clear():
    kd = KineticEnergyDistn(_groups())
    kd.add([1, 1, 1, 1, 2, 2], [[5, 1, 0], [4, 0, 0]], [[1.0, 0.25, 0.5], [2.0, 0.75, 0.875]])
    kd.add([0, 2, 0, 0, 1, 0], [[2, 0, 0], [3, 1, 1]], [[0.5, 0.125, 0.375], [1.0, 0.5, 1.5]])
    assert list(kd.cnt) == [1, 3, 1, 1, 3, 2] and kd.tallies.tolist() == [[7, 1, 0], [7, 1, 1]]
    assert list(kd.sum) == [1.5, 3.0] and list(kd.min) == [0.125, 0.5] and list(kd.max) == [0.5, 1.5]
    kd.clear()
    assert not kd.cnt.any() and not kd.tallies.any() and not kd.sum.any() and list(kd.min) == [1e300, 1e300] and list(kd.max) == [0.0, 0.0]


def test_empty_group_prints_what_c_prints():
    kd = KineticEnergyDistn(_groups())      # nothing added: cntTotal = 0
    lines = kd.dist_text(1).splitlines()
    assert len(lines) == 3
    for j, ln in enumerate(lines[1:]):
        m = re.fullmatch(r"(\S+) (-?nan) (\S+)", ln)      # 0/0 under %e
        assert m and float(m.group(3)) == 0.0 and abs(float(m.group(1)) - (0.02 + 0.02 * j)) < 1e-6
    e, pdf, cnt = parse_kdist_output(kd.dist_text(1))
    assert np.all(np.isnan(pdf)) and not cnt.any()
    line = kd.line(7, 0.0)
    w = line.split()
    assert len(w) == 16 and w[2] == "0.000000" and w[4] == "0.00000000" and w[5:8] == ["0", "0", "0"]      # ave 0 where cntTotal is 0
    assert w[3] == ("%12.8f" % (1e300 * EC)).strip() and len(w[3]) > 280      # the minimum nobody lowered: 1e300 eC in full
    (_, _, val), = parse_kinetic_output(line)
    assert val[0, 1] == float(w[3]) and abs(val[0, 1] / (1e300 * EC) - 1) < 1e-15


def test_zero_groups():
    kd = KineticEnergyDistn([])
    assert kd.line(10, 5.0) == "\n" and kd.nd == 0 and list(kd.species_dist(["A", "B"])) == [-1, -1]
    kd.add(np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3)))
    out = parse_kinetic_output(kd.header() + kd.line(10, 5.0))
    assert len(out) == 1 and out[0][0].shape == (0,) and out[0][2].shape == (0, 6)

"""CPU tests of ddcmd_amd.analysis.VelocityAutocorrelation: the windows of velocityAutocorrelation_eval and the file of
velocityAutocorrelation_output (velocityAutocorrelation.c:117-327) against sums done by hand, the file's round trip, the gate."""
import numpy as np
import pytest

from ddcmd_amd.analysis import VelocityAutocorrelation, parse_vaf_output
from ddcmd_amd.deck import units_convert


class ThreeBeads(object):
    """three beads, two groups {0, 1 | 2}, two species {0 | 1, 2}, moving on straight lines with velocities that change sign"""

    def __init__(self):
        self.group, self.species = np.array([0, 0, 1]), np.array([0, 1, 1])
        self.t = 0
        self.v = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, -3.0]])
        self.r = np.zeros((3, 3))
        self.norigin = 0

    def step(self):
        self.t += 1
        self.r += self.v
        self.v = self.v * np.array([[1.0], [-0.5], [2.0]])

    def origin(self):
        self.v0, self.r0 = self.v.copy(), self.r.copy()
        self.norigin += 1

    def sample(self):
        a = (self.v0 * self.v).sum(axis=1)
        b = ((self.r - self.r0) ** 2).sum(axis=1)
        cls = [np.ones(3, bool), self.group == 0, self.group == 1, self.species == 0, self.species == 1]
        return np.array([a[m].sum() for m in cls]), np.array([b[m].sum() for m in cls])


def test_two_windows_of_three_beads_by_hand():
    b = ThreeBeads()
    an = VelocityAutocorrelation(2, 2, length=2, eval_rate=1, outputrate=4)
    an.eval(b.sample, b.origin)      # the startup evaluation: the first origin, sample 0
    assert b.norigin == 1 and an.last == 1 and an.nsample == 0
    for k in range(4):
        b.step()
        an.eval(b.sample, b.origin)
    assert b.norigin == 3 and an.nsample == 2 and an.last == 1
    # by hand.  velocities: bead 0 (1,0,0) always; bead 1 y = 2, -1, .5, -.25, .125; bead 2 z = -3, -6, -12, -24, -48
    # window 1 (origin t = 0): vaf k = 0, 1, 2 -- bead 0: 1 1 1; bead 1: 4 -2 1; bead 2: 9 18 36; d: bead 0: 0 1 2; bead 1: 0 2 1; bead 2: 0 3 9
    # window 2 (origin t = 2): bead 0: 1 1 1; bead 1: .25 -.125 .0625; bead 2: 144 288 576; d: 0 1 2; 0 .5 .25; 0 12 36
    vaf_b = np.array([[[1, 1, 1], [4, -2, 1], [9, 18, 36]], [[1, 1, 1], [.25, -.125, .0625], [144, 288, 576]]], float)
    d_b = np.array([[[0, 1, 2], [0, 2, 1], [0, 3, 9]], [[0, 1, 2], [0, .5, .25], [0, 12, 36]]], float)
    vb, mb = vaf_b.sum(axis=0), (d_b ** 2).sum(axis=0)      # [bead, k] summed over the windows
    want_v = np.array([vb.sum(axis=0), vb[0] + vb[1], vb[2], vb[0], vb[1] + vb[2]])
    want_m = np.array([mb.sum(axis=0), mb[0] + mb[1], mb[2], mb[0], mb[1] + mb[2]])
    assert np.array_equal(an.vaf_, want_v) and np.array_equal(an.msd_, want_m)
    # the third window has begun: its sample 0
    assert an.vaf0[0, 0] == 1 + .125 ** 2 + 48.0 ** 2 and np.all(an.msd0 == 0)
    assert an.gate()
    text = an.output_text(dt=2.0, nglobal=3, group_counts=[2, 1], species_counts=[1, 2], group_names=["a", "b"], species_names=["X", "Y"])
    assert an.nsample == 0 and np.all(an.vaf_ == 0) and np.all(an.msd_ == 0)
    labels, t, vaf, msd = parse_vaf_output(text)
    assert labels == ["System", "Group a", "Group b", "Species X", "Species Y"]
    tc, v2c, r2c = units_convert(1.0, None, "t"), units_convert(1.0, None, "velocity^2"), units_convert(1.0, None, "l^2")
    assert np.isfinite(v2c) and v2c > 0
    assert np.allclose(t, tc * np.arange(3) * 2.0 * 1, rtol=0, atol=1e-6)
    cnt = np.array([3, 2, 1, 1, 2], float)[:, None]
    assert np.allclose(vaf, v2c * want_v / 2 / cnt, rtol=2e-6) and np.allclose(msd, r2c * want_m / 2 / cnt, rtol=2e-6)


def test_file_format_and_the_single_group_single_species_rule():
    an = VelocityAutocorrelation(1, 1, length=1, eval_rate=5, outputrate=5)
    an.add([2.0, 2.0, 2.0], [0.0, 0.0, 0.0], k=0)
    an.add([1.0, 1.0, 1.0], [4.0, 4.0, 4.0], k=1)
    an.accumulate()
    text = an.output_text(1.0, 2, [2], [2], ["all"], ["W"])
    lines = text.splitlines()
    assert lines[0] == "%-33s" % "#time (fs)  System vaf MSD" + " (vaf in Ang^2/fs^2; msd in Ang^2)"
    assert len(lines) == 3 and all(len(ln.split()) == 3 for ln in lines[1:])      # no group and no species columns
    assert lines[1].split()[0] == "0.000000" and lines[1].split()[2] == "0.000000e+00"
    an2 = VelocityAutocorrelation(2, 3, length=1, eval_rate=5, outputrate=5)
    an2.add(np.arange(6.0), np.zeros(6), k=0)
    an2.add(np.arange(6.0), np.arange(6.0), k=1)
    an2.accumulate()
    text2 = an2.output_text(1.0, 6, [3, 3], [2, 2, 2], ["g0", "g1"], ["A", "B", "C"])
    head = text2.splitlines()[0]
    assert head.startswith("%-33s" % "#time (fs)  System vaf MSD" + "%-26s" % "  Group g0 vaf MSD" + "%-26s" % "  Group g1 vaf MSD" + "%-26s" % "  Species A vaf MSD")
    labels, t, vaf, msd = parse_vaf_output(text2)
    assert labels == ["System", "Group g0", "Group g1", "Species A", "Species B", "Species C"] and vaf.shape == (6, 2) and msd.shape == (6, 2)
    assert all(len(ln.split()) == 13 for ln in text2.splitlines()[1:])


def test_gate_shut_writes_nothing_and_resets_nothing():
    an = VelocityAutocorrelation(1, 1, length=2, eval_rate=5, outputrate=30)      # one window is 10 steps: three make 30
    for w in range(2):
        for k in range(3):
            an.add([1.0] * 3, [float(k)] * 3, k=k)
        an.accumulate()
    assert not an.gate() and an.output_text(1.0, 1, [1], [1], ["g"], ["s"]) is None
    assert an.nsample == 2 and an.msd_[0, 2] == 4.0
    for k in range(3):
        an.add([1.0] * 3, [float(k)] * 3, k=k)
    an.accumulate()
    assert an.gate() and an.output_text(1.0, 1, [1], [1], ["g"], ["s"]) is not None and an.nsample == 0


def test_length_below_one_is_refused():
    with pytest.raises(ValueError):
        VelocityAutocorrelation(1, 1, length=0)

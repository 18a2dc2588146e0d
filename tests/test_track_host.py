"""CPU tests of the FORCE_AVERAGE analysis' host side: the three entry points are declared and exported, and analysis.ForceAverage
writes forceAverage.c's texts -- the header of forceAverage_parms, the line of forceAverage_output from its formats, the gate
nSnapSum * eval_rate < outputrate, and the clearing that only a written line does."""
import os
import subprocess

import numpy as np
import pytest

from ddcmd_amd.analysis import ForceAverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ddcmi_track_set", "ddcmi_track_accumulate", "ddcmi_track_read")


def test_the_three_symbols_are_declared_and_exported(built):
    header = open(os.path.join(ROOT, "include", "ddcmi.h")).read()
    assert "int ddcmi_track_set(ddcmi_ctx *ctx, int64_t n, const uint64_t *gid);" in header
    assert "int ddcmi_track_accumulate(ddcmi_ctx *ctx, int what" in header
    assert "int ddcmi_track_read(ddcmi_ctx *ctx, int64_t n, double *sum" in header
    for lib in ("libddcmi.so", "libddcmi_test.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "ddcmd_amd", "lib", lib)], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(NAMES) <= exported, lib
        assert not [n for n in exported if "track" in n and n not in NAMES], lib      # no group entry: the three are legal for a group's contexts


class FakeContext(object):
    """what ForceAverage asks of a Martini* object: the list, one sample, the read with its reset; every sample adds `value` per gid"""

    def __init__(self):
        self.calls = []

    def track_set(self, gids):
        self.gids = list(gids)
        self.tot, self.hits = np.zeros((len(self.gids), 3)), np.zeros(len(self.gids), np.int64)
        self.calls.append("set")

    def track_accumulate(self, what):
        self.calls.append(what)
        self.tot += self.value
        self.hits += 1

    def track_read(self, reset=False):
        self.calls.append("read+reset" if reset else "read")
        out = self.tot.copy(), self.hits.copy()
        if reset:
            self.tot[:], self.hits[:] = 0.0, 0
        return out


def test_header_text():
    an = ForceAverage([2 ** 40 + 3, 7, 7], "force")
    assert an.header() == "# loop  time  1099511627779  7  7  \n"      # "%llu  " per id, duplicates as listed
    assert ForceAverage([], "position").header() == "# loop  time  \n"


def test_line_text_from_the_formats_of_forceAverage_output():
    # loopFormat() is "%12.12lu"; then " %10.6f " of the time; per id " %12.7f %12.7f %12.7f " of sum / nSnapSum; internal units
    an = ForceAverage([5, 9], "velocity", eval_rate=1, outputrate=1)
    an.nsnap = 4
    total = np.array([[1.0, -2.0, 0.5], [4e-7, 123456.7891236, -0.00000004]])
    got = an.text(120, 2400.5, total, [4, 4])
    assert got == ("000000000120" + " 2400.500000 " + "    0.2500000   -0.5000000    0.1250000 " + "    0.0000001 30864.1972809   -0.0000000 " + "\n")
    with pytest.raises(RuntimeError, match="gid 9 was found 3 times in 4 evaluations"):
        an.text(120, 2400.5, total, [4, 3])


def test_data_type_and_eval_rate_are_checked():
    assert ForceAverage([1], "POSITION").data_type == "position"
    with pytest.raises(ValueError, match="none of force, velocity, position"):
        ForceAverage([1], "momentum")
    with pytest.raises(ValueError, match="eval_rate = 0"):
        ForceAverage([1], "force", eval_rate=0)


def test_gate_and_clear_after_a_written_line_only():
    """eval_rate 2, outputrate 5, the reference's arithmetic nSnapSum * eval_rate < outputrate: at loop 5 the two samples of loops 2 and 4
    give 4 < 5 -- nothing is written and nothing is cleared; at loop 10 the window holds five samples and is written and cleared.  A
    window of the three samples of loops 6, 8, 10 gives 6 >= 5 and is written at loop 10 as well."""
    m = FakeContext()
    m.value = np.array([[1.0, 2.0, 3.0]])
    an = ForceAverage([11], "force", eval_rate=2, outputrate=5)
    an.sample(m); an.clear()      # the startup sample, discarded
    assert m.calls == ["set", "force", "read+reset"] and an.nsnap == 0
    written = {}
    for loop in range(1, 11):
        if loop % 2 == 0:
            an.sample(m)
        if loop % 5 == 0:
            written[loop] = an.line(loop, 20.0 * loop)
            if loop == 5:
                assert written[5] is None and an.nsnap == 2 and m.hits[0] == 2      # gated: not written, not cleared
    assert written[10] == "000000000010" + " 200.000000 " + "    1.0000000    2.0000000    3.0000000 " + "\n"      # 5 samples: 5 / 5
    assert an.nsnap == 0 and m.hits[0] == 0 and m.calls[-2:] == ["read", "read+reset"]
    # three samples at loop 10
    an = ForceAverage([11], "force", eval_rate=2, outputrate=5)
    m = FakeContext()
    m.value = np.array([[3.0, 0.0, -3.0]])
    for loop in (6, 8, 10):
        an.sample(m)
    assert an.nsnap * an.eval_rate >= an.outputrate      # 3 * 2 >= 5
    assert an.line(10, 0.0) == "000000000010" + "   0.000000 " + "    3.0000000    0.0000000   -3.0000000 " + "\n"
    assert an.line(10, 0.0) is None      # cleared: 0 * 2 < 5

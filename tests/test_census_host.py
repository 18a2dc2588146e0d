"""CPU tests of analysis.VcmWrite and analysis.ZDensity: the text of vcmWrite.c:38-58,117-130 and zdensity.c:164-172 from hand-made
sums."""
import numpy as np
import pytest

from ddcmd_amd.analysis import VcmWrite, ZDensity, parse_vcm_output
from ddcmd_amd.deck import units_convert


def test_vcm_header_widths():
    v = VcmWrite(["group", "free"], ["WxW", "WFxWF"])
    h = v.header()
    # "-%12s %14s": the reference's format string as it stands -- a literal '-', then both words right-aligned
    assert h.startswith("-" + " " * 7 + "#loop" + " " + " " * 6 + "time(fs)")
    assert h.endswith("\n") and len(h) == 1 + 12 + 1 + 14 + 51 * 5 + 1
    body = h[28:-1]
    blocks = [body[k * 51:(k + 1) * 51] for k in range(5)]
    assert blocks[0] == "%-51s" % "     System vx vy vz (Ang/fs)"
    assert [b.rstrip() for b in blocks[1:]] == ["     Group group vx vy vz (Ang/fs)", "     Group free vx vy vz (Ang/fs)",
                                                "     Species WxW vx vy vz (Ang/fs)", "     Species WFxWF vx vy vz (Ang/fs)"]
    # a single group and a single species keep their blocks
    assert len(VcmWrite(["g"], ["s"]).header()) == 1 + 12 + 1 + 14 + 51 * 3 + 1


def test_vcm_line_divides_by_the_mass_where_there_is_one():
    v = VcmWrite(["a", "b"], ["s"])
    vc = units_convert(1.0, None, "Ang/fs")
    mv = np.array([[2.0, -4.0, 6.0], [1.0, 1.0, 1.0], [3.0, 0.0, -3.0], [2.0, -4.0, 6.0]])
    m = np.array([4.0, 0.0, 1.5, 4.0])      # class 1 (group a) has no mass: its sums are written undivided
    t = 123.456 * units_convert(1.0, "fs", None)
    line = v.line(20, t, mv, m)
    want = "%12d" % 20 + " %16.6f" % 123.456
    for c, div in enumerate((4.0, None, 1.5, 4.0)):
        x = mv[c] * (1 / div) if div else mv[c]
        want += " %16.6e %16.6e %16.6e" % tuple(x * vc)
    assert line == want + "\n"
    assert len(line) == 12 + 17 + 4 * 3 * 17 + 1
    loop, time, vcm = parse_vcm_output(v.header() + line + v.line(30, 2 * t, mv, m))
    assert list(loop) == [20, 30] and np.allclose(time, [123.456, 246.912]) and vcm.shape == (2, 4, 3)
    assert np.allclose(vcm[0, 1], mv[1] * vc, rtol=1e-6) and np.allclose(vcm[0, 2], mv[2] / 1.5 * vc, rtol=1e-6)


def test_zdensity_text_columns():
    ang = units_convert(1.0, "Angstrom", None)
    box = (10.0 * ang, 20.0 * ang, 40.0 * ang)      # 8000 A^3
    z = ZDensity(4, filename="p.dat")
    txt = z.output_text([1.0, 0.0, 2.5, 1000000.0], box)
    lines = txt.splitlines()
    assert len(lines) == 4 and txt.endswith("\n")
    assert lines[0] == "0.125000 0.000500 1.000000"
    assert lines[1] == "0.375000 0.000000 0.000000"
    assert lines[2] == "0.625000 0.001250 2.500000"
    assert lines[3] == "0.875000 500.000000 1000000.000000"
    assert ZDensity(1).output_text([7.0], box) == "0.500000 0.000875 7.000000\n"


def test_zdensity_words_and_refusal():
    assert ZDensity(3, smear_method="HAT").smear_method == "hat" and ZDensity(3, smear_method="other").smear_method == "impulse"
    with pytest.raises(ValueError):
        ZDensity(0)

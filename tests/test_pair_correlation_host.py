"""CPU tests of the host side of ANALYSIS PAIRCORRELATION (ddcmd_amd/analysis.py): comboIndex, the accumulation of samples and the
normalisation of paircorrelation_output against hand-computed numbers, and the output file's format."""
import numpy as np

from ddcmd_amd.analysis import PairCorrelation, bin_edges, combo_index, combo_pairs, parse_output
from ddcmd_amd.deck import units_convert


def test_combo_index_is_the_references():
    # comboIndex(i, j, ns) = (max - min) + ns*min - min(min-1)/2: for 3 species AA AB AC BB BC CC
    assert [combo_index(a, b, 3) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))] == [0, 1, 2, 3, 4, 5]
    assert combo_index(2, 0, 3) == combo_index(0, 2, 3)
    assert combo_pairs(19)[-1] == (18, 18) and len(combo_pairs(19)) == 190
    assert sorted(combo_index(a, b, 19) for a in range(19) for b in range(a, 19)) == list(range(190))


def test_bin_edges_linear_and_log():
    left, right = bin_edges(1.0, 0.5, 4)
    assert np.allclose(left, [1.0, 1.5, 2.0, 2.5]) and np.allclose(right, [1.5, 2.0, 2.5, 3.0])
    left, right = bin_edges(1.0, 4.5, 2, log=True)      # rmax = 10: one decade in two bins
    assert np.allclose(left, [1.0, 10 ** 0.5]) and np.allclose(right, [10 ** 0.5, 10.0])


def test_normalisation_by_hand():
    """two species (N_A = 2, N_B = 4), one bin [1, 2), two samples, box volume 100"""
    pc = PairCorrelation(2, rmin=1.0, delta_r=1.0, nbins=1)
    pc.add([[4], [8], [12]], [2, 4])          # AA: 4 / (2*2) = 1, AB: 8 / (2*4) = 1, BB: 12 / (4*4) = 0.75
    pc.add([[2], [0], [4]], [2, 4])           # 0.5, 0, 0.25
    assert pc.nsample == 2 and np.allclose(pc.g[:, 0], [1.5, 1.0, 1.0])
    dv = 4.0 * np.pi / 3.0 * (8.0 - 1.0)
    assert np.allclose(pc.normalised(100.0)[:, 0], np.array([1.5, 1.0, 1.0]) * (100.0 / 2) / dv)


def test_output_file_format_and_clear():
    ang = units_convert(1.0, "Angstrom", None)
    pc = PairCorrelation(2, rmin=0.0, delta_r=0.5 * ang, nbins=3, eval_rate=10, outputrate=50)
    pc.add(np.arange(9).reshape(3, 3), [3, 5])
    txt = pc.output_text(1000.0, ["W", "NA"])
    lines = txt.splitlines()
    assert lines[0] == "# rmin = 0.000000 Ang; delta_r = 0.500000 Ang; length = 3; eval_rate = 10; outputrate = 50;"
    assert lines[1] == "# nsample = 1;"
    assert lines[2] == "# r(Ang) W-W W-NA NA-NA "
    assert lines[3].startswith("0.250000 ") and len(lines) == 6
    fields, ns, names, r, g = parse_output(txt)
    assert ns == 1 and names == ["W-W", "W-NA", "NA-NA"] and fields["length"] == "3"
    assert np.allclose(r, [0.25, 0.75, 1.25])
    assert g.shape == (3, 3) and g[0, 0] == 0.0 and np.isclose(g[1, 2], 5.0 / 15 * 1000.0 / (4 * np.pi / 3 * ((1.5 * ang) ** 3 - ang ** 3)), rtol=1e-6)
    assert pc.nsample == 0 and not pc.g.any()      # cleared
    assert pc.output_text(1000.0, ["W", "NA"]) is None

"""CPU tests of analysis.DynamicStructureFactor: the wave vectors of addKvectors (dsf.c:234-269), the pick of their columns out of the
device's [3, mmax] block, the division by the count, the buffer of outputrate / eval_rate + 1 rows, and the header and row text --
against literal strings written out by hand from dsf.c's format strings ("%-8s %16s", "%-30s" of "    (%d,%d,%d)"; "%8.8d %16.6f",
"   %13.6e %13.6e")."""
import numpy as np
import pytest

from ddcmd_amd.analysis import DynamicStructureFactor, parse_dsf_output


def test_wave_vectors_follow_the_list():
    an = DynamicStructureFactor([2, 1, 2, 0, -3], eval_rate=1, outputrate=1)
    assert an.kvec == [(0, 0, 2), (0, 2, 0), (2, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 2), (0, 2, 0), (2, 0, 0)]
    assert an.mmax == 2 and an.filename == "rho_k.data" and an.select(["A", "B"]) is None
    rho = np.array([[10 + 1j, 20 + 2j], [30 + 3j, 40 + 4j], [50 + 5j, 60 + 6j]])      # [axis, m - 1]
    assert an.pick(rho).tolist() == [60 + 6j, 40 + 4j, 20 + 2j, 50 + 5j, 30 + 3j, 10 + 1j, 60 + 6j, 40 + 4j, 20 + 2j]
    none = DynamicStructureFactor([0, -1], eval_rate=1, outputrate=1)
    assert none.kvec == [] and none.mmax == 0 and none.header() == "#loop                time\n"


def test_species_and_refusals():
    an = DynamicStructureFactor([1], species="PO4", eval_rate=10, outputrate=20)
    assert an.filename == "rho_k_PO4.data" and an.nbufmax == 3
    assert an.select(["NC3", "PO4", "GL1"]).tolist() == [0, 1, 0] and an.select(["NC3", "PO4", "GL1"]).dtype == np.int32
    with pytest.raises(ValueError, match="species PO4 is not a species of the system"):
        an.select(["W"])
    assert DynamicStructureFactor([1], species="PO4", eval_rate=1, outputrate=1, filename="x.dat").filename == "x.dat"
    for ev, out in ((0, 1), (1, 0), (-1, 5)):
        with pytest.raises(ValueError, match="both must be at least 1"):
            DynamicStructureFactor([1], eval_rate=ev, outputrate=out)
    with pytest.raises(ValueError, match="no m"):
        DynamicStructureFactor([], eval_rate=1, outputrate=1)


def test_header_and_rows_are_the_references_text():
    an = DynamicStructureFactor([1, 12], eval_rate=10, outputrate=20)
    assert an.header() == ("#loop                time"
                           "    (0,0,1)                   " "    (0,1,0)                   " "    (1,0,0)                   "
                           "    (0,0,12)                  " "    (0,12,0)                  " "    (12,0,0)                  " "\n")
    rho = np.zeros((3, 12), np.complex128)
    rho[2, 0], rho[1, 0], rho[0, 0] = 4.0 - 2.0j, 1.0e-7 + 0.5j, -123.456 + 0j
    rho[2, 11], rho[1, 11], rho[0, 11] = 0, 8.0j, -1.0 / 3.0 + 2.0e10j
    assert an.add(30, 1234.5678916, rho, 4) == ""      # divided by the count
    assert an.add(123456789, 0.0, rho, 0) == ""      # a count of zero divides nothing
    assert an.output() == ("00000030      1234.567892"
                           "    1.000000e+00 -5.000000e-01" "    2.500000e-08  1.250000e-01" "   -3.086400e+01  0.000000e+00"
                           "    0.000000e+00  0.000000e+00" "    0.000000e+00  2.000000e+00" "   -8.333333e-02  5.000000e+09" "\n"
                           "123456789         0.000000"
                           "    4.000000e+00 -2.000000e+00" "    1.000000e-07  5.000000e-01" "   -1.234560e+02  0.000000e+00"
                           "    0.000000e+00  0.000000e+00" "    0.000000e+00  8.000000e+00" "   -3.333333e-01  2.000000e+10" "\n")
    assert an.output() == ""      # emptied


def test_a_full_buffer_is_flushed_by_the_next_evaluation():
    an = DynamicStructureFactor([1], eval_rate=10, outputrate=25)      # 25 / 10 + 1 = 3 rows
    assert an.nbufmax == 3
    rho = np.ones((3, 1), np.complex128)
    assert [an.add(10 * k, float(k), rho * k, 1) for k in range(3)] == ["", "", ""]
    flushed = an.add(30, 3.0, rho * 3, 1)
    loop, time, z = parse_dsf_output(flushed)
    assert loop.tolist() == [0, 10, 20] and time.tolist() == [0.0, 1.0, 2.0] and z.shape == (3, 3) and np.array_equal(z[:, 0], [0, 1, 2])
    loop, _, z = parse_dsf_output(an.header() + an.output())
    assert loop.tolist() == [30] and z.tolist() == [[3, 3, 3]]
    one = DynamicStructureFactor([1], eval_rate=10, outputrate=5)      # 5 / 10 + 1 = 1 row: every evaluation flushes the one before
    assert one.add(0, 0.0, rho, 1) == "" and one.add(10, 1.0, rho, 1).startswith("00000000 ") and one.output().startswith("00000010 ")

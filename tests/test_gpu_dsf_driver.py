"""GPU tests (-m gpu) of the ANALYSIS type DSF in the ddcmi_md driver on the lipid deck (charged head groups): the file in the run
directory -- one header at init, one row per evaluation, the startup one included, written at every output and, for what is still
buffered, at the end of the run -- held against analysis.DynamicStructureFactor fed by a Python run of the same deck
(Martini.charge_density_modes at the loops of the evaluations); one rank against two."""
import os

import numpy as np
import pytest

from ddcmd_amd.analysis import DynamicStructureFactor, parse_dsf_output
from ddcmd_amd.deck import load_deck
from ranks import copy_deck, run_driver

pytestmark = pytest.mark.gpu
DSF = ("po4 ANALYSIS { type = DSF; m = 1 2 4; species = DPPCxPO4; eval_rate = 10; outputrate = 20; }\n"
       "all ANALYSIS { type = DynamicStructureFactor; m = 3 0 1; eval_rate = 10; outputrate = 20; filename = everything.data; }\n")
SIM = "simulate SIMULATE { analysis = po4 all; deltaloop = 50; maxloop = 50; printrate = 10; snapshotrate = 100000; checkpointrate = 100000; }\n"
LOOPS = [0, 10, 20, 30, 40, 50]      # 20 and 40 write three and two rows; the row of loop 50 is written when the run ends


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    d = copy_deck(tmp_path_factory.mktemp("dsf"), "lipid_deck", "one")
    return d, run_driver(d, SIM + DSF)


def _python_files(deck):
    """the same run through the Python layer, in the driver's batches of ten steps: {filename: text}"""
    from ddcmd_amd.martini import MartiniHIP
    s = load_deck(deck, extra_objects=SIM + DSF)
    ans = [DynamicStructureFactor(a["m"], a["species"], a["eval_rate"], a["outputrate"], a["filename"]) for a in s.analysis]
    assert [a.filename for a in ans] == ["rho_k_DPPCxPO4.data", "everything.data"] and [a.mmax for a in ans] == [4, 3]
    m = MartiniHIP(s, constraints=s.integrator_type.upper().startswith("NGLFCONSTRAINT") and s.nresicons > 0)
    m.eval_forces()
    m.group_temperatures()
    text = {a.filename: a.header() for a in ans}
    time = s.time
    for loop in LOOPS:
        if loop:
            m.step(10)
            m.energies()
            m.group_temperatures()
            for _ in range(10):
                time += s.dt      # the sum the driver forms step by step
        for a in ans:
            rho, count = m.charge_density_modes(a.mmax, select=a.select(s.species_name))
            text[a.filename] += a.add(loop, time, rho, count)
            if loop and loop % a.outputrate == 0:
                text[a.filename] += a.output()
    for a in ans:
        text[a.filename] += a.output()      # dsf_close
    m.close()
    return s, ans, text


def _close(got, want):
    """two rows' values to the digits printed: 7 significant ones (and a sum that cancels to nothing may print anything below 1e-12)"""
    return np.all(np.abs(got - want) <= 1.01e-6 * np.abs(want) + 1e-12)


def test_driver_writes_the_rows_of_a_python_run(one_rank):
    d, outs = one_rank
    assert not [l for l in outs[0][1].splitlines() if "not supported" in l]
    s, ans, text = _python_files(str(d / "object.data"))
    npo4 = int((s.species == s.species_name.index("DPPCxPO4")).sum())
    assert npo4 > 0 and s.charge[s.species_name.index("DPPCxPO4")] == -1.0
    for a in ans:
        got = open(str(d / a.filename)).read()
        want = text[a.filename]
        gl, wl = got.splitlines(), want.splitlines()
        assert got.endswith("\n") and got.count("#") == 1 and gl[0] == wl[0] == a.header()[:-1]      # one header, at start
        assert len(gl) == len(wl) == 1 + len(LOOPS) and [len(x) for x in gl] == [len(x) for x in wl]
        loop, time, z = parse_dsf_output(got)
        wloop, wtime, wz = parse_dsf_output(want)
        assert loop.tolist() == wloop.tolist() == LOOPS      # the startup sample is kept, the last row is written at the end
        assert np.all(np.abs(time - wtime) <= 1.01e-6) and time[0] == round(s.time, 6) and abs(time[-1] - (s.time + 50 * s.dt)) <= 1e-5
        assert z.shape == (len(LOOPS), len(a.kvec)) == wz.shape
        print(a.filename, np.abs(z - wz).max())
        assert _close(z.real, wz.real) and _close(z.imag, wz.imag)
    po4 = parse_dsf_output(open(str(d / "rho_k_DPPCxPO4.data")).read())[2]
    assert ans[0].kvec == [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 2), (0, 2, 0), (2, 0, 0), (0, 0, 4), (0, 4, 0), (4, 0, 0)]
    assert np.all(np.abs(po4) <= 1.0 + 1e-6) and np.abs(po4).max() > 1e-3      # (1/N) sum of N unit phases times q = -1
    assert ans[1].kvec == [(0, 0, 3), (0, 3, 0), (3, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
    assert not os.path.exists(str(d / "rho_k.data"))


def test_driver_two_ranks_write_the_same_rows(one_rank, tmp_path):
    d1, _ = one_rank
    d2 = copy_deck(tmp_path, "lipid_deck", "two")
    outs = run_driver(d2, SIM + DSF, world=2)
    assert not [l for o in outs for l in o[1].splitlines() if "not supported" in l]
    for f in ("rho_k_DPPCxPO4.data", "everything.data"):
        a, b = open(str(d1 / f)).read(), open(str(d2 / f)).read()
        assert a.count("#") == 1 and b.count("#") == 1 and a.splitlines()[0] == b.splitlines()[0]      # rank 0 alone opens the file
        (la, ta, za), (lb, tb, zb) = parse_dsf_output(a), parse_dsf_output(b)
        assert la.tolist() == lb.tolist() == LOOPS and np.array_equal(ta, tb) and za.shape == zb.shape
        print(f, np.abs(za - zb).max())
        assert _close(za.real, zb.real) and _close(za.imag, zb.imag)      # the ranks' sums are added in another order: the last digit may differ

"""GPU tests (-m gpu) of the ANALYSIS type KINETICENERGYDISTN in the ddcmi_md driver: kinetic.data in the run directory (one header
at init, one line per output with loop and time repeated per group) and snapshot.<loop>/<BIN name>_kDist.data, held against the
restatement of kineticEnergyDistn.c applied to the restart states the driver writes at the loops of the evaluations; several
evaluations per output; one rank against two; a mixed list against the same list without the new type."""
import os

import numpy as np
import pytest

from ddcmd_amd.analysis import KineticEnergyDistn, parse_kdist_output, parse_kinetic_output
from ddcmd_amd.deck import load_deck
from ranks import GOLDEN, copy_deck, run_driver, tree_files

pytestmark = pytest.mark.gpu
KD = ("kd ANALYSIS { type = KINETICENERGYDISTN; eval_rate = 5; outputrate = 10; distGroups = wDist fDist none; }\n"
      "wDist BIN { species = WxW; emin = 0 eV; emax = 0.2 eV; nBins = 20; }\n"      # the Langevin groups hold 310 K: kT = 0.0267 eV, 0.2 eV = 7.5 kT
      "fDist BIN { species = WFxWF; emin = 0.01 eV; emax = 0.1 eV; nBins = 8; }\n"      # 0.37 kT to 3.7 kT: about 15 % of the beads below, 6 % above
      "none BIN { species = NA; emin = 0.01 eV; emax = 0.03 eV; nBins = 2; }\n")      # a species the deck lacks: an empty group
SIM = "simulate SIMULATE { %sdeltaloop = 20; maxloop = 20; printrate = 5; snapshotrate = 5; checkpointrate = 100000; }\n"


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    d = copy_deck(tmp_path_factory.mktemp("kdist"), "water_deck", "one")
    return d, run_driver(d, SIM % "analysis = kd; " + KD)


def _restated(d, an, loops):
    """kineticEnergyDistn_eval over the restart states of the given loops, float64 in bead order, accumulated into an"""
    nearest = 1.0
    for lp in loops:
        s = load_deck(str(d / "object.data"), restart_file=str(d / ("snapshot.%012d" % lp) / "restart"))
        assert s.loop == lp
        sd = an.species_dist(s.species_name)
        K = (0.5 * s.mass[s.species]) * ((s.vx * s.vx + s.vy * s.vy) + s.vz * s.vz)
        counts, tallies, stats = [], np.zeros((an.nd, 3)), np.zeros((an.nd, 3))
        for g in range(an.nd):
            Kg = K[sd[s.species] == g]
            delta = (an.emax[g] - an.emin[g]) / int(an.nbins[g])
            sub, sup = Kg < an.emin[g], Kg >= an.emax[g]
            q = (Kg[~sub & ~sup] - an.emin[g]) / delta
            # (the restart prints 14 digits of every velocity: a K within 1e-12 of an edge could change bin between the device's
            # velocity and the file's; none is that close here)
            if len(Kg):
                nearest = min(nearest, np.abs(q - np.rint(q)).min(), np.abs((Kg - an.emax[g]) / delta).min())
            counts.append(np.bincount(np.minimum(np.trunc(q).astype(np.int64), an.nbins[g] - 1), minlength=int(an.nbins[g])))
            tallies[g] = len(Kg), sub.sum(), sup.sum()
            stats[g] = (Kg.sum(), min(1e300, Kg.min()), max(0.0, Kg.max())) if len(Kg) else (0.0, 1e300, 0.0)
        an.add(np.concatenate(counts), tallies, stats)
    assert nearest > 1e-9
    return s


def test_driver_writes_kinetic_data_and_the_dist_files(one_rank, tmp_path):
    d, outs = one_rank
    assert not [l for l in outs[0][1].splitlines() if "not supported" in l]
    d0 = copy_deck(tmp_path, "water_deck", "without")
    run_driver(d0, SIM % "")
    assert open(str(d / "data"), "rb").read() == open(str(d0 / "data"), "rb").read()      # the analysis changes nothing of the run
    s0 = load_deck(str(d / "object.data"), extra_objects=SIM % "analysis = kd; " + KD)
    (a,) = s0.analysis
    an = KineticEnergyDistn(a["dist_groups"], a["eval_rate"], a["outputrate"])
    assert an.nd == 3 and list(an.species_dist(s0.species_name)) == [0, 1]
    txt = open(str(d / "kinetic.data")).read()
    lines = txt.splitlines()
    assert len(lines) == 3 and txt.endswith("\n") and lines[0] + "\n" == an.header() and txt.count("#") == 1      # one header, at start
    rows = parse_kinetic_output(txt)
    nw, nf = int((s0.species == 0).sum()), int((s0.species == 1).sum())
    for k, (lp, evals) in enumerate(((10, (5, 10)), (20, (15, 20)))):
        s = _restated(d, an, evals)
        loop, time, val = rows[k]
        assert list(loop) == [lp] * 3 and np.all(np.abs(time - s.time) <= 2e-6)      # loop and time once per group; the time in internal units
        # the startup sample (loop 0 is due) was discarded and every output cleared: two evaluations in each line, not three or four
        assert val[:, 5].tolist() == [2 * nw, 2 * nf, 0]
        want_line = an.line(lp, s.time)
        (_, _, want), = parse_kinetic_output(want_line)
        assert len(lines[1 + k]) == len(want_line) - 1
        assert np.array_equal(val[:, 3:], want[:, 3:])      # subCnt, supCnt, cntTotal
        assert want[0, 3] == 0 and want[1, 3] > 0 and want[1, 4] > 0      # both outer counts occur
        print(lp, np.abs(val[:, :3] - want[:, :3]).max(axis=0))
        assert np.all(np.abs(val[:2, 0] - want[:2, 0]) <= 1.01e-6) and np.all(np.abs(val[:2, 1:3] - want[:2, 1:3]) <= 1.01e-8)      # the digits printed
        assert val[2, 0] == 0.0 and val[2, 2] == 0.0 and val[2, 1] == want[2, 1] > 1e280      # the empty group: ave 0, max 0, min 1e300 eC
        for g in range(3):
            got_txt = open(str(d / ("snapshot.%012d" % lp) / an.filename(g))).read()
            assert got_txt.splitlines()[0] == an.dist_text(g).splitlines()[0]
            e, pdf, cnt = parse_kdist_output(got_txt)
            we, wpdf, wcnt = parse_kdist_output(an.dist_text(g))
            assert np.array_equal(cnt, wcnt) and np.array_equal(e, we) and len(cnt) == an.nbins[g]
            if g < 2:
                assert cnt.sum() == val[g, 5] - val[g, 3] - val[g, 4] and np.allclose(pdf, wpdf, rtol=1.01e-6, atol=0)
            else:
                assert np.all(np.isnan(pdf)) and not cnt.any()      # 0/0
        an.clear()
    assert not os.path.exists(str(d / ("snapshot.%012d" % 5) / an.filename(0)))      # loop 5 evaluates and writes nothing


def test_driver_two_ranks_write_the_same_files(one_rank, tmp_path):
    d1, _ = one_rank
    d2 = copy_deck(tmp_path, "water_deck", "two")
    outs = run_driver(d2, SIM % "analysis = kd; " + KD, world=2)
    assert not [l for o in outs for l in o[1].splitlines() if "not supported" in l]
    a, b = open(str(d1 / "kinetic.data")).read(), open(str(d2 / "kinetic.data")).read()
    assert a.count("#") == 1 and b.count("#") == 1      # rank 0 alone opens the file
    ra, rb = parse_kinetic_output(a), parse_kinetic_output(b)
    assert len(ra) == len(rb) == 2
    for (la, ta, va), (lb, tb, vb) in zip(ra, rb):
        assert np.array_equal(la, lb) and np.array_equal(ta, tb) and np.array_equal(va[:, 3:], vb[:, 3:])      # integer counts: any split gives the same sums
        assert np.array_equal(va[:, 1:3], vb[:, 1:3])      # minimum of minima, maximum of maxima: exact
        assert np.all(np.abs(va[:, 0] - vb[:, 0]) <= 1.01e-6)      # the sum of K is added in another order: the last printed digit may differ
    for loop in (10, 20):
        for name in ("wDist", "fDist", "none"):
            f = os.path.join("snapshot.%012d" % loop, name + "_kDist.data")
            assert open(str(d1 / f), "rb").read() == open(str(d2 / f), "rb").read(), f      # counts and their quotients only


def test_driver_mixed_list_leaves_the_other_types_files_as_they_are(tmp_path):
    sim = "simulate SIMULATE { %sdeltaloop = 20; maxloop = 20; printrate = 5; snapshotrate = 100000; checkpointrate = 100000; }\n"
    others = ("vaf ANALYSIS { type = VELOCITYAUTOCORRELATION; eval_rate = 5; length = 2; outputrate = 10; }\n"
              "vcm ANALYSIS { type = vcmWrite; outputrate = 10; }\n"
              "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 20; delta_r = 0.1 Angstrom; length = 100; }\n"
              "zden ANALYSIS { type = zdensity; outputrate = 10; nz = 16; }\n")
    mixed = copy_deck(tmp_path, "water_deck", "mixed")
    outs = run_driver(mixed, sim % "analysis = vaf vcm kd rdf zden; " + others + KD)
    assert not [l for l in outs[0][1].splitlines() if "not supported" in l]
    four = copy_deck(tmp_path, "water_deck", "four")
    run_driver(four, sim % "analysis = vaf vcm rdf zden; " + others)
    golden = set(tree_files(os.path.join(GOLDEN, "water_deck")))
    theirs = sorted(set(tree_files(four)) - golden)
    assert "vcm.data" in theirs and "snapshot.%012d/zden.dat" % 20 in theirs and "snapshot.%012d/vaf.dat" % 10 in theirs \
        and "snapshot.%012d/paircorrelation.dat" % 20 in theirs and "data" in theirs
    for f in theirs:
        assert open(str(four / f), "rb").read() == open(str(mixed / f), "rb").read(), f      # byte for byte
    new = sorted(set(tree_files(mixed)) - golden - set(theirs))
    assert new == sorted(["kinetic.data"] + ["snapshot.%012d/%s_kDist.data" % (lp, n) for lp in (10, 20) for n in ("wDist", "fDist", "none")])

"""GPU tests (-m gpu) of the ANALYSIS type FORCE_AVERAGE in the ddcmi_md driver: two objects in one deck (force and position, which
take turns on the context's one tracked list), the files' header and lines against analysis.ForceAverage driven from Python over the
same run, one rank and two ranks over the host transport on one device, the gate, and the append of a second run."""
import os

import numpy as np
import pytest

from ddcmd_amd.analysis import ForceAverage
from ddcmd_amd.deck import load_deck
from ranks import GOLDEN, copy_deck, run_driver

pytestmark = pytest.mark.gpu
SIM = "simulate SIMULATE { analysis = fF fP; deltaloop = 40; maxloop = 40; printrate = 10; snapshotrate = 100000; checkpointrate = 100000; }\n"
FA = ("fF ANALYSIS { type = FORCE_AVERAGE; idParticle = %(ids)s; eval_rate = 2; outputrate = %(out)d; }\n"
      "fP ANALYSIS { type = force_average; idParticle = %(ids)s; data_type = position; filename = pos.dat; eval_rate = 2; outputrate = %(out)d; }\n")
FILES = ("force.dat", "pos.dat")
UNIT = 1e-7      # one unit of the last printed digit (" %12.7f")


def _ids():
    gid = load_deck(os.path.join(GOLDEN, "water_deck", "object.data")).gid
    pick = [int(gid[k]) for k in (0, 17, len(gid) - 1, 17, len(gid) // 2)]      # a duplicate among them
    return pick


def _extra(out=10):
    return SIM + FA % {"ids": " ".join(str(g) for g in _ids()), "out": out}


def _python_texts(deck, outputrate=10):
    """the same run through the Python layer in the driver's batches of two steps, once per object: {filename: text}"""
    from ddcmd_amd.martini import MartiniHIP
    texts = {}
    for name, what in zip(FILES, ("force", "position")):
        s = load_deck(deck)
        m = MartiniHIP(s, constraints=s.integrator_type.upper().startswith("NGLFCONSTRAINT") and s.nresicons > 0)
        m.eval_forces()
        m.group_temperatures()
        an = ForceAverage(_ids(), what, eval_rate=2, outputrate=outputrate)
        text = an.header()
        an.sample(m)      # the startup sample (loop 0 is due), discarded
        an.clear()
        time = s.time
        for loop in range(2, 41, 2):
            m.step(2)
            m.energies()
            m.group_temperatures()
            time += s.dt; time += s.dt      # the sum the driver forms step by step
            an.sample(m)
            if loop % outputrate == 0:
                text += an.line(loop, time) or ""
        m.close()
        texts[name] = text
    return texts


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    d = copy_deck(tmp_path_factory.mktemp("track1"), "water_deck", "one")
    return d, run_driver(d, _extra())


def test_one_rank_writes_what_python_writes_character_for_character(one_rank, tmp_path):
    d, outs = one_rank
    assert not [l for l in outs[0].stderr.splitlines() if "not supported" in l]
    want = _python_texts(str(d / "object.data"))
    for name in FILES:
        got = open(str(d / name)).read()
        assert got.count("\n") == 5 and got.splitlines()[0] == "# loop  time  " + "".join("%d  " % g for g in _ids())
        assert [l[:12] for l in got.splitlines()[1:]] == ["%012d" % k for k in (10, 20, 30, 40)]
        assert got == want[name], name
    rows = np.array([[float(x) for x in l.split()[2:]] for l in open(str(d / "pos.dat")).read().splitlines()[1:]])
    assert np.array_equal(rows[:, 3:6], rows[:, 9:12]) and np.any(rows != 0.0)      # the duplicate gets equal values
    d0 = copy_deck(tmp_path, "water_deck", "without")
    run_driver(d0, SIM.replace("analysis = fF fP; ", ""))
    assert open(str(d / "data"), "rb").read() == open(str(d0 / "data"), "rb").read()      # the analyses change nothing of the run


def test_two_ranks_agree_to_the_printed_digits(one_rank, tmp_path):
    """The two ranks' partial sums are added in rank order: a sum of up to 5 samples in two parts rounds up to 5 + 2 times, a relative
    2^-53 of the magnitudes each, so a printed mean can differ from the one-rank file by at most 7 * 2^-53 * |mean| * (5 / 1): far
    below 1e-7.  A field may therefore differ only by one unit of the last printed digit, and only where the one-rank value lies that
    close to a rounding boundary (k + 0.5) 1e-7 -- a closer cap than the 1e-7 such a field needs in any case."""
    d1, _ = one_rank
    d2 = copy_deck(tmp_path, "water_deck", "two")
    outs = run_driver(d2, _extra(), world=2)
    assert not [l for o in outs for l in o.stderr.splitlines() if "not supported" in l]
    differed = near = 0
    for name in FILES:
        a, b = open(str(d1 / name)).read().splitlines(), open(str(d2 / name)).read().splitlines()
        assert len(a) == len(b) == 5 and a[0] == b[0]
        for la, lb in zip(a[1:], b[1:]):
            fa, fb = la.split(), lb.split()
            assert fa[:2] == fb[:2] and len(fa) == len(fb) == 2 + 3 * 5
            for x, y in zip(fa[2:], fb[2:]):
                v = float(x)
                width = 7 * 2.0 ** -53 * 5 * max(abs(v), UNIT) + 1e-22
                t = abs(v) / UNIT
                on_edge = abs(t - np.floor(t) - 0.5) * UNIT <= width + 2.0 ** -52 * abs(v)      # (and the rounding of t itself)
                near += on_edge
                if x != y:
                    differed += 1
                    assert abs(float(x) - float(y)) <= 1.01 * UNIT and on_edge, (name, x, y)
    print("fields that differ between one rank and two: %d; fields on a rounding boundary: %d" % (differed, near))
    assert differed <= near


def test_the_gate_and_the_append_of_a_second_run(tmp_path):
    """outputrate 5, eval_rate 2: the outputs of loops 5, 15, 25, 35 find the two samples of the loops before them, 4 < 5, and neither
    write nor clear; those of loops 10, 20, 30, 40 find five samples each.  A second run in the same directory appends."""
    d = copy_deck(tmp_path, "water_deck", "gate")
    extra = _extra(5)
    run_driver(d, extra)
    got = open(str(d / "force.dat")).read()
    assert [l[:12] for l in got.splitlines()[1:]] == ["%012d" % k for k in (10, 20, 30, 40)]      # 5, 15, 25, 35: gated (4 < 5)
    first = {name: open(str(d / name)).read() for name in FILES}
    run_driver(d, extra)      # the same deck again: the files are opened for append
    for name in FILES:
        now = open(str(d / name)).read()
        assert now.startswith(first[name]) and now[len(first[name]):].startswith(first[name].splitlines()[0] + "\n")
        assert now.count("# loop  time") == 2

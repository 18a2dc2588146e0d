"""CPU tests: the deck loader reads ANALYSIS objects of the type FORCE_AVERAGE (forceAverage.c:28-73) -- the head match in any case,
idParticle in the deck's order with duplicates kept, the defaults of forceAverage_parms, each data_type -- and refuses at load what
the reference leaves to an abort, an exit or a receive that never returns."""
import os
import shutil

import numpy as np
import pytest

from ddcmd_amd import _lib
from ddcmd_amd.deck import load_deck

HERE = os.path.dirname(os.path.abspath(__file__))
WATER = os.path.join(HERE, "golden", "water_deck")
HEAD = "simulate SIMULATE { analysis = %s; }\n"


@pytest.fixture(scope="module")
def deck(tmp_path_factory):
    d = tmp_path_factory.mktemp("track") / "deck"
    shutil.copytree(WATER, str(d))
    return str(d / "object.data")


@pytest.fixture(scope="module")
def gids(deck):
    return [int(g) for g in load_deck(deck).gid]


def test_heads_order_duplicates_and_defaults(deck, gids):
    a, b, c = gids[5], gids[0], gids[-1]
    extra = (HEAD % "fa fb fc"
             + "fa ANALYSIS { type = FORCE_AVERAGE; idParticle = %d %d %d %d; }\n" % (a, b, a, c)
             + "fb ANALYSIS { type = force_averageFoo; idParticle = %d; data_type = Velocity; eval_rate = 2; outputrate = 10; filename = v.dat; }\n" % c
             + "fc ANALYSIS { type = Force_Average; idParticle = %d %d; data_type = POSITION; }\n" % (b, a))
    fa, fb, fc = load_deck(deck, extra_objects=extra).analysis
    assert fa["supported"] and fb["supported"] and fc["supported"]
    assert fa["gids"].dtype == np.uint64 and list(fa["gids"]) == [a, b, a, c]      # the deck's order, the duplicate kept
    assert (fa["data_type"], fa["filename"], fa["eval_rate"], fa["outputrate"]) == ("force", "force.dat", 1, 1)      # forceAverage_parms' defaults
    assert (fb["data_type"], fb["filename"], fb["eval_rate"], fb["outputrate"]) == ("velocity", "v.dat", 2, 10) and list(fb["gids"]) == [c]
    assert fc["data_type"] == "position" and list(fc["gids"]) == [b, a] and fc["type"] == "Force_Average"
    assert _lib.AN_FORCEAVERAGE == 10      # enum ddcmi_analysis_kind: the row behind cholAnalysis


def test_the_head_must_match(deck, gids):
    s = load_deck(deck, extra_objects=HEAD % "fa" + "fa ANALYSIS { type = FORCEAVERAGE; idParticle = %d; }\n" % gids[0])
    assert not s.analysis[0]["supported"]


@pytest.mark.parametrize("keys, message", [
    ("", "fa: no idParticle key"),                                                       # ABORT_IF_NOT_FOUND
    ("idParticle = %(g)d; data_type = momentum;", "fa: data_type = momentum is none of force, velocity, position"),      # exit(19) at the first evaluation
    ("idParticle = %(g)d %(missing)d;", "fa: idParticle names gid %(missing)d, and no atom of the collection carries it"),      # MPI_Recv for ever
    ("idParticle = %(g)d; eval_rate = 0;", "fa: eval_rate = 0, it must be at least 1"),
    ("idParticle = %(g)d; eval_rate = -3;", "fa: eval_rate = -3, it must be at least 1"),
])
def test_refusals_name_the_object(deck, gids, keys, message):
    v = {"g": gids[3], "missing": max(gids) + 12345}
    with pytest.raises(RuntimeError, match="ANALYSIS " + message % v):
        load_deck(deck, extra_objects=HEAD % "fa" + "fa ANALYSIS { type = FORCE_AVERAGE; %s }\n" % (keys % v))


def test_more_ids_than_the_cap_are_refused(deck, gids):
    cap = 1 << 20
    ids = " ".join([str(gids[0])] * (cap + 1))      # duplicates are legal, so one gid serves
    with pytest.raises(RuntimeError, match="ANALYSIS fa: idParticle lists %d gids, the device tracks at most %d" % (cap + 1, cap)):
        load_deck(deck, extra_objects=HEAD % "fa" + "fa ANALYSIS { type = FORCE_AVERAGE; idParticle = %s; }\n" % ids)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ddcmi.h")).read()
    assert "#define DDCMI_TRACK_MAX_IDS (1 << 20)" in header

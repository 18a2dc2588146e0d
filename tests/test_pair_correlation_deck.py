"""CPU tests: the deck loader reads SIMULATE `analysis` and its ANALYSIS objects (analysis.c:120-160, paircorrelation.c:68-135) --
units, defaults, a list of two analyses, an unknown type, the refusals."""
import os
import shutil

import pytest

from ddcmd_amd.deck import load_deck, units_convert

HERE = os.path.dirname(os.path.abspath(__file__))
WATER = os.path.join(HERE, "golden", "water_deck")


def _deck(tmp_path, extra):
    d = tmp_path / "deck"
    shutil.copytree(WATER, str(d))
    return str(d / "object.data"), extra


def test_two_analyses_units_and_defaults(tmp_path):
    obj, _ = _deck(tmp_path, None)
    extra = ("simulate SIMULATE { analysis = rdf writeCharmm; }\n"
             "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 50; delta_r = 0.1 Angstrom; length = 100; }\n"
             "writeCharmm ANALYSIS { type = subsetWrite; outputrate = 1000; }\n")
    s = load_deck(obj, extra_objects=extra)
    assert [a["name"] for a in s.analysis] == ["rdf", "writeCharmm"]
    rdf, other = s.analysis
    assert rdf["supported"] and rdf["type"] == "PAIRCORRELATION" and rdf["eval_rate"] == 10 and rdf["outputrate"] == 50
    assert rdf["length"] == 100 and abs(rdf["delta_r"] - units_convert(0.1, "Angstrom", None)) < 1e-15 and rdf["rmin"] == 0.0
    assert rdf["filename"] == "paircorrelation.dat" and rdf["rscale"] == "normal" and rdf["method"] == "geom"
    assert not other["supported"] and other["type"] == "subsetWrite" and other["eval_rate"] == 0 and other["outputrate"] == 1000


def test_prefix_match_log_scale_and_method(tmp_path):
    obj, _ = _deck(tmp_path, None)
    extra = ("simulate SIMULATE { analysis = g; }\n"
             "g ANALYSIS { type = paircorrelationX; rmin = 0.2 nm; delta_r = 0.5 Angstrom; length = 20; rscale = log; method = neighborList;"
             " filename = gofr.dat; }\n")
    (a,) = load_deck(obj, extra_objects=extra).analysis
    assert a["supported"] and a["rscale"] == "log" and a["method"] == "neighborList" and a["filename"] == "gofr.dat"
    assert abs(a["rmin"] - units_convert(2.0, "Angstrom", None)) < 1e-12 and a["eval_rate"] == 0 and a["outputrate"] == 0


def test_no_analysis_key(tmp_path):
    obj, _ = _deck(tmp_path, None)
    assert load_deck(obj).analysis == []


@pytest.mark.parametrize("body,msg", [("type = PAIRCORRELATION; rscale = cubic;", "rscale"), ("type = PAIRCORRELATION; method = fast;", "method"),
                                      ("type = PAIRCORRELATION; rscale = log;", "rmin > 0")])
def test_bad_parameters_are_refused(tmp_path, body, msg):
    obj, _ = _deck(tmp_path, None)
    with pytest.raises(RuntimeError, match=msg):
        load_deck(obj, extra_objects="simulate SIMULATE { analysis = g; }\ng ANALYSIS { %s }\n" % body)


def test_missing_analysis_object_is_refused(tmp_path):
    obj, _ = _deck(tmp_path, None)
    with pytest.raises(RuntimeError, match="ANALYSIS nothere not found"):
        load_deck(obj, extra_objects="simulate SIMULATE { analysis = nothere; }\n")

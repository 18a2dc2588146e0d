"""CPU tests: the deck loader reads ANALYSIS objects of type VELOCITYAUTOCORRELATION (velocityAutocorrelation.c:59-60; the prefix
match of analysis.c:178) -- keys, defaults, the refusal of length < 1 -- and still reports other types as not supported."""
import os
import shutil

import pytest

from ddcmd_amd.deck import load_deck, units_convert

HERE = os.path.dirname(os.path.abspath(__file__))
WATER = os.path.join(HERE, "golden", "water_deck")


def _deck(tmp_path):
    d = tmp_path / "deck"
    shutil.copytree(WATER, str(d))
    return str(d / "object.data")


def test_keys_defaults_and_neighbours_in_the_list(tmp_path):
    extra = ("simulate SIMULATE { analysis = vaf rdf writeCharmm; }\n"
             "vaf ANALYSIS { type = VELOCITYAUTOCORRELATION; eval_rate = 5; length = 4; outputrate = 40; }\n"
             "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 50; delta_r = 0.1 Angstrom; length = 100; }\n"
             "writeCharmm ANALYSIS { type = subsetWrite; outputrate = 1000; }\n")
    vaf, rdf, other = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert vaf == {"name": "vaf", "type": "VELOCITYAUTOCORRELATION", "eval_rate": 5, "outputrate": 40, "supported": True, "filename": "vaf.dat", "length": 4}
    assert rdf["supported"] and rdf["length"] == 100 and rdf["filename"] == "paircorrelation.dat" and "delta_r" in rdf
    assert not other["supported"] and other["type"] == "subsetWrite" and "length" not in other and "filename" not in other


def test_prefix_match_any_case_default_length_and_filename(tmp_path):
    extra = ("simulate SIMULATE { analysis = d; }\n"
             "d ANALYSIS { type = velocityAutocorrelationOfLipids; eval_rate = 2; filename = diffusion.dat; }\n")
    (a,) = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert a["supported"] and a["length"] == 1 and a["filename"] == "diffusion.dat" and a["eval_rate"] == 2 and a["outputrate"] == 0
    assert "delta_r" not in a and "rscale" not in a


@pytest.mark.parametrize("length", [0, -3])
def test_length_below_one_is_refused(tmp_path, length):
    with pytest.raises(RuntimeError, match="ANALYSIS v: length = %d" % length):
        load_deck(_deck(tmp_path), extra_objects="simulate SIMULATE { analysis = v; }\nv ANALYSIS { type = VELOCITYAUTOCORRELATION; length = %d; }\n" % length)


def test_other_types_stay_unsupported(tmp_path):
    extra = ("simulate SIMULATE { analysis = a b; }\na ANALYSIS { type = subsetWrite; }\nb ANALYSIS { type = VELOCITY; }\n")
    a, b = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert not a["supported"] and not b["supported"]      # (a shorter word is no prefix match)


def test_mixed_list_keeps_each_objects_own_parameters(tmp_path):
    """two PAIRCORRELATION objects of different length and rscale round a subsetWrite and a VELOCITYAUTOCORRELATION object: four dicts in
    list order, and nothing of a neighbour's record shows in another's"""
    extra = ("simulate SIMULATE { analysis = rdf writeCharmm vaf rdf2; }\n"
             "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 50; delta_r = 0.1 Angstrom; length = 100; }\n"
             "writeCharmm ANALYSIS { type = subsetWrite; outputrate = 1000; }\n"
             "vaf ANALYSIS { type = VELOCITYAUTOCORRELATION; eval_rate = 5; length = 4; outputrate = 40; }\n"
             "rdf2 ANALYSIS { type = PAIRCORRELATION; eval_rate = 20; outputrate = 60; rmin = 1 Angstrom; delta_r = 0.5 Angstrom; length = 30;"
             " rscale = log; method = grid; filename = gofr.dat; }\n")
    rdf, other, vaf, rdf2 = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    ang = units_convert(1.0, "Angstrom", None)
    assert rdf == {"name": "rdf", "type": "PAIRCORRELATION", "eval_rate": 10, "outputrate": 50, "supported": True, "filename": "paircorrelation.dat",
                   "length": 100, "delta_r": rdf["delta_r"], "rmin": 0.0, "rscale": "normal", "method": "geom"}
    assert abs(rdf["delta_r"] - 0.1 * ang) < 1e-15
    assert other == {"name": "writeCharmm", "type": "subsetWrite", "eval_rate": 0, "outputrate": 1000, "supported": False}
    assert vaf == {"name": "vaf", "type": "VELOCITYAUTOCORRELATION", "eval_rate": 5, "outputrate": 40, "supported": True, "filename": "vaf.dat", "length": 4}
    assert rdf2 == {"name": "rdf2", "type": "PAIRCORRELATION", "eval_rate": 20, "outputrate": 60, "supported": True, "filename": "gofr.dat",
                    "length": 30, "delta_r": rdf2["delta_r"], "rmin": rdf2["rmin"], "rscale": "log", "method": "grid"}
    assert abs(rdf2["delta_r"] - 0.5 * ang) < 1e-15 and abs(rdf2["rmin"] - ang) < 1e-15

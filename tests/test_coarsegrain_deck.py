"""CPU tests: the deck loader reads ANALYSIS objects of the type COARSEGRAIN (matched by its head in any case, analysis.c:162 of the
reference) -- keys, defaults and units of coarsegrain_parms (coarsegrain.c:80-119) -- refuses with a message what the reference leaves
to a division by zero, an abort or an assert, and leaves an object with outputMode = 3 (E = f / q) unsupported."""
import os
import shutil

import pytest

from ddcmd_amd.deck import load_deck, units_convert

HERE = os.path.dirname(os.path.abspath(__file__))
WATER = os.path.join(HERE, "golden", "water_deck")      # two species
SIM = "simulate SIMULATE { analysis = cg; }\n"
UNITS = "field_units = 1 1 1 1 amu eV eV eV eV eV amu*Angstrom/fs amu*Angstrom/fs amu*Angstrom/fs;"


def _load(tmp_path, body, word="COARSEGRAIN"):
    d = tmp_path / "deck"
    if not d.exists():
        shutil.copytree(WATER, str(d))
    return load_deck(str(d / "object.data"), extra_objects=SIM + "cg ANALYSIS { type = %s; %s }\n" % (word, body))


def test_defaults(tmp_path):
    (d,) = _load(tmp_path, "nx = 4; ny = 5; nz = 6; eval_rate = 2; outputrate = 6; " + UNITS).analysis
    assert d == {"name": "cg", "type": "COARSEGRAIN", "eval_rate": 2, "outputrate": 6, "supported": True, "filename": "cgrid", "length": 1,
                 "nx": 4, "ny": 5, "nz": 6, "output_mode": 2, "nfiles": 0, "smear_radius": 0.0, "smear_method": "impulse"}


def test_every_key_with_its_unit(tmp_path):
    (d,) = _load(tmp_path, "nx = 64; ny = 1; nz = 2; filename = rho; outputMode = 1; nfiles = 8; smearRadius = 0.3 nm; smearMethod = HaT; eval_rate = 10; outputrate = 100; " + UNITS).analysis
    assert (d["nx"], d["ny"], d["nz"], d["filename"], d["output_mode"], d["nfiles"], d["smear_method"]) == (64, 1, 2, "rho", 1, 8, "hat")
    assert d["smear_radius"] == pytest.approx(units_convert(3.0, "Angstrom", None), rel=1e-14)
    (d,) = _load(tmp_path, "nx = 1; ny = 1; nz = 1; smearRadius = 2.5; smearMethod = gaussian; " + UNITS).analysis
    assert d["smear_radius"] == pytest.approx(units_convert(2.5, "l", None), rel=1e-14) and d["smear_method"] == "impulse"      # anything else is impulse


@pytest.mark.parametrize("word", ["COARSEGRAIN", "coarsegrain", "CoarseGrain", "coarsegrainFoo", "COARSEGRAIN2"])
def test_the_head_matches_in_any_case(tmp_path, word):
    (d,) = _load(tmp_path, "nx = 2; ny = 2; nz = 2; " + UNITS, word).analysis
    assert d["supported"] and d["type"] == word and d["nx"] == 2


@pytest.mark.parametrize("word", ["COARSEGRAI", "xCOARSEGRAIN", "COARSE_GRAIN", "cgrid"])
def test_other_words_do_not_match(tmp_path, word):
    (d,) = _load(tmp_path, "nx = 2; ny = 2; nz = 2; outputrate = 5; " + UNITS, word).analysis
    assert d == {"name": "cg", "type": word, "eval_rate": 0, "outputrate": 5, "supported": False}


@pytest.mark.parametrize("body,message", [
    ("ny = 2; nz = 2; " + UNITS, "ANALYSIS cg: nx = 0, ny = 2, nz = 2: each must be at least 1"),      # the reference's default 0 divides by zero
    ("nx = 2; ny = -3; nz = 2; " + UNITS, "ANALYSIS cg: nx = 2, ny = -3, nz = 2: each must be at least 1"),
    ("nx = 2; ny = 2; nz = 0; " + UNITS, "ANALYSIS cg: nx = 2, ny = 2, nz = 0: each must be at least 1"),
    ("nx = 2; ny = 2; nz = 2;", "ANALYSIS cg: no field_units key"),                                   # the reference aborts
    ("nx = 2; ny = 2; nz = 2; outputMode = 0; " + UNITS, r"ANALYSIS cg: outputMode = 0 \(1, 2 or 3\)"),
    ("nx = 2; ny = 2; nz = 2; outputMode = 4; " + UNITS, r"ANALYSIS cg: outputMode = 4 \(1, 2 or 3\)"),
    ("nx = 1024; ny = 1024; nz = 129; " + UNITS, "ANALYSIS cg: 1024 x 1024 x 129 cells x 2 species = 270532608 keys, the device takes at most 268435456"),
    ("nx = 100000; ny = 100000; nz = 100000; " + UNITS, "ANALYSIS cg: 100000 x 100000 x 100000 cells, the device takes at most 268435456 keys"),
])
def test_refusals(tmp_path, body, message):
    with pytest.raises(RuntimeError, match=message):
        _load(tmp_path, body)


def test_the_largest_key_space_loads(tmp_path):
    (d,) = _load(tmp_path, "nx = 1024; ny = 1024; nz = 128; " + UNITS).analysis      # x 2 species = 2^28
    assert d["supported"] and d["nz"] == 128


def test_output_mode_3_is_ignored(tmp_path):
    """E = f / q divides by the species' charge: the object stays unsupported, whatever else it says -- a grid the supported modes refuse included"""
    (d,) = _load(tmp_path, "nx = 0; outputMode = 3; outputrate = 7;").analysis
    assert d == {"name": "cg", "type": "COARSEGRAIN", "eval_rate": 0, "outputrate": 7, "supported": False}

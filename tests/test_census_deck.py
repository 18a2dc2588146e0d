"""CPU tests: the deck loader reads ANALYSIS objects of the types vcmWrite (vcmWrite.c:23-31) and zdensity (zdensity.c:36-50) -- keys,
defaults, the full-name match of analysis.c:240,317 in any case, the refusal of nz < 1 -- and still reports other types as not
supported."""
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


def test_defaults(tmp_path):
    extra = ("simulate SIMULATE { analysis = vcm zden; }\n"
             "vcm ANALYSIS { type = vcmWrite; outputrate = 100; }\n"
             "zden ANALYSIS { type = zdensity; outputrate = 1000; nz = 100; }\n")
    vcm, zden = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert vcm == {"name": "vcm", "type": "vcmWrite", "eval_rate": 0, "outputrate": 100, "supported": True, "filename": "vcm.data", "length": 1}
    assert zden == {"name": "zden", "type": "zdensity", "eval_rate": 0, "outputrate": 1000, "supported": True, "filename": "zden.dat", "length": 1,
                    "nz": 100, "smear_radius": 0.0, "smear_method": "impulse"}


def test_every_key_set(tmp_path):
    extra = ("simulate SIMULATE { analysis = vcm zden; }\n"
             "vcm ANALYSIS { type = vcmWrite; eval_rate = 3; outputrate = 7; filename = drift.data; }\n"
             "zden ANALYSIS { type = zdensity; eval_rate = 2; outputrate = 50; nz = 250; filename = profile.dat; smearRadius = 2.5 Angstrom; smearMethod = HAT; }\n")
    vcm, zden = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert vcm["filename"] == "drift.data" and vcm["eval_rate"] == 3 and vcm["outputrate"] == 7 and "nz" not in vcm
    assert zden["filename"] == "profile.dat" and zden["nz"] == 250 and zden["smear_method"] == "hat" and zden["eval_rate"] == 2 and zden["outputrate"] == 50
    assert abs(zden["smear_radius"] - 2.5 * units_convert(1.0, "Angstrom", None)) < 1e-14


@pytest.mark.parametrize("word,method", [("impulse", "impulse"), ("hat", "hat"), ("Hat", "hat"), ("gaussian", "impulse")])
def test_smear_method_words(tmp_path, word, method):
    extra = "simulate SIMULATE { analysis = z; }\nz ANALYSIS { type = zdensity; nz = 4; smearMethod = %s; }\n" % word
    (z,) = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert z["smear_method"] == method      # anything but hat is impulse, as the reference reads it


@pytest.mark.parametrize("word,kind", [("vcmWrite", "vcm"), ("vcm_write", "vcm"), ("VCMWRITE", "vcm"), ("VCM_Write", "vcm"), ("zdensity", "zd"), ("ZDensity", "zd"), ("ZDENSITY", "zd")])
def test_spellings_in_any_case(tmp_path, word, kind):
    extra = "simulate SIMULATE { analysis = a; }\na ANALYSIS { type = %s; nz = 8; }\n" % word
    (a,) = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert a["supported"] and a["type"] == word
    assert a["filename"] == ("vcm.data" if kind == "vcm" else "zden.dat") and ("nz" in a) == (kind == "zd")


@pytest.mark.parametrize("word", ["zdensityX", "zdensityFoo", "vcm", "vcmWriter", "vcm_write2", "zdens", "vcmwrit"])
def test_no_prefix_match_for_these_two(tmp_path, word):
    extra = "simulate SIMULATE { analysis = a; }\na ANALYSIS { type = %s; nz = 8; }\n" % word
    (a,) = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert not a["supported"] and "filename" not in a and "nz" not in a


def test_prefix_rows_keep_matching_by_prefix(tmp_path):
    extra = ("simulate SIMULATE { analysis = a b; }\na ANALYSIS { type = paircorrelationFunction; delta_r = 0.1 Angstrom; length = 10; }\n"
             "b ANALYSIS { type = velocityAutocorrelationOfLipids; }\n")
    a, b = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    assert a["supported"] and "delta_r" in a and b["supported"] and b["filename"] == "vaf.dat"


@pytest.mark.parametrize("nz", [0, -5])
def test_nz_below_one_is_refused_with_the_objects_name(tmp_path, nz):
    with pytest.raises(RuntimeError, match="ANALYSIS profile: nz = %d" % nz):
        load_deck(_deck(tmp_path), extra_objects="simulate SIMULATE { analysis = profile; }\nprofile ANALYSIS { type = zdensity; nz = %d; }\n" % nz)


def test_nz_defaults_to_zero_and_is_refused(tmp_path):
    with pytest.raises(RuntimeError, match="ANALYSIS z: nz = 0"):
        load_deck(_deck(tmp_path), extra_objects="simulate SIMULATE { analysis = z; }\nz ANALYSIS { type = zdensity; }\n")


def test_mixed_list_of_all_four_types_and_an_unsupported_one(tmp_path):
    extra = ("simulate SIMULATE { analysis = vaf vcm writeCharmm rdf zden; }\n"
             "vaf ANALYSIS { type = VELOCITYAUTOCORRELATION; eval_rate = 5; length = 4; outputrate = 40; }\n"
             "vcm ANALYSIS { type = vcmWrite; outputrate = 100; }\n"
             "writeCharmm ANALYSIS { type = subsetWrite; outputrate = 1000; }\n"
             "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 50; delta_r = 0.1 Angstrom; length = 100; }\n"
             "zden ANALYSIS { type = zdensity; outputrate = 200; nz = 64; smearRadius = 1 Angstrom; smearMethod = hat; }\n")
    vaf, vcm, other, rdf, zden = load_deck(_deck(tmp_path), extra_objects=extra).analysis
    ang = units_convert(1.0, "Angstrom", None)
    assert vaf == {"name": "vaf", "type": "VELOCITYAUTOCORRELATION", "eval_rate": 5, "outputrate": 40, "supported": True, "filename": "vaf.dat", "length": 4}
    assert vcm == {"name": "vcm", "type": "vcmWrite", "eval_rate": 0, "outputrate": 100, "supported": True, "filename": "vcm.data", "length": 1}
    assert other == {"name": "writeCharmm", "type": "subsetWrite", "eval_rate": 0, "outputrate": 1000, "supported": False}
    assert rdf == {"name": "rdf", "type": "PAIRCORRELATION", "eval_rate": 10, "outputrate": 50, "supported": True, "filename": "paircorrelation.dat",
                   "length": 100, "delta_r": rdf["delta_r"], "rmin": 0.0, "rscale": "normal", "method": "geom"}
    assert abs(rdf["delta_r"] - 0.1 * ang) < 1e-15
    assert zden == {"name": "zden", "type": "zdensity", "eval_rate": 0, "outputrate": 200, "supported": True, "filename": "zden.dat", "length": 1,
                    "nz": 64, "smear_radius": zden["smear_radius"], "smear_method": "hat"}
    assert abs(zden["smear_radius"] - ang) < 1e-15

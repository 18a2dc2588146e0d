"""CPU tests: the deck loader reads ANALYSIS objects of the type KINETICENERGYDISTN (kineticEnergyDistn.c:45-93) with the BIN
objects their distGroups name -- keys, defaults, units, the prefix match of analysis.c:154 in any case, the refusals -- and leaves
the dicts of the other types as they are."""
import os
import shutil

import pytest

from ddcmd_amd.deck import load_deck, units_convert

HERE = os.path.dirname(os.path.abspath(__file__))
WATER = os.path.join(HERE, "golden", "water_deck")      # species WxW and WFxWF
MAX_LDS = 65536      # DDCMI_KDIST_MAX_LDS: 4 B per bin and 108 B per group of one workgroup's LDS


def _deck(tmp_path):
    d = tmp_path / "deck"
    if not d.exists():
        shutil.copytree(WATER, str(d))
    return str(d / "object.data")


def _load(tmp_path, extra):
    return load_deck(_deck(tmp_path), extra_objects=extra).analysis


def test_keys_and_defaults(tmp_path):
    extra = ("simulate SIMULATE { analysis = kd; }\n"
             "kd ANALYSIS { type = KINETICENERGYDISTN; eval_rate = 10; outputrate = 100; distGroups = wDist fDist; }\n"
             "wDist BIN { species = WxW; emin = 0 eV; emax = 0.2 eV; nBins = 100; }\n"
             "fDist BIN { species = WFxWF; emax = 1; }\n")
    (kd,) = _load(tmp_path, extra)
    ev = units_convert(1.0, "eV", None)
    assert kd == {"name": "kd", "type": "KINETICENERGYDISTN", "eval_rate": 10, "outputrate": 100, "supported": True, "filename": "kinetic.data", "length": 1,
                  "dist_groups": [{"name": "wDist", "species": "WxW", "emin": 0.0, "emax": kd["dist_groups"][0]["emax"], "nbins": 100},
                                  {"name": "fDist", "species": "WFxWF", "emin": 0.0, "emax": 1.0, "nbins": 1}]}      # emin "0", nBins 1
    assert abs(kd["dist_groups"][0]["emax"] - 0.2 * ev) <= 1e-15 * ev


def test_no_dist_groups_is_an_analysis_of_zero_groups(tmp_path):
    (kd,) = _load(tmp_path, "simulate SIMULATE { analysis = kd; }\nkd ANALYSIS { type = KINETICENERGYDISTN; outputrate = 5; }\n")
    assert kd["supported"] and kd["dist_groups"] == []


def test_units(tmp_path):
    extra = ("simulate SIMULATE { analysis = kd; }\nkd ANALYSIS { type = KINETICENERGYDISTN; distGroups = a b c; }\n"
             "a BIN { species = WxW; emin = 0.01 eV; emax = 0.2 eV; nBins = 5; }\n"
             "b BIN { species = WFxWF; emin = 0.0003; emax = 0.0125; nBins = 5; }\n"      # bare numbers: the default unit "energy", internal units
             "c BIN { species = other; emin = 1 kJ/mol; emax = 10 kJ*mol^-1; nBins = 3; }\n")
    a, b, c = _load(tmp_path, extra)[0]["dist_groups"]
    ev, kjmol = units_convert(1.0, "eV", None), units_convert(1.0, "kJ/mol", None)
    assert abs(a["emin"] - 0.01 * ev) <= 1e-15 * ev and abs(a["emax"] - 0.2 * ev) <= 1e-15 * ev
    assert b["emin"] == 0.0003 and b["emax"] == 0.0125      # as written, to the bit
    assert abs(c["emin"] - kjmol) <= 1e-15 * kjmol and abs(c["emax"] - 10 * kjmol) <= 1e-14 * kjmol
    assert abs(kjmol / ev - 0.0103642697) < 1e-9      # 1 kJ/mol = 0.010364 eV
    assert units_convert(2.5, "energy", None) == 2.5 and units_convert(2.5, None, "energy") == 2.5
    assert c["species"] == "other" and c["nbins"] == 3      # a BIN of a species the deck lacks loads (and stays empty)


@pytest.mark.parametrize("word", ["KINETICENERGYDISTN", "kineticEnergyDistn", "kineticenergydistn", "kineticEnergyDistnFoo", "KineticEnergyDistnOfWater"])
def test_prefix_match_in_any_case(tmp_path, word):
    extra = "simulate SIMULATE { analysis = kd; }\nkd ANALYSIS { type = %s; distGroups = w; }\nw BIN { species = WxW; emax = 1; }\n" % word
    (kd,) = _load(tmp_path, extra)
    assert kd["supported"] and kd["type"] == word and len(kd["dist_groups"]) == 1


@pytest.mark.parametrize("word", ["KINETICENERGY", "kineticEnergyDist", "KINETICENERGYDIST_N", "xKINETICENERGYDISTN"])
def test_shorter_or_other_words_do_not_match(tmp_path, word):
    extra = "simulate SIMULATE { analysis = kd; }\nkd ANALYSIS { type = %s; distGroups = w; }\nw BIN { species = WxW; emax = 1; }\n" % word
    (kd,) = _load(tmp_path, extra)
    assert kd == {"name": "kd", "type": word, "eval_rate": 0, "outputrate": 0, "supported": False}


HEAD = "simulate SIMULATE { analysis = kd; }\nkd ANALYSIS { type = KINETICENERGYDISTN; distGroups = %s; }\n"


@pytest.mark.parametrize("objects,message", [
    (HEAD % "w nobody" + "w BIN { species = WxW; emax = 1; }\n", r"ANALYSIS kd: distGroups names nobody, and there is no BIN object of that name"),
    (HEAD % "w" + "w NIB { species = WxW; emax = 1; }\n", r"ANALYSIS kd: distGroups names w, and there is no BIN object of that name"),
    (HEAD % "w" + "w BIN { species = WxW; emax = 1; nBins = 0; }\n", r"ANALYSIS kd: BIN w: nBins = 0"),
    (HEAD % "w" + "w BIN { species = WxW; emax = 1; nBins = -4; }\n", r"ANALYSIS kd: BIN w: nBins = -4"),
    (HEAD % "w" + "w BIN { species = WxW; emin = 0.5; emax = 0.5; }\n", r"ANALYSIS kd: BIN w: emax = 0.5 <= emin = 0.5"),
    (HEAD % "w" + "w BIN { species = WxW; emin = 2 eV; emax = 1 eV; }\n", r"ANALYSIS kd: BIN w: emax = \S+ <= emin = \S+"),
    (HEAD % "w" + "w BIN { species = WxW; }\n", r"ANALYSIS kd: BIN w: emax = 0 <= emin = 0"),      # both default to "0"
    (HEAD % "w f again" + "w BIN { species = WxW; emax = 1; }\nf BIN { species = WFxWF; emax = 1; }\nagain BIN { species = WxW; emax = 2; }\n",
     r"ANALYSIS kd: species WxW is claimed by BIN w and by BIN again"),
    (HEAD % "w" + "w BIN { species = WxW; emax = 1; nBins = %d; }\n" % ((MAX_LDS - 108) // 4 + 1), r"ANALYSIS kd: 16358 bins in 1 groups need 65540 bytes of the device's LDS, at most 65536"),
    (HEAD % "w f" + "w BIN { species = WxW; emax = 1; nBins = 8192; }\nf BIN { species = WFxWF; emax = 1; nBins = 8139; }\n",
     r"ANALYSIS kd: 16331 bins in 2 groups need 65540 bytes of the device's LDS, at most 65536"),
])
def test_refusals_by_message(tmp_path, objects, message):
    with pytest.raises(RuntimeError, match=message):
        _load(tmp_path, objects)


def test_the_largest_histograms_load(tmp_path):
    one = (MAX_LDS - 108) // 4      # 16357
    (kd,) = _load(tmp_path, HEAD % "w" + "w BIN { species = WxW; emax = 1; nBins = %d; }\n" % one)
    assert kd["dist_groups"][0]["nbins"] == one == 16357
    (kd,) = _load(tmp_path, HEAD % "w f" + "w BIN { species = WxW; emax = 1; nBins = 8192; }\nf BIN { species = WFxWF; emax = 1; nBins = 8138; }\n")
    assert [g["nbins"] for g in kd["dist_groups"]] == [8192, 8138] and 4 * (8192 + 8138) + 2 * 108 == MAX_LDS


def test_mixed_list_leaves_the_other_types_dicts_as_they_are(tmp_path):
    extra = ("simulate SIMULATE { analysis = vaf vcm writeCharmm kd rdf zden; }\n"
             "vaf ANALYSIS { type = VELOCITYAUTOCORRELATION; eval_rate = 5; length = 4; outputrate = 40; }\n"
             "vcm ANALYSIS { type = vcmWrite; outputrate = 100; }\n"
             "writeCharmm ANALYSIS { type = subsetWrite; outputrate = 1000; }\n"
             "kd ANALYSIS { type = KINETICENERGYDISTN; eval_rate = 10; outputrate = 100; distGroups = wDist; }\n"
             "wDist BIN { species = WxW; emin = 0 eV; emax = 0.2 eV; nBins = 100; }\n"
             "rdf ANALYSIS { type = PAIRCORRELATION; eval_rate = 10; outputrate = 50; delta_r = 0.1 Angstrom; length = 100; }\n"
             "zden ANALYSIS { type = zdensity; outputrate = 200; nz = 64; smearRadius = 1 Angstrom; smearMethod = hat; }\n")
    vaf, vcm, other, kd, rdf, zden = _load(tmp_path, extra)
    assert vaf == {"name": "vaf", "type": "VELOCITYAUTOCORRELATION", "eval_rate": 5, "outputrate": 40, "supported": True, "filename": "vaf.dat", "length": 4}
    assert vcm == {"name": "vcm", "type": "vcmWrite", "eval_rate": 0, "outputrate": 100, "supported": True, "filename": "vcm.data", "length": 1}
    assert other == {"name": "writeCharmm", "type": "subsetWrite", "eval_rate": 0, "outputrate": 1000, "supported": False}
    assert rdf == {"name": "rdf", "type": "PAIRCORRELATION", "eval_rate": 10, "outputrate": 50, "supported": True, "filename": "paircorrelation.dat",
                   "length": 100, "delta_r": rdf["delta_r"], "rmin": 0.0, "rscale": "normal", "method": "geom"}
    assert zden == {"name": "zden", "type": "zdensity", "eval_rate": 0, "outputrate": 200, "supported": True, "filename": "zden.dat", "length": 1,
                    "nz": 64, "smear_radius": zden["smear_radius"], "smear_method": "hat"}
    ang = units_convert(1.0, "Angstrom", None)
    assert abs(rdf["delta_r"] - 0.1 * ang) < 1e-15 and abs(zden["smear_radius"] - ang) < 1e-15
    assert kd["supported"] and sorted(kd) == sorted(["name", "type", "eval_rate", "outputrate", "supported", "filename", "length", "dist_groups"])
    assert [g["name"] for g in kd["dist_groups"]] == ["wDist"]

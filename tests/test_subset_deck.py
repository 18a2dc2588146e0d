"""CPU tests: the deck loader reads ANALYSIS objects of the type subsetWrite | subset_write (whole name, any case; analysis.c:170-171)
whose format is binaryCharmm (a case-sensitive comparison, subsetWrite.c:175) -- keys, defaults and units of subsetWrite_parms
(subsetWrite.c:72-139), and the refusals that stand where the reference crashes -- and leaves every other subsetWrite object, the
default format pio among them, exactly as unsupported as before.

The pinfo range beyond 4 bytes (the reference's assert, subsetWrite.c:419) needs groups x species >= 2^32, which no deck of a size
that can be committed reaches; that refusal is tested on the check itself in test_subset_host.py."""
import os
import shutil

import pytest

from ddcmd_amd.deck import load_deck, units_convert

HERE = os.path.dirname(os.path.abspath(__file__))
WATER = os.path.join(HERE, "golden", "water_deck")      # species WxW and WFxWF
SIM = "simulate SIMULATE { analysis = w; }\n"
GID_MAX = 2 ** 64 - 1


def _load(tmp_path, extra):
    d = tmp_path / "deck"
    if not d.exists():
        shutil.copytree(WATER, str(d))
    return load_deck(str(d / "object.data"), extra_objects=extra)


def _unsupported(word, outputrate):
    return {"name": "w", "type": word, "eval_rate": 0, "outputrate": outputrate, "supported": False}


def test_defaults(tmp_path):
    s = _load(tmp_path, SIM + "w ANALYSIS { type = subsetWrite; format = binaryCharmm; outputrate = 10; }\n")
    (d,) = s.analysis
    # the bounds the deck leaves out: -+ the longest box edge through "%e" in the external length unit, -+ DBL_MAX likewise (subsetWrite.c:119-139)
    big = units_convert(float("%e" % units_convert(max(s.h[0], s.h[4], s.h[8]), None, "l")), "l", None)
    vbig = units_convert(float("%e" % 1.7976931348623157e308), "l/t", None)
    assert d == {"name": "w", "type": "subsetWrite", "eval_rate": 0, "outputrate": 10, "supported": True, "filename": "subset", "length": 1,
                 "format": "binaryCharmm", "length_unit": "Ang", "modulus": 1, "odd": 0, "nfiles": 0, "idmin": 0, "idmax": GID_MAX, "id_list": None,
                 "species": None, "rmin": [-big] * 3, "rmax": [big] * 3, "vmin": [-vbig] * 3, "vmax": [vbig] * 3}
    assert big >= max(s.h[0], s.h[4], s.h[8]) * (1 - 1e-6) and vbig > 1e300


def test_every_key_with_its_unit(tmp_path):
    body = ("type = subsetWrite; format = binaryCharmm; outputrate = 50; filename = po4; lengthUnit = nm; modulus = 3; odd = 1; idmin = 7; idmax = 4294967296000; "
            "idList = 30 4294967296 5 5; species = WFxWF; nfiles = 4; xmin = -1 Ang; xmax = 2.5 Ang; ymin = -0.3 nm; ymax = 0.4 nm; zmin = -7; zmax = 8 bohr; "
            "vxmin = -0.001 Ang/fs; vxmax = 0.002 Ang/fs; vymin = -0.003; vymax = 0.004; vzmin = -5e-4 bohr/fs; vzmax = 6e-4 bohr/fs;")
    (d,) = _load(tmp_path, SIM + "w ANALYSIS { %s }\n" % body).analysis
    ang, vel = units_convert(1.0, "Ang", None), units_convert(1.0, "Ang/fs", None)
    assert d["supported"] and d["filename"] == "po4" and d["length_unit"] == "nm" and d["outputrate"] == 50
    assert (d["modulus"], d["odd"], d["idmin"], d["idmax"], d["nfiles"]) == (3, 1, 7, 4294967296000, 4)
    assert d["id_list"] == [5, 5, 30, 4294967296]      # sorted, as the reference's qsort leaves it
    assert d["species"] == ["WFxWF"]
    want_r = ([-1 * ang, -3 * ang, -7 * units_convert(1.0, "l", None)], [2.5 * ang, 4 * ang, 8 * units_convert(1.0, "bohr", None)])
    want_v = ([-0.001 * vel, -0.003 * units_convert(1.0, "l/t", None), -5e-4 * units_convert(1.0, "bohr/fs", None)],
              [0.002 * vel, 0.004 * units_convert(1.0, "l/t", None), 6e-4 * units_convert(1.0, "bohr/fs", None)])
    for got, want in ((d["rmin"], want_r[0]), (d["rmax"], want_r[1]), (d["vmin"], want_v[0]), (d["vmax"], want_v[1])):
        assert got == pytest.approx(want, rel=1e-14, abs=0)


def test_a_bound_that_is_given_leaves_the_others_at_their_defaults(tmp_path):
    s = _load(tmp_path, SIM + "w ANALYSIS { type = subsetWrite; format = binaryCharmm; outputrate = 1; zmax = 0; vxmin = 0; }\n")
    (d,) = s.analysis
    assert d["rmax"][2] == 0.0 and d["vmin"][0] == 0.0
    assert d["rmax"][0] == d["rmax"][1] == -d["rmin"][0] == -d["rmin"][2] > 0 and d["vmax"][0] == -d["vmin"][1] > 1e300


def test_an_empty_id_list_is_a_list(tmp_path):
    (d,) = _load(tmp_path, SIM + "w ANALYSIS { type = subsetWrite; format = binaryCharmm; outputrate = 1; idList = ; }\n").analysis
    assert d["supported"] and d["id_list"] == []


@pytest.mark.parametrize("word", ["subsetWrite", "subset_write", "SUBSETWRITE", "sUbSeT_wRiTe", "subsetwrite"])
def test_the_whole_name_matches_in_any_case(tmp_path, word):
    (d,) = _load(tmp_path, SIM + "w ANALYSIS { type = %s; format = binaryCharmm; outputrate = 5; }\n" % word).analysis
    assert d["supported"] and d["type"] == word and d["format"] == "binaryCharmm"


@pytest.mark.parametrize("word", ["subsetWriteFoo", "subsetWrit", "subset", "subset_writes", "xsubsetWrite"])
def test_other_words_do_not_match(tmp_path, word):
    (d,) = _load(tmp_path, SIM + "w ANALYSIS { type = %s; format = binaryCharmm; outputrate = 5; }\n" % word).analysis
    assert d == _unsupported(word, 5)


@pytest.mark.parametrize("fmt", ["", "format = pio;", "format = ovito;", "format = BinaryCharmm;", "format = binarycharmm;", "format = binaryCharmm2;", "format = ;"])
@pytest.mark.parametrize("word", ["subsetWrite", "subset_write"])
def test_every_other_format_stays_exactly_as_unsupported_as_before(tmp_path, word, fmt):
    """no format key is pio: the five-key dict, whatever else the object says -- a modulus the supported format refuses included"""
    (d,) = _load(tmp_path, SIM + "w ANALYSIS { type = %s; %s outputrate = 10000; modulus = 0; species = nosuch; }\n" % (word, fmt)).analysis
    assert d == _unsupported(word, 10000)


@pytest.mark.parametrize("body,message", [
    ("modulus = 0;", r"ANALYSIS w: modulus = 0, it must be at least 1"),
    ("modulus = -2;", r"ANALYSIS w: modulus = -2, it must be at least 1"),
    ("species = WxW nosuch;", r"ANALYSIS w: species = nosuch, and the system has no species of that name"),
])
def test_refusals(tmp_path, body, message):
    with pytest.raises(RuntimeError, match=message):
        _load(tmp_path, SIM + "w ANALYSIS { type = subsetWrite; format = binaryCharmm; outputrate = 10; %s }\n" % body)


def test_the_order_of_a_list_is_kept(tmp_path):
    extra = ("simulate SIMULATE { analysis = a w b c; }\n"
             "a ANALYSIS { type = zdensity; nz = 4; outputrate = 10; }\n"
             "w ANALYSIS { type = subsetWrite; format = binaryCharmm; outputrate = 10; modulus = 2; }\n"
             "b ANALYSIS { type = subsetWrite; outputrate = 10; }\n"
             "c ANALYSIS { type = vcmWrite; outputrate = 10; }\n")
    an = _load(tmp_path, extra).analysis
    assert [(d["name"], d["supported"]) for d in an] == [("a", True), ("w", True), ("b", False), ("c", True)]
    assert an[1]["modulus"] == 2 and an[2] == {"name": "b", "type": "subsetWrite", "eval_rate": 0, "outputrate": 10, "supported": False}


def test_the_shipped_waterbox_deck_still_loads():
    """its writeCharmm object asks for binaryCharmm (object.data:104); the SIMULATE object's analysis line is commented out as shipped"""
    ref = os.path.join(HERE, "golden", "ref_waterbox", "object.data")
    s = load_deck(ref)
    assert s.analysis == []
    (d,) = load_deck(ref, extra_objects="simulate SIMULATE { analysis = writeCharmm; }\n").analysis
    assert d["supported"] and d["outputrate"] == 10000 and d["format"] == "binaryCharmm" and d["filename"] == "subset" and d["species"] is None
